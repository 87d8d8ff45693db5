"""sgm unCLIP keyframe path — host mirror of the pieces ``utils.unclip_recon`` (utils.py:302-350) drives:

  NativeSGMUNet            ~ sgm.modules.diffusionmodules.openaimodel.UNetModel (:472; forward :816-853) behind
                             OpenAIWrapper (wrappers.py:23-34); every FLOP runs in libneurons_amd.so
  LegacyDDPMDiscretization ~ discretizer.py:42-69 (+ make_beta_schedule util.py:20-33, append_zero sgm/util.py:188)
  NativeOpenAIWrapper      ~ wrappers.py:23-34: ``model(x, t, {"crossattn":…, "vector":…})``
  DiscreteDenoiser         ~ denoiser.py:23-75 with EpsScaling denoiser_scaling.py:29-37: ``denoiser(network, x, sigma, cond)``
  EulerEDMSampler          ~ sampling.py:41-62,98-135,216-220 with VanillaCFG guiders.py:24-42: ``sampler(denoiser_fn, x, cond=, uc=)``;
                             on a native denoiser the per-element update (c_out/c_skip, CFG, to_d, Euler step) is the HIP kernel
                             nr_edm_cfg_euler_step; a foreign closure gets the reference's loop, statement for statement
  DPMPP2MSampler           ~ sampling.py:292-367 with VanillaCFG: the second-order multistep sampler on the same loop and table, opt-in; its
                             per-element update is the HIP kernel nr_edm_cfg_dpmpp2m_step (coefficients: dpmpp2m_coefficients)
  NativeDiffusionEngine    ~ sgm/models/diffusion.py DiffusionEngine, the attributes utils.unclip_recon (utils.py:302-350) and
                             recon_keyframe_neurons_enhance.py:300-324 touch: the drop-in boundary of the keyframe path
  unclip_sample            ~ the sampling part of utils.unclip_recon (:308-340), on explicit z / noise tensors; ``init`` / ``strength``
                             start it from an image instead of pure noise (the img2img reading of utils.py:308)
  Img2ImgDiscretizationWrapper, do_img2img
                           ~ sgm/inference/helpers.py:77-98,243-305: the pruned sigma table and the img2img call; the noised start
                             (posterior sample, offset noise, sigma0, 1 / sqrt(1 + sigma0^2)) is the HIP kernel nr_edm_img2img_start
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .unet3d import _on_device, _NativeNet, _ff_keys


@dataclass
class SGMUNetConfig:
    """generative_models/configs/unclip6.yaml:47-63 (network_config.params)."""
    in_channels: int = 4
    out_channels: int = 4
    model_channels: int = 320
    num_res_blocks: int = 2
    attention_resolutions: Tuple[int, ...] = (4, 2)
    channel_mult: Tuple[int, ...] = (1, 2, 4)
    num_head_channels: int = 64
    transformer_depth: Tuple[int, ...] = (1, 2, 10)
    context_dim: int = 1664
    adm_in_channels: int = 1024
    num_classes: str = "sequential"
    use_linear_in_transformer: bool = True
    norm_num_groups: int = 32        # GroupNorm32 (diffusionmodules/util.py:274-276), eps 1e-5


def _sgm_levels(cfg: SGMUNetConfig):
    chans = [m * cfg.model_channels for m in cfg.channel_mult]
    attn = [(2 ** i) in cfg.attention_resolutions for i in range(len(chans))]
    return chans, attn


def sgm_c_config(cfg: SGMUNetConfig) -> _lib.NrNetConfig:
    if cfg.num_classes != "sequential" or not cfg.use_linear_in_transformer:
        raise NotImplementedError("only the unclip6.yaml variant (num_classes='sequential', linear proj in/out) is built")
    if len(cfg.channel_mult) > _lib.NR_MAX_LEVELS:
        raise ValueError("too many levels")
    chans, attn = _sgm_levels(cfg)
    c = _lib.NrNetConfig()
    c.kind = _lib.NR_KIND_SGM_UNET
    c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
    c.num_levels = len(chans)
    depth = list(cfg.transformer_depth) if not isinstance(cfg.transformer_depth, int) else [cfg.transformer_depth] * len(chans)
    for i, ch in enumerate(chans):
        c.block_out_channels[i] = ch
        c.down_block_has_attn[i] = 1 if attn[i] else 0
        c.up_block_has_attn[i] = 1 if attn[i] else 0
        c.transformer_depth[i] = depth[i]
    c.layers_per_block = cfg.num_res_blocks
    c.num_heads = 0
    c.num_head_channels = cfg.num_head_channels
    c.cross_attention_dim = cfg.context_dim
    c.norm_num_groups = cfg.norm_num_groups
    c.norm_eps = 1e-5
    c.adm_in_channels = cfg.adm_in_channels
    return c


def _sgm_res_keys(p, cin, cout, temb):
    k = {f"{p}.in_layers.0.weight": (cin,), f"{p}.in_layers.0.bias": (cin,), f"{p}.in_layers.2.weight": (cout, cin, 3, 3),
         f"{p}.in_layers.2.bias": (cout,), f"{p}.emb_layers.1.weight": (cout, temb), f"{p}.emb_layers.1.bias": (cout,),
         f"{p}.out_layers.0.weight": (cout,), f"{p}.out_layers.0.bias": (cout,), f"{p}.out_layers.3.weight": (cout, cout, 3, 3),
         f"{p}.out_layers.3.bias": (cout,)}
    if cin != cout:
        k[f"{p}.skip_connection.weight"] = (cout, cin, 1, 1)
        k[f"{p}.skip_connection.bias"] = (cout,)
    return k


def _sgm_st_keys(p, c, ctx, depth):
    k = {f"{p}.norm.weight": (c,), f"{p}.norm.bias": (c,), f"{p}.proj_in.weight": (c, c), f"{p}.proj_in.bias": (c,),
         f"{p}.proj_out.weight": (c, c), f"{p}.proj_out.bias": (c,)}
    for d in range(depth):
        b = f"{p}.transformer_blocks.{d}"
        for n in ("norm1", "norm2", "norm3"):
            k[f"{b}.{n}.weight"] = (c,)
            k[f"{b}.{n}.bias"] = (c,)
        for a, kd in (("attn1", c), ("attn2", ctx)):
            k[f"{b}.{a}.to_q.weight"] = (c, c)
            k[f"{b}.{a}.to_k.weight"] = (c, kd)
            k[f"{b}.{a}.to_v.weight"] = (c, kd)
            k[f"{b}.{a}.to_out.0.weight"] = (c, c)
            k[f"{b}.{a}.to_out.0.bias"] = (c,)
        k.update(_ff_keys(f"{b}.ff", c))
    return k


def sgm_state_dict_schema(cfg: SGMUNetConfig) -> Dict[str, tuple]:
    """Parameter names / shapes of the reference ``UNetModel.state_dict()`` (construction order openaimodel.py:640-813)."""
    chans, attn = _sgm_levels(cfg)
    L = len(chans)
    mc, temb, ctx = cfg.model_channels, 4 * cfg.model_channels, cfg.context_dim
    depth = list(cfg.transformer_depth)
    k = {"time_embed.0.weight": (temb, mc), "time_embed.0.bias": (temb,), "time_embed.2.weight": (temb, temb), "time_embed.2.bias": (temb,),
         "label_emb.0.0.weight": (temb, cfg.adm_in_channels), "label_emb.0.0.bias": (temb,),
         "label_emb.0.2.weight": (temb, temb), "label_emb.0.2.bias": (temb,),
         "input_blocks.0.0.weight": (mc, cfg.in_channels, 3, 3), "input_blocks.0.0.bias": (mc,)}
    idx, ch = 1, mc
    skip_chans = [mc]
    for lev in range(L):
        for _ in range(cfg.num_res_blocks):
            k.update(_sgm_res_keys(f"input_blocks.{idx}.0", ch, chans[lev], temb))
            ch = chans[lev]
            if attn[lev]:
                k.update(_sgm_st_keys(f"input_blocks.{idx}.1", ch, ctx, depth[lev]))
            skip_chans.append(ch)
            idx += 1
        if lev != L - 1:
            k[f"input_blocks.{idx}.0.op.weight"] = (ch, ch, 3, 3)
            k[f"input_blocks.{idx}.0.op.bias"] = (ch,)
            skip_chans.append(ch)
            idx += 1
    k.update(_sgm_res_keys("middle_block.0", ch, ch, temb))
    k.update(_sgm_st_keys("middle_block.1", ch, ctx, depth[-1]))
    k.update(_sgm_res_keys("middle_block.2", ch, ch, temb))
    idx = 0
    for lev in reversed(range(L)):
        for i in range(cfg.num_res_blocks + 1):
            ich = skip_chans.pop()
            k.update(_sgm_res_keys(f"output_blocks.{idx}.0", ch + ich, chans[lev], temb))
            ch = chans[lev]
            sub = 1
            if attn[lev]:
                k.update(_sgm_st_keys(f"output_blocks.{idx}.1", ch, ctx, depth[lev]))
                sub = 2
            if lev and i == cfg.num_res_blocks:
                k[f"output_blocks.{idx}.{sub}.conv.weight"] = (ch, ch, 3, 3)
                k[f"output_blocks.{idx}.{sub}.conv.bias"] = (ch,)
            idx += 1
    k["out.0.weight"] = (ch,)
    k["out.0.bias"] = (ch,)
    k["out.2.weight"] = (cfg.out_channels, mc, 3, 3)
    k["out.2.bias"] = (cfg.out_channels,)
    return k


def sgm_random_state_dict(cfg: SGMUNetConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights (zero-initialised layers of the reference — out conv, proj_out, ResBlock out conv —
    are randomised so every path is numerically visible)."""
    from .synth import randn
    sd = {}
    for name, shape in sgm_state_dict_schema(cfg).items():
        z = randn(name, shape, seed)
        if name.endswith(".bias"):
            is_norm = ".norm" in name or "in_layers.0" in name or "out_layers.0" in name or name.startswith("out.0")
            t = (0.1 if is_norm else 0.02) * z
        elif len(shape) == 1:
            t = 1.0 + 0.1 * z
        else:
            t = z / (int(np.prod(shape[1:])) ** 0.5)
        sd[name] = t
    return sd


class NativeSGMUNet(_NativeNet):
    """``network(x * c_in, c_noise, cond)`` of denoiser.py:36-39: call as ``net(x, timesteps, context=..., y=...)``."""
    _kind = _lib.NR_KIND_SGM_UNET
    _config_cls = SGMUNetConfig

    def _build_cconf(self, config):
        return sgm_c_config(config)

    def _build_schema(self, config):
        return sgm_state_dict_schema(config)

    def _on_plan(self):
        b, f, h, w, L = self._plan_key
        dev = self.device
        self._io_x = torch.empty(b, self.config.in_channels, h, w, dtype=torch.float32, device=dev)
        self._io_ctx = torch.empty(b, L, self.config.context_dim, dtype=torch.float32, device=dev)
        self._io_y = torch.empty(b, self.config.adm_in_channels, dtype=torch.float32, device=dev)
        self._io_out = torch.empty(b, self.config.out_channels, h, w, dtype=torch.float32, device=dev)

    @_on_device
    def forward(self, x, timesteps=None, context=None, y=None, in_scale: float = 1.0, **kwargs):
        if kwargs:
            raise NotImplementedError(f"unsupported arguments {sorted(kwargs)}")
        if (y is None) or (context is None) or (timesteps is None):
            raise AssertionError("must specify y if and only if the model is class-conditional")   # openaimodel.py:832-834
        if not x.is_cuda:
            raise RuntimeError("NativeSGMUNet.forward: CUDA (ROCm) tensors required; there is no CPU fallback")
        b, c, h, w = x.shape
        if y.shape[0] != b or context.shape[0] != b:
            raise AssertionError("batch mismatch")                                                    # :840
        self._ensure_plan(b, 1, h, w, context.shape[1])
        self._io_x.copy_(x)
        self._set_context(context)
        self._io_y.copy_(y)
        ts = self._timesteps_host(timesteps, b)
        lib = _lib.load()
        _lib.check(lib.nr_sgm_unet_forward(self._h, torch.cuda.current_stream().cuda_stream, self._io_x.data_ptr(),
                                           float(in_scale), ts, self._io_ctx.data_ptr(), context.shape[1],
                                           self._io_y.data_ptr(), self._io_out.data_ptr()))
        return self._io_out.clone()

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------
# sampler-side host logic (scalars / tables only)
# ---------------------------------------------------------------------------------------------------------
class LegacyDDPMDiscretization:
    def __init__(self, linear_start=0.00085, linear_end=0.0120, num_timesteps=1000):
        self.num_timesteps = num_timesteps
        # make_beta_schedule("linear"): linspace in sqrt(beta), float64 (diffusionmodules/util.py:20-33) — SURVEY F12
        betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, num_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas, axis=0)

    def get_sigmas(self, n):
        if n < self.num_timesteps:
            timesteps = np.linspace(self.num_timesteps - 1, 0, n, endpoint=False).astype(int)[::-1]   # discretizer.py:11-14
            ac = self.alphas_cumprod[timesteps]
        elif n == self.num_timesteps:
            ac = self.alphas_cumprod
        else:
            raise ValueError
        sigmas = torch.tensor((1 - ac) / ac, dtype=torch.float32) ** 0.5
        return torch.flip(sigmas, (0,))

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        sigmas = self.get_sigmas(n)
        if do_append_zero:
            sigmas = torch.cat([sigmas, sigmas.new_zeros([1])])                                       # sgm/util.py:188-189
        sigmas = sigmas if not flip else torch.flip(sigmas, (0,))
        return sigmas.to(device)


class Img2ImgDiscretizationWrapper:
    """``Img2ImgDiscretizationWrapper`` (sgm/inference/helpers.py:77-98): wraps a discretization and keeps the LAST
    ``max(int(strength * len(sigmas)), 1)`` entries of whatever it returns (appended zero included), so the sampler starts part-way down the
    schedule.  ``strength = 1`` hands the wrapped table through; ``strength = 0`` leaves the one-entry table ``[0]``: no step at all.  The
    pruned table is a suffix of the full one, so a native network meets only (sigma, c_in) values the full schedule has too."""

    def __init__(self, discretization, strength: float = 1.0):
        self.discretization = discretization
        self.strength = strength
        assert 0.0 <= self.strength <= 1.0

    def __call__(self, *args, **kwargs):
        sigmas = self.discretization(*args, **kwargs)          # large first, then decreasing
        keep = max(int(self.strength * len(sigmas)), 1)
        if keep >= len(sigmas):
            return sigmas
        sigmas = torch.flip(sigmas, (0,))
        sigmas = sigmas[:keep]
        return torch.flip(sigmas, (0,))


def _unwrapped_discretization(discretization):
    while isinstance(discretization, Img2ImgDiscretizationWrapper):
        discretization = discretization.discretization
    return discretization


class EpsScaling:
    """denoiser_scaling.py:29-37: (c_skip, c_out, c_in, c_noise) = (1, -sigma, 1 / sqrt(sigma^2 + 1), sigma)."""

    def __call__(self, sigma: torch.Tensor):
        c_skip = torch.ones_like(sigma, device=sigma.device)
        c_out = -sigma
        c_in = 1 / (sigma ** 2 + 1.0) ** 0.5
        c_noise = sigma.clone()
        return c_skip, c_out, c_in, c_noise


def append_dims(x: torch.Tensor, target_dims: int) -> torch.Tensor:
    """sgm/util.py:192-199."""
    dims_to_append = target_dims - x.ndim
    if dims_to_append < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x[(...,) + (None,) * dims_to_append]


class DiscreteDenoiser:
    """``DiscreteDenoiser`` (denoiser.py:42-75) with ``EpsScaling``: callable exactly like the reference module —
    ``denoiser(network, input, sigma, cond)`` with a per-sample ``sigma`` tensor (``Denoiser.forward`` :23-39) — plus the host-scalar
    view (``scalars``) the fused sampler path uses.  ``network`` is any callable ``network(x, c_noise, cond_dict)``; when it is a
    ``NativeOpenAIWrapper`` and the batch shares one sigma (always the case under the EDM sampler) ``c_in`` rides into the HIP
    boundary conv as ``in_scale`` instead of a separate elementwise pass."""

    def __init__(self, num_idx=1000, discretization: Optional[LegacyDDPMDiscretization] = None, do_append_zero=False,
                 quantize_c_noise=True, flip=True):
        self.discretization = discretization or LegacyDDPMDiscretization()
        self.sigmas = self.discretization(num_idx, do_append_zero=do_append_zero, flip=flip)     # ascending table (flip=True)
        self.quantize_c_noise = quantize_c_noise
        self.num_idx = num_idx
        self.scaling = EpsScaling()
        self._sig_dev = {}

    # ---- reference tensor surface (denoiser.py:61-75) ----
    def _table(self, device):
        t = self._sig_dev.get(device)
        if t is None:
            t = self._sig_dev[device] = self.sigmas.to(device)
        return t

    def sigma_to_idx(self, sigma):
        if not torch.is_tensor(sigma):
            return int((torch.as_tensor(sigma, dtype=torch.float32) - self.sigmas).abs().argmin())
        dists = sigma - self._table(sigma.device)[:, None]
        return dists.abs().argmin(dim=0).view(sigma.shape)

    def idx_to_sigma(self, idx):
        return self._table(idx.device)[idx] if torch.is_tensor(idx) else self.sigmas[idx]

    def possibly_quantize_sigma(self, sigma):
        return self.idx_to_sigma(self.sigma_to_idx(sigma))

    def possibly_quantize_c_noise(self, c_noise):
        return self.sigma_to_idx(c_noise) if self.quantize_c_noise else c_noise

    def forward(self, network, input: torch.Tensor, sigma: torch.Tensor, cond: Dict, **additional_model_inputs) -> torch.Tensor:
        sigma = self.possibly_quantize_sigma(sigma)
        sigma_shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = self.possibly_quantize_c_noise(c_noise.reshape(sigma_shape))
        if isinstance(network, NativeOpenAIWrapper) and not additional_model_inputs and bool((sigma == sigma.reshape(-1)[0]).all()):
            net = network(input, c_noise, cond, in_scale=float(c_in.reshape(-1)[0]))
        else:
            net = network(input * c_in, c_noise, cond, **additional_model_inputs)
        return net * c_out + input * c_skip

    __call__ = forward

    # ---- host scalars for the fused HIP update (nr_edm_cfg_euler_step) ----
    def scalars(self, sigma: float):
        """-> (sigma_quantised, c_in, c_noise index)"""
        idx = self.sigma_to_idx(float(sigma))
        sq = float(self.sigmas[idx])
        c_in = float(1.0 / (torch.tensor(sq, dtype=torch.float32) ** 2 + 1.0) ** 0.5)
        return sq, c_in, idx


class VanillaCFG:
    """guiders.py:24-42."""

    def __init__(self, scale: float):
        self.scale = scale

    def __call__(self, x: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
        x_u, x_c = x.chunk(2)
        return x_u + self.scale * (x_c - x_u)

    def prepare_inputs(self, x, s, c, uc):
        c_out = dict()
        for k in c:
            if k in ["vector", "crossattn", "concat"]:
                c_out[k] = torch.cat((uc[k], c[k]), 0)
            else:
                assert c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


class NativeOpenAIWrapper:
    """``OpenAIWrapper`` (wrappers.py:23-34) around a ``NativeSGMUNet``: ``model(x, t, c_dict)`` with the conditioning under the
    keys ``crossattn`` / ``vector`` (an empty or absent ``concat`` is accepted, a non-empty one is not on the NEURONS path)."""

    def __init__(self, diffusion_model: "NativeSGMUNet", compile_model: bool = False):
        self.diffusion_model = diffusion_model

    def forward(self, x: torch.Tensor, t: torch.Tensor, c: dict, **kwargs) -> torch.Tensor:
        cc = c.get("concat", None)
        if cc is not None and cc.numel() > 0:
            raise NotImplementedError("'concat' conditioning is not used by unclip6.yaml")
        return self.diffusion_model(x, timesteps=t, context=c.get("crossattn", None), y=c.get("vector", None), **kwargs)

    __call__ = forward

    def to(self, device=None, dtype=None):
        self.diffusion_model.to(device)
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())


def _canonical_denoiser(engine):
    def denoiser(x, sigma, c):
        return engine.denoiser(engine.model, x, sigma, c)
    return denoiser


def _closure_engine(fn):
    """The object ``fn`` closes over IF ``fn`` is, instruction for instruction, the one-liner utils.unclip_recon builds (utils.py:337-338)::

        def denoiser(x, sigma, c):
            return diffusion_engine.denoiser(diffusion_engine.model, x, sigma, c)

    i.e. a plain function of three positional arguments with ONE free variable whose bytecode, attribute names and constants equal the
    canonical closure's (variable names do not enter the bytecode).  Anything else -- a closure that post-processes the output, passes
    additional inputs, changes cond or sigma, a bound method, a functools.partial -- returns None and takes the sampler's generic path,
    which calls it as the reference's loop does."""
    import types
    if not isinstance(fn, types.FunctionType) or fn.__defaults__ or fn.__kwdefaults__:
        return None
    cells = fn.__closure__ or ()
    if len(cells) != 1:
        return None
    ref = _canonical_denoiser(None).__code__
    c = fn.__code__
    if (c.co_code != ref.co_code or c.co_names != ref.co_names or c.co_consts != ref.co_consts or c.co_argcount != 3 or
            c.co_kwonlyargcount != 0 or c.co_flags != ref.co_flags or len(c.co_freevars) != 1 or c.co_nlocals != ref.co_nlocals):
        return None
    try:
        return cells[0].cell_contents
    except ValueError:
        return None


class _GuidedSampler:
    """``BaseDiffusionSampler`` (sampling.py:21-62) + ``VanillaCFG``, and what the native samplers share on top of it: the recognition of a native
    denoiser and the entry of the fused path.  A subclass supplies ``_fused_loop`` (HIP) and ``_generic_loop`` (the reference's loop in torch)."""

    def __init__(self, num_steps, scale, discretization, verbose, device):
        self.num_steps = num_steps
        self.guider = VanillaCFG(scale)
        self.discretization = discretization or LegacyDDPMDiscretization()
        # host scalars of the fused path: the 1000-entry table the network is evaluated on, never an img2img-pruned one
        self.denoiser = DiscreteDenoiser(discretization=_unwrapped_discretization(self.discretization))
        self.verbose = verbose
        self.device = device
        self._engine = None          # set by NativeDiffusionEngine: lets the sampler recognise the engine's own denoiser closure

    @property
    def scale(self):
        return self.guider.scale

    @scale.setter
    def scale(self, v):
        self.guider.scale = v

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps, device=x.device)
        uc = cond if uc is None else uc
        x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)                                                   # sampling.py:52
        num_sigmas = len(sigmas)
        s_in = x.new_ones([x.shape[0]])
        return x, s_in, sigmas, num_sigmas, cond, uc

    def _native_network(self, denoiser):
        """The NativeSGMUNet behind ``denoiser`` if it is one of the recognised native forms, else None."""
        if isinstance(denoiser, NativeSGMUNet):
            return denoiser
        if isinstance(denoiser, NativeOpenAIWrapper):
            return denoiser.diffusion_model
        if isinstance(denoiser, NativeDiffusionEngine):
            return denoiser.model.diffusion_model
        # opt-in tag: NativeDiffusionEngine.native_denoiser() hands out a callable carrying the engine it belongs to
        tagged = getattr(denoiser, "_nr_native", None)
        if isinstance(tagged, NativeDiffusionEngine) and tagged.is_native():
            return tagged.model.diffusion_model
        # utils.unclip_recon's own closure, recognised by its CODE (not by what it merely references): any variation of it is a
        # different function and is called through the generic loop
        obj = _closure_engine(denoiser)
        if isinstance(obj, NativeDiffusionEngine) and (self._engine is None or obj is self._engine) and obj.is_native():
            return obj.model.diffusion_model
        return None

    def __call__(self, denoiser, x, cond: Dict[str, torch.Tensor], uc: Optional[Dict[str, torch.Tensor]] = None,
                 num_steps: Optional[int] = None, **loop_args):
        network = self._native_network(denoiser)
        if network is None:            # a foreign denoiser: the reference's loop around it, on whatever device its tensors live
            return self._generic_loop(denoiser, x, cond, uc, num_steps, **loop_args)
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs the HIP kernels: CUDA (ROCm) tensors required; there is no CPU fallback")
        uc = cond if uc is None else uc
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps)
        x = (x * torch.sqrt(1.0 + sigmas[0] ** 2.0).to(x.device)).to(torch.float32).contiguous()       # sampling.py:52
        ctx = torch.cat((uc["crossattn"], cond["crossattn"]), 0)                                     # guiders.py:38 (uc first)
        vec = torch.cat((uc["vector"], cond["vector"]), 0)
        return self._fused_loop(network, x, sigmas, ctx, vec, **loop_args)


class EulerEDMSampler(_GuidedSampler):
    """``EulerEDMSampler`` (sampling.py:216-220; ``EDMSampler.__call__`` :114-135, ``sampler_step`` :98-112 with s_churn = 0 =>
    gamma = 0; ``prepare_sampling_loop`` :41-57) + ``VanillaCFG``.  Call it as the reference does::

        samples = sampler(denoiser, x, cond=c, uc=uc)        # denoiser(x, sigma, c) -> denoised      (utils.py:337-340)

    ``denoiser`` may be
      * the closure utils.unclip_recon builds around a ``NativeDiffusionEngine`` (recognised by its code: exactly
        ``engine.denoiser(engine.model, x, sigma, c)``, nothing more), ``engine.native_denoiser()`` (the explicit opt-in), a
        ``NativeDiffusionEngine`` / ``NativeOpenAIWrapper`` / ``NativeSGMUNet``: the FUSED path — the network evaluation with ``c_in`` folded
        into its boundary conv, then ONE HIP kernel (nr_edm_cfg_euler_step) for c_out / c_skip, CFG combine, to_d and the Euler update;
      * any other callable ``denoiser(x, sigma, c)``: the generic path, statement for statement the reference's loop (guider.prepare_inputs
        -> denoiser -> guider -> to_d -> euler_step) on torch tensors.  A foreign closure that routes into a native network still runs
        every network FLOP in HIP; only the per-step scalars differ in where they are applied."""

    def __init__(self, num_steps=38, scale=5.0, discretization: Optional[LegacyDDPMDiscretization] = None, s_churn=0.0, s_tmin=0.0,
                 s_tmax=float("inf"), s_noise=1.0, verbose=False, device="cuda"):
        if s_churn != 0.0:
            raise NotImplementedError("s_churn != 0 (stochastic churn) is not on the NEURONS path (unclip6.yaml sampler_config)")
        super().__init__(num_steps, scale, discretization, verbose, device)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise

    def _fused_loop(self, network, x, sigmas, ctx, vec):
        lib = _lib.load()
        n = x.numel()
        for i in range(len(sigmas) - 1):
            s, s_next = float(sigmas[i]), float(sigmas[i + 1])
            sq, c_in, idx = self.denoiser.scalars(s)
            xin = torch.cat([x] * 2)                                                                  # guiders.py:42
            net = network(xin, float(idx), context=ctx, y=vec, in_scale=c_in)
            x_new = torch.empty_like(x)
            _lib.check(lib.nr_edm_cfg_euler_step(torch.cuda.current_stream().cuda_stream, net.data_ptr(), x.data_ptr(),
                                                 x_new.data_ptr(), n, float(self.guider.scale), sq, s, s_next))
            x = x_new
        return x

    def _generic_loop(self, denoiser, x, cond, uc, num_steps):
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x.to(torch.float32), cond, uc, num_steps)
        for i in range(num_sigmas - 1):
            sigma, next_sigma = s_in * sigmas[i], s_in * sigmas[i + 1]                                # gamma = 0: sigma_hat = sigma
            denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))                      # sampling.py:59-62
            denoised = self.guider(denoised, sigma)
            d = (x - denoised) / append_dims(sigma, x.ndim)                                           # to_d, sampling_utils.py:34-35
            x = x + append_dims(next_sigma - sigma, x.ndim) * d                                       # euler_step, sampling.py:83-84
        return x


def dpmpp2m_coefficients(sigma_prev: Optional[float], sigma: float, sigma_next: float):
    """The doubles ``nr_edm_cfg_dpmpp2m_step`` forms from its (fp32) sigmas: ``x_out = c_x x + c_d den + c_o old`` is one step of
    ``DPMPP2MSampler`` (sampling.py:292-347).  With t = -log sigma, h = t_next - t, r = (t - t_prev) / h::

        c_x = sigma_next / sigma        c_d = -expm1(-h) (1 + 1 / (2 r))        c_o = expm1(-h) / (2 r)

    ``sigma_prev = None`` (the first step of a table) or ``sigma_next == 0`` (its last: sampling.py:335) is the first-order step: c_d = -expm1(-h),
    c_o = None.  At ``sigma_next == 0`` h is +inf: (0, 1, None) exactly, the step returns the denoised estimate."""
    import math
    sigma, sigma_next = float(sigma), float(sigma_next)
    if sigma_next == 0.0:
        return 0.0, 1.0, None
    h = math.log(sigma) - math.log(sigma_next)
    em = math.expm1(-h)
    c_x = sigma_next / sigma
    if sigma_prev is None:
        return c_x, -em, None
    r = (math.log(float(sigma_prev)) - math.log(sigma)) / h
    return c_x, -em * (1.0 + 1.0 / (2.0 * r)), em / (2.0 * r)


class DPMPP2MSampler(_GuidedSampler):
    """``DPMPP2MSampler`` (sampling.py:292-367; Lu et al. 2022, DPM-Solver++ 2M in sigma space) + ``VanillaCFG``: the second-order multistep
    sampler of the keyframe loop.  One network evaluation per step, as Euler; the previous step's denoised estimate is the history.  Same sigma
    table as ``EulerEDMSampler``, same call, same recognition of a native denoiser (see there):
      * FUSED path: per step the network evaluation with ``c_in`` folded into its boundary conv, then ONE HIP kernel (nr_edm_cfg_dpmpp2m_step) for
        c_out / c_skip, CFG combine and the multistep update.  The history is one fp32 buffer per call, rewritten in place; the first step of any
        table (a pruned one included) and the step to sigma = 0 are first order;
      * generic path: the reference's loop, statement for statement, its fp32 log / exp coefficient arithmetic included.
    Opt-in (``NativeDiffusionEngine(sampler="dpmpp_2m")``): how few steps keep keyframe quality is a property of the checkpoint, see DESIGN section 7.
    ``record``: a list that receives ``(x, denoised)`` clones after every step."""

    def __init__(self, num_steps=38, scale=5.0, discretization: Optional[LegacyDDPMDiscretization] = None, verbose=False, device="cuda"):
        super().__init__(num_steps, scale, discretization, verbose, device)

    def _fused_loop(self, network, x, sigmas, ctx, vec, record: Optional[list] = None):
        lib = _lib.load()
        n = x.numel()
        old = torch.empty_like(x)                     # the history: written by every step, read from the second on
        for i in range(len(sigmas) - 1):
            s_prev, s, s_next = (float(sigmas[i - 1]) if i else 0.0), float(sigmas[i]), float(sigmas[i + 1])
            sq, c_in, idx = self.denoiser.scalars(s)
            xin = torch.cat([x] * 2)                                                                  # guiders.py:42
            net = network(xin, float(idx), context=ctx, y=vec, in_scale=c_in)
            # x is this call's own tensor (the product with sqrt(1 + sigma0^2)): updated in place, as the history is
            _lib.check(lib.nr_edm_cfg_dpmpp2m_step(torch.cuda.current_stream().cuda_stream, net.data_ptr(), x.data_ptr(),
                                                   old.data_ptr() if i else None, x.data_ptr(), old.data_ptr(), n, float(self.guider.scale),
                                                   sq, s_prev, s, s_next))
            if record is not None:
                record.append((x.clone(), old.clone()))
        return x

    # ---- the reference's statements (sampling.py:293-347), on torch tensors ----
    def get_variables(self, sigma, next_sigma, previous_sigma=None):
        t, t_next = [s.log().neg() for s in (sigma, next_sigma)]                                      # to_neg_log_sigma, sampling_utils.py:38-39
        h = t_next - t
        if previous_sigma is not None:
            h_last = t - previous_sigma.log().neg()
            r = h_last / h
            return h, r, t, t_next
        return h, None, t, t_next

    def get_mult(self, h, r, t, t_next, previous_sigma):
        mult1 = t_next.neg().exp() / t.neg().exp()                                                    # to_sigma, sampling_utils.py:42-43
        mult2 = (-h).expm1()
        if previous_sigma is not None:
            mult3 = 1 + 1 / (2 * r)
            mult4 = 1 / (2 * r)
            return mult1, mult2, mult3, mult4
        return mult1, mult2

    def sampler_step(self, old_denoised, previous_sigma, sigma, next_sigma, denoiser, x, cond, uc=None):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))                          # sampling.py:59-62
        denoised = self.guider(denoised, sigma)
        h, r, t, t_next = self.get_variables(sigma, next_sigma, previous_sigma)
        mult = [append_dims(m, x.ndim) for m in self.get_mult(h, r, t, t_next, previous_sigma)]
        x_standard = mult[0] * x - mult[1] * denoised
        if old_denoised is None or torch.sum(next_sigma) < 1e-14:
            return x_standard, denoised                                                               # the first step, or all noise levels 0
        denoised_d = mult[2] * denoised - mult[3] * old_denoised
        x_advanced = mult[0] * x - mult[1] * denoised_d
        x = torch.where(append_dims(next_sigma, x.ndim) > 0.0, x_advanced, x_standard)
        return x, denoised

    def _generic_loop(self, denoiser, x, cond, uc, num_steps, record: Optional[list] = None):
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x.to(torch.float32), cond, uc, num_steps)
        old_denoised = None
        for i in range(num_sigmas - 1):
            x, old_denoised = self.sampler_step(old_denoised, None if i == 0 else s_in * sigmas[i - 1], s_in * sigmas[i], s_in * sigmas[i + 1],
                                                denoiser, x, cond, uc=uc)
            if record is not None:
                record.append((x.clone(), old_denoised.clone()))
        return x


_SAMPLERS = {"euler_edm": EulerEDMSampler, "dpmpp_2m": DPMPP2MSampler}      # NativeDiffusionEngine(sampler=)


class NativeDiffusionEngine:
    """The surface of ``sgm.models.diffusion.DiffusionEngine`` that the keyframe script and ``utils.unclip_recon`` touch
    (recon_keyframe_neurons_enhance.py:300-324,458-462; utils.py:302-350), backed by libneurons_amd.so:

        .model                 NativeOpenAIWrapper(NativeSGMUNet)        model(x, t, c_dict)                        wrappers.py:23-34
        .denoiser              DiscreteDenoiser (EpsScaling)             denoiser(model, x, sigma, c)               denoiser.py:23-75
        .sampler               EulerEDMSampler + VanillaCFG              sampler(denoiser_fn, x, cond=, uc=); .discretization(n); .num_steps
                               (``sampler="dpmpp_2m"``: DPMPP2MSampler, opt-in; a sampler object may also be assigned to ``.sampler``)
        .first_stage_model     NativeVAEDecoder                          decode_first_stage(z)                      diffusion.py:118-135
        .first_stage_encoder   NativeVAEEncoder (same ddconfig)          encode_first_stage(x[, noise])             diffusion.py:137-150
        .ema_scope()           no-op context (use_ema is False in unclip6.yaml; diffusion.py:198-210)
        .eval() / .requires_grad_() / .to(device) / .load_state_dict(ckpt["state_dict"])

    ``load_state_dict`` takes the checkpoint's key names: ``model.diffusion_model.*`` -> the U-Net, ``first_stage_model.{decoder,
    post_quant_conv}.*`` -> the decoder, ``first_stage_model.{encoder,quant_conv}.*`` -> the encoder (optional as a whole: a checkpoint
    without them loads, and only ``encode_first_stage`` then raises); ``conditioner.*`` (open_clip embedders, not called by unclip_recon),
    ``denoiser.sigmas`` (regenerated), ``first_stage_model.loss.*`` and ``model_ema.*`` are ignored."""

    def __init__(self, network_config: Optional[SGMUNetConfig] = None, first_stage_config=None, num_steps: int = 38, scale: float = 5.0,
                 scale_factor: float = 0.18215, disable_first_stage_autocast: bool = True, use_ema: bool = False, sampler: str = "euler_edm",
                 **ignored):
        from .vae import NativeVAEDecoder, NativeVAEEncoder, VAEDecoderConfig
        if sampler not in _SAMPLERS:
            raise ValueError(f"sampler must be one of {sorted(_SAMPLERS)}, got {sampler!r}")
        if use_ema:
            raise NotImplementedError("use_ema: inference checkpoints carry the EMA weights already (unclip6.yaml has no EMA)")
        self.model = NativeOpenAIWrapper(NativeSGMUNet(network_config or SGMUNetConfig()))
        self.first_stage_model = NativeVAEDecoder(first_stage_config or VAEDecoderConfig())
        self.first_stage_encoder = NativeVAEEncoder(self.first_stage_model.config)       # same ddconfig as the decoder
        disc = LegacyDDPMDiscretization()
        self.denoiser = DiscreteDenoiser(discretization=disc)
        self.sampler = _SAMPLERS[sampler](num_steps=num_steps, scale=scale, discretization=disc)
        self.sampler._engine = self
        self.scale_factor = scale_factor
        self.disable_first_stage_autocast = disable_first_stage_autocast
        self.use_ema = False
        self.conditioner = None
        self._native_denoiser, self._native_model = self.denoiser, self.model

    def native_denoiser(self):
        """The explicit opt-in to the sampler's fused HIP path: ``engine.sampler(engine.native_denoiser(), x, cond=c, uc=uc)``.  Called
        directly it is the reference's closure (utils.py:337-338)."""
        fn = _canonical_denoiser(self)
        fn._nr_native = self
        return fn

    def is_native(self):
        """False once a caller has swapped .denoiser / .model for foreign objects: the sampler then takes the generic path."""
        return self.denoiser is self._native_denoiser and self.model is self._native_model

    def ema_scope(self, context=None):
        import contextlib
        return contextlib.nullcontext()

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def to(self, device=None, dtype=None):
        self.model.to(device)
        self.first_stage_model.to(device)
        self.first_stage_encoder.to(device)
        return self

    @property
    def device(self):
        return self.model.diffusion_model.device

    def load_state_dict(self, state_dict, strict=True):
        unet_sd, vae_sd, enc_sd, ignored, unexpected = {}, {}, {}, [], []
        for k, v in state_dict.items():
            if k.startswith("model.diffusion_model."):
                unet_sd[k[len("model.diffusion_model."):]] = v
            elif k.startswith("first_stage_model."):
                kk = k[len("first_stage_model."):]
                if kk.startswith("decoder.") or kk.startswith("post_quant_conv."):
                    vae_sd[kk] = v
                elif kk.startswith("encoder.") or kk.startswith("quant_conv."):
                    enc_sd[kk] = v
                else:
                    ignored.append(k)
            elif k.startswith(("conditioner.", "denoiser.", "model_ema.", "loss_fn.")):
                ignored.append(k)
            else:
                unexpected.append(k)
        m1, u1 = self.model.diffusion_model.load_state_dict(unet_sd, strict=False)
        m2, u2 = self.first_stage_model.load_state_dict(vae_sd, strict=False)
        # the encoder half is optional as a WHOLE (a decoder-only checkpoint serves every txt2img caller); given in part, the rest is missing
        m3, u3 = self.first_stage_encoder.load_state_dict(enc_sd, strict=False) if enc_sd else ([], [])
        missing = ["model.diffusion_model." + k for k in m1] + ["first_stage_model." + k for k in m2 + m3]
        unexpected += ["model.diffusion_model." + k for k in u1] + ["first_stage_model." + k for k in u2 + u3]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for NativeDiffusionEngine:\n\tMissing key(s): {missing[:8]}"
                               f"{'...' if len(missing) > 8 else ''}\n\tUnexpected key(s): {unexpected[:8]}")
        return missing, unexpected

    @torch.no_grad()
    def decode_first_stage(self, z):
        return self.first_stage_model.decode_first_stage(z, scale_factor=self.scale_factor)

    def _encoder(self):
        if not self.first_stage_encoder._loaded:
            raise RuntimeError("NativeDiffusionEngine: the checkpoint held no first_stage_model.encoder.* / quant_conv.* tensors; "
                               "img2img from an image needs them (there is no fallback encoder)")
        return self.first_stage_encoder

    @torch.no_grad()
    def encode_first_stage_moments(self, x):
        """``first_stage_model.encoder`` -> ``quant_conv`` (autoencoder.py:468-483): x [n][3][H][W] in [-1, 1] on the GPU -> the posterior's
        fp32 moments (mean | logvar) [n][2z][H/8][W/8], what ``nr_edm_img2img_start`` reads in its moments mode."""
        return self._encoder().moments(x)

    @torch.no_grad()
    def encode_first_stage(self, x, noise: Optional[torch.Tensor] = None):
        """``DiffusionEngine.encode_first_stage`` (diffusion.py:137-150) over ``AutoencodingEngineLegacy.encode`` (autoencoder.py:468-488):
        the regularizer is ``DiagonalGaussianRegularizer`` with its default ``sample=True`` (autoencoder.py:508-520, regularizers/__init__.py:13-31),
        so the latent is a posterior SAMPLE, ``scale_factor * (mean + std * eps)``, not the mode.  ``noise`` is that eps [n][z][H/8][W/8];
        ``None`` draws it where and when the reference does: ``torch.randn(mean.shape)`` on the host from the global generator, after the encoder
        ran (distributions.py:38-42)."""
        moments = self.encode_first_stage_moments(x)
        from .vae import DiagonalGaussianDistribution
        post = DiagonalGaussianDistribution(moments)
        if noise is None:
            return post.sample(scale=self.scale_factor, host_draw=True)
        if tuple(noise.shape) != tuple(post.mean.shape):
            raise ValueError(f"noise must have the latent's shape {tuple(post.mean.shape)}, got {tuple(noise.shape)}")
        return post._draw(_f32_cuda(noise, "noise"), self.scale_factor)


def _f32_cuda(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: CUDA (ROCm) tensors required; there is no CPU fallback")
    return t.to(torch.float32).contiguous()


def edm_img2img_start(noise, sigma0: float, z: Optional[torch.Tensor] = None, moments: Optional[torch.Tensor] = None,
                      enc_noise: Optional[torch.Tensor] = None, z_scale: float = 1.0, offset: Optional[torch.Tensor] = None,
                      offset_noise_level: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The noised, pre-scaled start of sgm img2img (helpers.py:276-291) in ONE HIP launch (``nr_edm_img2img_start``):
    ``(z + (noise + level * offset[b]) * sigma0) / sqrt(1 + sigma0^2)`` with ``z`` given (skip_encode) or formed from the encoder's
    ``moments`` and the posterior draw ``enc_noise`` as ``(mean + std * enc_noise) * z_scale``.  ``out`` may be ``z`` itself."""
    if (z is None) == (moments is None):
        raise ValueError("pass exactly one of z (a latent) and moments (the encoder's output, with enc_noise)")
    noise = _f32_cuda(noise, "noise")
    n = noise.shape[0]
    nps = noise.numel() // max(n, 1)
    if z is not None:
        src = z if out is z else _f32_cuda(z, "z")
        if out is z and (not z.is_cuda or z.dtype != torch.float32 or not z.is_contiguous()):
            raise ValueError("in-place start needs a contiguous fp32 CUDA latent")
        if tuple(src.shape) != tuple(noise.shape):
            raise ValueError(f"z {tuple(src.shape)} and noise {tuple(noise.shape)} differ in shape")
        mode, eps = _lib.NR_IMG2IMG_LATENT, None
    else:
        src = _f32_cuda(moments, "moments")
        if enc_noise is None:
            raise ValueError("moments need enc_noise, the posterior draw")
        eps = _f32_cuda(enc_noise, "enc_noise")
        if src.shape[0] != n or src.numel() != 2 * noise.numel() or tuple(eps.shape) != tuple(noise.shape):
            raise ValueError(f"moments {tuple(src.shape)}, enc_noise {tuple(eps.shape)} and noise {tuple(noise.shape)} do not belong together")
        mode = _lib.NR_IMG2IMG_MOMENTS
    off = None
    if offset is not None and offset_noise_level != 0.0:
        off = _f32_cuda(offset, "offset").reshape(-1)
        if off.numel() != n:
            raise ValueError(f"offset holds one scalar per sample: expected {n}, got {off.numel()}")
    if out is None:
        out = torch.empty_like(noise)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(noise.shape):
        raise ValueError("out must be a contiguous fp32 CUDA tensor of the noise's shape")
    _lib.check(_lib.load().nr_edm_img2img_start(
        torch.cuda.current_stream().cuda_stream, src.data_ptr() if mode == _lib.NR_IMG2IMG_LATENT else None,
        src.data_ptr() if mode == _lib.NR_IMG2IMG_MOMENTS else None, eps.data_ptr() if eps is not None else None, noise.data_ptr(),
        off.data_ptr() if off is not None else None, out.data_ptr(), n, nps, float(z_scale), float(sigma0), float(offset_noise_level), mode))
    return out


def _img2img_latents(img, model, sampler, denoiser, c, uc, noise, offset_noise_level, offset, skip_encode, enc_noise):
    """helpers.py:272-296: the start (one HIP launch) and the sampler (either class: only .discretization, .num_steps and the call are touched).
    ``model`` is only needed to encode."""
    if skip_encode:
        start = dict(z=img)
    else:
        if not isinstance(model, NativeDiffusionEngine):
            raise TypeError("img2img from an image needs a NativeDiffusionEngine to encode it (or pass a latent with skip_encode)")
        moments = model.encode_first_stage_moments(img)
        if enc_noise is None:           # the reference's draw: host, global generator, after the encoder ran (distributions.py:38-42)
            n, c2, h, w = moments.shape
            enc_noise = torch.randn((n, c2 // 2, h, w)).to(moments.device)
        start = dict(moments=moments, enc_noise=enc_noise, z_scale=model.scale_factor)
    sigmas = sampler.discretization(sampler.num_steps)
    use_offset = offset_noise_level > 0.0 and offset is not None                                      # helpers.py:281
    noised_z = edm_img2img_start(noise, float(sigmas[0]), offset=offset if use_offset else None,
                                 offset_noise_level=offset_noise_level if use_offset else 0.0, **start)
    return sampler(denoiser, noised_z, cond=c, uc=uc)


@torch.no_grad()
def do_img2img(img, model: NativeDiffusionEngine, sampler: Union[EulerEDMSampler, DPMPP2MSampler], c: Dict[str, torch.Tensor], uc: Dict[str, torch.Tensor],
               noise: torch.Tensor, offset_noise_level: float = 0.0, offset: Optional[torch.Tensor] = None, skip_encode: bool = False,
               return_latents: bool = False, enc_noise: Optional[torch.Tensor] = None, filter=None):
    """``do_img2img`` (sgm/inference/helpers.py:243-305) on explicit conditioning and explicit draws.  The reference builds ``c`` / ``uc`` from
    ``model.conditioner`` (:256-270); that stays PyTorch and the caller's, so the dicts (``crossattn`` / ``vector``, one row per sample) come in
    as arguments.  ``img``: [n][3][H][W] in [-1, 1], or with ``skip_encode`` a latent [n][4][h][w].  ``noise`` [n][4][h][w] is the
    ``randn_like(z)`` of :276, ``sampler`` an EulerEDMSampler or a DPMPP2MSampler, ``offset`` (n,) the per-sample draw of :282-284 (read when ``offset_noise_level > 0``), ``enc_noise`` the posterior
    draw inside ``encode_first_stage`` (``None``: drawn as the reference draws it).  Strength is the sampler's: give it
    ``Img2ImgDiscretizationWrapper(discretization, strength)`` as its discretization.  Returns images in [0, 1] (and the latents)."""
    samples_z = _img2img_latents(img, model, sampler, model.native_denoiser(), c, uc, noise, offset_noise_level, offset, skip_encode, enc_noise)
    samples_x = model.decode_first_stage(samples_z)
    samples = torch.clamp((samples_x + 1.0) / 2.0, min=0.0, max=1.0)
    if filter is not None:
        samples = filter(samples)
    if return_latents:
        return samples, samples_z
    return samples


def unclip_sample(network, tokens, vector_suffix, z, noise, uc_tokens, sampler: Union[EulerEDMSampler, DPMPP2MSampler],
                  offset_noise: Optional[torch.Tensor] = None, offset_noise_level: float = 0.04, init: Optional[torch.Tensor] = None,
                  strength: float = 1.0, enc_noise: Optional[torch.Tensor] = None):
    """Sampling part of ``utils.unclip_recon`` (utils.py:308-340) on explicit tensors: ``tokens`` (1,256,1664) prior
    tokens x key-object mask, ``vector_suffix`` (1,1024), starting ``z`` and ``noise`` (n,4,h,w), ``uc_tokens`` the
    random unconditional tokens (:318), ``offset_noise`` (n,) the per-sample offset draw (:328-331).  ``network``: a NativeSGMUNet or
    anything else ``EulerEDMSampler.__call__`` accepts as its denoiser; ``sampler``: an EulerEDMSampler or a DPMPP2MSampler.

    img2img ("can change to VAE outputs of initial image for img2img", utils.py:308): ``init`` replaces ``z`` (which may then be None), one per
    sample: a latent (n,4,h,w), or an image (n,3,8h,8w) in [-1, 1], which ``network``, then a NativeDiffusionEngine, encodes (``enc_noise``: its
    posterior draw).  ``strength`` prunes the sampler's sigma table for this call (Img2ImgDiscretizationWrapper).  Without ``init`` and at
    ``strength == 1.0`` nothing of this is touched."""
    if init is None and strength == 1.0:
        n = z.shape[0]
        c = {"crossattn": tokens.repeat(n, 1, 1).to(z.device), "vector": vector_suffix.repeat(n, 1).to(z.device)}
        uc = {"crossattn": uc_tokens.repeat(n, 1, 1).to(z.device), "vector": vector_suffix.repeat(n, 1).to(z.device)}
        sigmas = sampler.discretization(sampler.num_steps)
        sigma = sigmas[0].to(z.device)
        if offset_noise_level > 0.0 and offset_noise is not None:
            noise = noise + offset_noise_level * offset_noise.to(z.device).reshape(-1, 1, 1, 1)
        noised_z = z + noise * sigma
        noised_z = noised_z / torch.sqrt(1.0 + sigmas[0] ** 2.0).to(z.device)
        return sampler(network, noised_z, cond=c, uc=uc)
    start = z if init is None else init
    n, dev = noise.shape[0], noise.device
    if start.shape[0] != n:
        raise ValueError(f"one init per sample: noise has {n} samples, init {start.shape[0]}")
    c = {"crossattn": tokens.repeat(n, 1, 1).to(dev), "vector": vector_suffix.repeat(n, 1).to(dev)}
    uc = {"crossattn": uc_tokens.repeat(n, 1, 1).to(dev), "vector": vector_suffix.repeat(n, 1).to(dev)}
    full = sampler.discretization
    sampler.discretization = Img2ImgDiscretizationWrapper(full, strength)
    try:
        return _img2img_latents(start, network, sampler, network, c, uc, noise, offset_noise_level, offset_noise,
                                tuple(start.shape) == tuple(noise.shape), enc_noise)
    finally:
        sampler.discretization = full

