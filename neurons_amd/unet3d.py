"""NativeUNet3D — drop-in for ``animatediff.models.unet.UNet3DConditionModel`` on the inference path.

Same constructor keywords that matter (unet.py:42-90), same ``forward`` signature and ``.sample`` output
(unet.py:320-333,472-475), ``load_state_dict`` with the reference key names, ``.in_channels``,
``.config.sample_size`` (read at pipeline_neuroclips.py:349-350,382).  Every FLOP of the forward runs in
libneurons_amd.so (C ABI ``nr_unet3d_forward``); there is no torch fallback.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


@dataclass
class UNet3DConfig:
    sample_size: Optional[int] = 64
    in_channels: int = 4
    out_channels: int = 4
    down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D")
    up_block_types: Tuple[str, ...] = ("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D")
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    cross_attention_dim: int = 768          # SD-1.5 unet/config.json (the class default 1280 is never used by NEURONS)
    attention_head_dim: int = 8             # = number of heads (diffusers naming quirk, sparse_controlnet.py:143-149)
    use_inflated_groupnorm: bool = True     # inference-v3.yaml:2 (per-frame GroupNorm)
    use_motion_module: bool = True
    motion_module_resolutions: Tuple[int, ...] = (1, 2, 4, 8)
    motion_module_mid_block: bool = False
    motion_module_type: str = "Vanilla"
    motion_module_kwargs: dict = field(default_factory=lambda: dict(
        num_attention_heads=8, num_transformer_block=1, attention_block_types=("Temporal_Self", "Temporal_Self"),
        temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1,
        zero_initialize=True))
    # SparseCtrl only
    conditioning_channels: int = 4
    set_noisy_sample_input_to_zero: bool = True
    use_simplified_condition_embedding: bool = True
    concate_conditioning_mask: bool = True
    # image-condition variant (use_simplified_condition_embedding=False): SparseControlNetConditioningEmbedding widths
    # (sparse_controlnet.py:52-56,186-190); the condition is then at 2^(len - 1) x the latent resolution
    conditioning_embedding_out_channels: Tuple[int, ...] = (16, 32, 96, 256)


@dataclass
class UNet3DConditionOutput:
    sample: torch.Tensor


def _check_supported(cfg: UNet3DConfig, kind: int):
    n = len(cfg.block_out_channels)
    if len(cfg.down_block_types) != n:
        raise ValueError("Must provide the same number of `block_out_channels` as `down_block_types`.")
    for t in cfg.down_block_types:
        if t not in ("CrossAttnDownBlock3D", "DownBlock3D"):
            raise ValueError(f"{t} does not exist.")
    if kind == _lib.NR_KIND_UNET3D:
        for t in cfg.up_block_types:
            if t not in ("CrossAttnUpBlock3D", "UpBlock3D"):
                raise ValueError(f"{t} does not exist.")
    if not cfg.use_inflated_groupnorm:
        raise NotImplementedError("only use_inflated_groupnorm=True (per-frame GroupNorm, the NEURONS v3 config) is built")
    mm = cfg.motion_module_kwargs
    if cfg.use_motion_module:
        if cfg.motion_module_type != "Vanilla":
            raise ValueError("unknown motion_module_type")
        if tuple(cfg.motion_module_resolutions) != tuple(2 ** i for i in range(n)):
            raise NotImplementedError("motion modules at every resolution only (inference-v3.yaml:4)")
        if mm.get("num_transformer_block", 1) != 1 or mm.get("temporal_attention_dim_div", 1) != 1:
            raise NotImplementedError("num_transformer_block=1, temporal_attention_dim_div=1 only")
        if any(b != "Temporal_Self" for b in mm.get("attention_block_types", ())):
            raise NotImplementedError("Temporal_Self attention blocks only")
        if not mm.get("temporal_position_encoding", False):
            raise NotImplementedError("temporal_position_encoding=True only")
    if kind == _lib.NR_KIND_SPARSECTRL:
        if not cfg.concate_conditioning_mask:
            raise NotImplementedError("SparseCtrl needs concate_conditioning_mask=True (latent_condition.yaml / image_condition.yaml)")
        if not cfg.use_simplified_condition_embedding:
            ch = tuple(cfg.conditioning_embedding_out_channels)
            ok = 1 <= len(ch) <= _lib.NR_MAX_LEVELS and ch[0] in (16, 32) and cfg.conditioning_channels + 1 <= 8 and \
                all(c in (16, 32, 64, 96, 128, 256) for c in ch)
            if not ok:
                raise NotImplementedError(f"SparseCtrl condition embedding {ch} with conditioning_channels={cfg.conditioning_channels}: "
                                          "1-4 levels, the first 16 or 32 channels, the others 16/32/64/96/128/256, at most 7 condition channels")


def condition_upscale(cfg: UNet3DConfig) -> int:
    """Condition resolution over the latent resolution: 1 for the latent-condition variant, 2 per stride-2 embedding block otherwise."""
    if cfg.use_simplified_condition_embedding:
        return 1
    return 2 ** (len(cfg.conditioning_embedding_out_channels) - 1)


def make_c_config(cfg: UNet3DConfig, kind: int) -> _lib.NrNetConfig:
    _check_supported(cfg, kind)
    c = _lib.NrNetConfig()
    c.kind = kind
    c.in_channels = cfg.in_channels
    c.out_channels = cfg.out_channels
    n = len(cfg.block_out_channels)
    c.num_levels = n
    for i in range(n):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.down_block_has_attn[i] = 1 if cfg.down_block_types[i] == "CrossAttnDownBlock3D" else 0
        if kind == _lib.NR_KIND_UNET3D:
            c.up_block_has_attn[i] = 1 if cfg.up_block_types[i] == "CrossAttnUpBlock3D" else 0
    c.layers_per_block = cfg.layers_per_block
    c.num_heads = cfg.attention_head_dim
    c.cross_attention_dim = cfg.cross_attention_dim
    c.norm_num_groups = cfg.norm_num_groups
    c.norm_eps = cfg.norm_eps
    c.use_motion_module = 1 if cfg.use_motion_module else 0
    mm = cfg.motion_module_kwargs
    c.motion_num_heads = mm.get("num_attention_heads", 8)
    c.motion_num_attention_blocks = len(mm.get("attention_block_types", ("Temporal_Self", "Temporal_Self")))
    c.motion_pe_max_len = mm.get("temporal_position_encoding_max_len", 24)
    c.motion_module_mid_block = 1 if cfg.motion_module_mid_block else 0
    c.conditioning_channels = cfg.conditioning_channels
    c.set_noisy_sample_input_to_zero = 1 if cfg.set_noisy_sample_input_to_zero else 0
    if kind == _lib.NR_KIND_SPARSECTRL and not cfg.use_simplified_condition_embedding:
        ch = tuple(cfg.conditioning_embedding_out_channels)
        c.cond_embedding_levels = len(ch)
        for i, v in enumerate(ch):
            c.cond_embedding_channels[i] = v
    return c


# ---------------------------------------------------------------------------------------------------
# state-dict schema: reference parameter names -> shapes (what nn.Module.state_dict() of the reference
# classes contains; ``pos_encoder.pe`` is a non-persistent buffer, motion_module.py:239, and is regenerated)
# ---------------------------------------------------------------------------------------------------
def _resnet_keys(p, cin, cout, temb):
    k = {f"{p}.norm1.weight": (cin,), f"{p}.norm1.bias": (cin,), f"{p}.conv1.weight": (cout, cin, 3, 3), f"{p}.conv1.bias": (cout,),
         f"{p}.time_emb_proj.weight": (cout, temb), f"{p}.time_emb_proj.bias": (cout,),
         f"{p}.norm2.weight": (cout,), f"{p}.norm2.bias": (cout,), f"{p}.conv2.weight": (cout, cout, 3, 3), f"{p}.conv2.bias": (cout,)}
    if cin != cout:
        k[f"{p}.conv_shortcut.weight"] = (cout, cin, 1, 1)
        k[f"{p}.conv_shortcut.bias"] = (cout,)
    return k


def _ff_keys(p, c):
    return {f"{p}.net.0.proj.weight": (8 * c, c), f"{p}.net.0.proj.bias": (8 * c,), f"{p}.net.2.weight": (c, 4 * c), f"{p}.net.2.bias": (c,)}


def _attn_keys(p, c, kdim):
    return {f"{p}.to_q.weight": (c, c), f"{p}.to_k.weight": (c, kdim), f"{p}.to_v.weight": (c, kdim),
            f"{p}.to_out.0.weight": (c, c), f"{p}.to_out.0.bias": (c,)}


def _transformer_keys(p, c, ctx):
    k = {f"{p}.norm.weight": (c,), f"{p}.norm.bias": (c,), f"{p}.proj_in.weight": (c, c, 1, 1), f"{p}.proj_in.bias": (c,),
         f"{p}.proj_out.weight": (c, c, 1, 1), f"{p}.proj_out.bias": (c,)}
    b = f"{p}.transformer_blocks.0"
    for n in ("norm1", "norm2", "norm3"):
        k[f"{b}.{n}.weight"] = (c,)
        k[f"{b}.{n}.bias"] = (c,)
    k.update(_attn_keys(f"{b}.attn1", c, c))
    k.update(_attn_keys(f"{b}.attn2", c, ctx))
    k.update(_ff_keys(f"{b}.ff", c))
    return k


def _motion_keys(p, c, nblocks):
    p = f"{p}.temporal_transformer"
    k = {f"{p}.norm.weight": (c,), f"{p}.norm.bias": (c,), f"{p}.proj_in.weight": (c, c), f"{p}.proj_in.bias": (c,),
         f"{p}.proj_out.weight": (c, c), f"{p}.proj_out.bias": (c,)}
    b = f"{p}.transformer_blocks.0"
    for i in range(nblocks):
        k.update(_attn_keys(f"{b}.attention_blocks.{i}", c, c))
        k[f"{b}.norms.{i}.weight"] = (c,)
        k[f"{b}.norms.{i}.bias"] = (c,)
    k.update(_ff_keys(f"{b}.ff", c))
    k[f"{b}.ff_norm.weight"] = (c,)
    k[f"{b}.ff_norm.bias"] = (c,)
    return k


def state_dict_schema(cfg: UNet3DConfig, kind: int = _lib.NR_KIND_UNET3D) -> dict:
    boc = list(cfg.block_out_channels)
    L = len(boc)
    temb = 4 * boc[0]
    ctx = cfg.cross_attention_dim
    nmm = len(cfg.motion_module_kwargs.get("attention_block_types", ())) if cfg.use_motion_module else 0
    k = {"conv_in.weight": (boc[0], cfg.in_channels, 3, 3), "conv_in.bias": (boc[0],),
         "time_embedding.linear_1.weight": (temb, boc[0]), "time_embedding.linear_1.bias": (temb,),
         "time_embedding.linear_2.weight": (temb, temb), "time_embedding.linear_2.bias": (temb,)}
    out_c = boc[0]
    for i in range(L):
        in_c, out_c = out_c, boc[i]
        for j in range(cfg.layers_per_block):
            k.update(_resnet_keys(f"down_blocks.{i}.resnets.{j}", in_c if j == 0 else out_c, out_c, temb))
            if cfg.down_block_types[i] == "CrossAttnDownBlock3D":
                k.update(_transformer_keys(f"down_blocks.{i}.attentions.{j}", out_c, ctx))
            if nmm:
                k.update(_motion_keys(f"down_blocks.{i}.motion_modules.{j}", out_c, nmm))
        if i != L - 1:
            k[f"down_blocks.{i}.downsamplers.0.conv.weight"] = (out_c, out_c, 3, 3)
            k[f"down_blocks.{i}.downsamplers.0.conv.bias"] = (out_c,)
    cm = boc[-1]
    k.update(_resnet_keys("mid_block.resnets.0", cm, cm, temb))
    k.update(_transformer_keys("mid_block.attentions.0", cm, ctx))
    if nmm and cfg.motion_module_mid_block:
        k.update(_motion_keys("mid_block.motion_modules.0", cm, nmm))
    k.update(_resnet_keys("mid_block.resnets.1", cm, cm, temb))
    if kind == _lib.NR_KIND_SPARSECTRL:
        if cfg.use_simplified_condition_embedding:
            k["controlnet_cond_embedding.weight"] = (boc[0], cfg.conditioning_channels + 1, 3, 3)
            k["controlnet_cond_embedding.bias"] = (boc[0],)
        else:                                                   # SparseControlNetConditioningEmbedding (sparse_controlnet.py:49-70)
            ch = list(cfg.conditioning_embedding_out_channels)
            p = "controlnet_cond_embedding"
            k[f"{p}.conv_in.weight"] = (ch[0], cfg.conditioning_channels + 1, 3, 3)
            k[f"{p}.conv_in.bias"] = (ch[0],)
            for i in range(len(ch) - 1):
                k[f"{p}.blocks.{2 * i}.weight"] = (ch[i], ch[i], 3, 3)
                k[f"{p}.blocks.{2 * i}.bias"] = (ch[i],)
                k[f"{p}.blocks.{2 * i + 1}.weight"] = (ch[i + 1], ch[i], 3, 3)
                k[f"{p}.blocks.{2 * i + 1}.bias"] = (ch[i + 1],)
            k[f"{p}.conv_out.weight"] = (boc[0], ch[-1], 3, 3)
            k[f"{p}.conv_out.bias"] = (boc[0],)
        chans = [boc[0]]
        for i in range(L):
            chans += [boc[i]] * cfg.layers_per_block
            if i != L - 1:
                chans.append(boc[i])
        for i, c in enumerate(chans):
            k[f"controlnet_down_blocks.{i}.weight"] = (c, c, 1, 1)
            k[f"controlnet_down_blocks.{i}.bias"] = (c,)
        k["controlnet_mid_block.weight"] = (cm, cm, 1, 1)
        k["controlnet_mid_block.bias"] = (cm,)
        return k
    rev = boc[::-1]
    out_c = rev[0]
    for i in range(L):
        prev_out, out_c = out_c, rev[i]
        in_c = rev[min(i + 1, L - 1)]
        for j in range(cfg.layers_per_block + 1):
            skip_c = in_c if j == cfg.layers_per_block else out_c
            res_in = prev_out if j == 0 else out_c
            k.update(_resnet_keys(f"up_blocks.{i}.resnets.{j}", res_in + skip_c, out_c, temb))
            if cfg.up_block_types[i] == "CrossAttnUpBlock3D":
                k.update(_transformer_keys(f"up_blocks.{i}.attentions.{j}", out_c, ctx))
            if nmm:
                k.update(_motion_keys(f"up_blocks.{i}.motion_modules.{j}", out_c, nmm))
        if i != L - 1:
            k[f"up_blocks.{i}.upsamplers.0.conv.weight"] = (out_c, out_c, 3, 3)
            k[f"up_blocks.{i}.upsamplers.0.conv.bias"] = (out_c,)
    k["conv_norm_out.weight"] = (boc[0],)
    k["conv_norm_out.bias"] = (boc[0],)
    k["conv_out.weight"] = (cfg.out_channels, boc[0], 3, 3)
    k["conv_out.bias"] = (cfg.out_channels,)
    return k


def random_state_dict(cfg: UNet3DConfig, kind: int = _lib.NR_KIND_UNET3D, seed: int = 0, zero_init_heads: bool = False) -> dict:
    """Seeded synthetic weights with a forward-stable scale (no checkpoints are available offline).

    Linear/conv weights ~ N(0, 1/fan_in); norm gains ~ 1 + 0.1 N(0,1); biases ~ 0.02 N(0,1).  The layers
    the reference zero-initialises (motion ``proj_out`` motion_module.py:74-75, ControlNet zero-convs
    sparse_controlnet.py:244-246,281-295) are random too unless ``zero_init_heads`` — otherwise the temporal
    and control paths would be numerically invisible.  Of the image-condition embedding only ``conv_out`` (weight and
    bias) is zero-initialised, as the reference's ``zero_module`` (sparse_controlnet.py:66-68)."""
    from .synth import randn
    image_embed = kind == _lib.NR_KIND_SPARSECTRL and not cfg.use_simplified_condition_embedding
    sd = {}
    for name, shape in state_dict_schema(cfg, kind).items():
        z = randn(name, shape, seed)
        if image_embed and name.startswith("controlnet_cond_embedding."):
            if name.endswith(".bias"):
                t = 0.02 * z
            else:
                t = z / (int(np.prod(shape[1:])) ** 0.5)
            if zero_init_heads and name.startswith("controlnet_cond_embedding.conv_out."):
                t = torch.zeros(shape)
        elif name.endswith(".bias"):
            is_norm = ".norm" in name or "norms." in name or "conv_norm_out" in name or "ff_norm" in name
            t = (0.1 if is_norm else 0.02) * z
        elif len(shape) == 1:
            t = 1.0 + 0.1 * z
        else:
            fan_in = int(np.prod(shape[1:]))
            t = z / (fan_in ** 0.5)
            zero = ("motion_modules" in name and ".proj_out." in name) or name.startswith("controlnet_down_blocks") or \
                name.startswith("controlnet_mid_block") or name.startswith("controlnet_cond_embedding")
            if zero and zero_init_heads:
                t = torch.zeros(shape)
        sd[name] = t
    return sd


def _tensors_in(args, kwargs):
    for a in list(args) + list(kwargs.values()):
        if torch.is_tensor(a):
            yield a
        elif isinstance(a, (list, tuple)):
            for b in a:
                if torch.is_tensor(b):
                    yield b
        elif isinstance(a, dict):
            for b in a.values():
                if torch.is_tensor(b):
                    yield b


def _on_device(fn):
    """Run a forward-like method with the handle's GPU current.  ``nr_net_create`` / ``hipMalloc`` / the plan arena and every
    kernel launch use the CURRENT HIP device, so a network moved with ``.to('cuda:1')`` must never run while device 0 is current;
    tensors living on another GPU are rejected instead of being handed to a kernel that cannot address them."""
    import functools

    @functools.wraps(fn)
    def inner(self, *args, **kwargs):
        cuda = [t for t in _tensors_in(args, kwargs) if t.is_cuda]
        if self.device.type != "cuda":
            if not cuda:
                return fn(self, *args, **kwargs)      # the method raises its own "CUDA tensors required" error
            self.device = cuda[0].device                 # never moved explicitly: adopt the first input's GPU (handle not created yet)
        for t in cuda:
            if t.device != self.device:
                raise RuntimeError(f"{type(self).__name__} lives on {self.device} but got a tensor on {t.device}")
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return inner


def tensor_version(t):
    """In-place version counter of ``t`` for identity-based caches, or a fresh unique object when the tensor has none (tensors created
    under torch.inference_mode raise on ``._version``): such tensors never hit a cache, they are re-staged / re-scanned on every call."""
    try:
        return t._version
    except RuntimeError:
        global _warned_versionless
        if not _warned_versionless:
            _warned_versionless = True
            import warnings
            warnings.warn("neurons_amd: a tensor created under torch.inference_mode() has no version counter, so the context / "
                          "condition caches cannot recognise it: every call re-stages it and recomputes the cross-attention K|V "
                          "(correct, but slower).  Use torch.no_grad() around the pipeline to keep the caches.", RuntimeWarning,
                          stacklevel=3)
        return object()


_warned_versionless = False


class _NativeNet:
    """Shared handle management for the two networks."""
    _kind = _lib.NR_KIND_UNET3D

    _config_cls = UNet3DConfig

    def __init__(self, config=None, **kwargs):
        if config is None:
            config = self._config_cls(**kwargs)
        elif kwargs:
            raise TypeError("pass either a UNet3DConfig or keyword arguments")
        self.config = config
        self.in_channels = config.in_channels
        self.sample_size = getattr(config, "sample_size", None)
        self.dtype = torch.float32          # dtype at the API boundary; compute is bf16/fp32-accumulate in HIP
        self.device = torch.device("cpu")
        self._cconf = self._build_cconf(config)
        self._schema = self._build_schema(config)
        self._h = None
        self._plan_key = None
        self._loaded = set()
        self._pending = {}
        self._graph = True

    def _build_cconf(self, config):
        return make_c_config(config, self._kind)

    def _build_schema(self, config):
        return state_dict_schema(config, self._kind)

    # -- module-like surface ---------------------------------------------------------------------------
    def to(self, device=None, dtype=None):
        if device is not None:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise RuntimeError("neurons_amd networks run on MI355X only (device must be 'cuda'); there is no CPU fallback")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
            if self._h is not None and dev != self.device:
                raise RuntimeError(f"{type(self).__name__} already holds weights on {self.device}; create a new instance for {dev}")
            self.device = dev
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    # Memory-saving switches of the reference classes that its callers flip before building the pipeline
    # (scripts/neuroclips_video.py:212-214 -> attention.py:228-254; unet.py:251-318; diffusers ModelMixin).  They select
    # among numerically equivalent PyTorch attention / autograd paths; the HIP engine has one attention path, no autograd
    # and a planned workspace, so they are accepted and change nothing.  Argument checks the reference makes are kept.
    def enable_xformers_memory_efficient_attention(self, *args, **kwargs):
        return None

    def disable_xformers_memory_efficient_attention(self):
        return None

    def set_use_memory_efficient_attention_xformers(self, valid=True, *args, **kwargs):
        return None

    def set_attention_slice(self, slice_size="auto"):
        """unet.py:251-314.  Accepted: "auto", "max", an int, or a list with one entry per attention layer."""
        if not (slice_size in ("auto", "max") or slice_size is None or isinstance(slice_size, (int, list, tuple))):
            raise ValueError(f"slice_size must be 'auto', 'max', an int or a list of ints, got {slice_size!r}")
        return None

    def enable_gradient_checkpointing(self):
        return None

    def disable_gradient_checkpointing(self):
        return None

    def _set_gradient_checkpointing(self, module=None, value=False):
        return None

    def train(self, mode=True):
        if mode:
            raise RuntimeError("neurons_amd networks are inference-only (no autograd through the HIP engine)")
        return self

    def enable_graph(self, flag=True):
        self._graph = bool(flag)
        if self._h is not None:
            _lib.check(_lib.load().nr_net_set_graph(self._h, 1 if flag else 0))
        return self

    def set_attention_fp8(self, flag=True):
        """BASELINE config 5: spatial self- and text cross-attention with OCP e4m3 MFMA operands (fp32 softmax and accumulation).
        bf16 stays the default; the next forward re-plans."""
        _lib.check(_lib.load().nr_net_set_attention_fp8(self._handle(), 1 if flag else 0))
        self._plan_key = None
        return self

    def set_weight_fp8(self, flag=True):
        """Weight-only OCP e4m3 storage (one power-of-two scale per row) for the Linears the small-M kernel serves (``nr_net_set_weight_fp8``;
        ``neurons_amd/w8.py`` has the format).  A numerics variant: bf16 stays the default (``NR_W8=1`` turns it on for new handles); the
        bf16 matrices stay resident, so it saves no memory.  The next forward re-plans."""
        _lib.check(_lib.load().nr_net_set_weight_fp8(self._handle(), 1 if flag else 0))
        self._plan_key = None
        return self

    def set_deterministic_batch(self, flag=True):
        """Batch-independent arithmetic (``nr_net_set_deterministic_batch``): plan choices are made per clip, so a clip's result does not
        depend on how many clips share the call.  Default off (``NR_DETERMINISTIC_BATCH=1`` turns it on for new handles)."""
        _lib.check(_lib.load().nr_net_set_deterministic_batch(self._handle(), 1 if flag else 0))
        self._plan_key = None
        return self

    def set_clip_samples(self, samples):
        """Samples of one clip in the batch: 2 = CFG pair (default), 1 = guidance off (``nr_net_set_clip_samples``; read in
        deterministic-batch mode only)."""
        if getattr(self, "_clip_samples", 2) != int(samples):
            _lib.check(_lib.load().nr_net_set_clip_samples(self._handle(), int(samples)))
            self._clip_samples = int(samples)
            self._plan_key = None
        return self

    def _set_cfg_pair_identical(self, flag):
        """``nr_net_set_cfg_pair_identical``: the next forwards' batches are [x; x] with one timestep (the denoising loop's CFG input), so the engine may
        evaluate the layers in front of the first cross-attention on half the batch.  Set by the pipeline-only entry points
        (``forward_with_controlnet`` / ``forward_after`` with ``cfg_pair_identical=True``), cleared by every plain ``forward``."""
        flag = bool(flag)
        if getattr(self, "_cfg_dup", False) != flag:
            _lib.check(_lib.load().nr_net_set_cfg_pair_identical(self._handle(), 1 if flag else 0))
            self._cfg_dup = flag
            self._plan_key = None

    def state_dict_keys(self):
        return list(self._schema.keys())

    def _handle(self):
        if self._h is None:
            if not torch.cuda.is_available():
                raise RuntimeError("neurons_amd: no HIP device visible; the networks run in libneurons_amd.so on MI355X only")
            if self.device.type != "cuda":
                self.device = torch.device("cuda", torch.cuda.current_device())
            lib = _lib.load()
            h = C.c_void_p()
            with torch.cuda.device(self.device):       # the handle is bound to the device that is current at creation
                _lib.check(lib.nr_net_create(C.byref(self._cconf), C.byref(h)))
            self._h = h
            _lib.check(lib.nr_net_set_graph(self._h, 1 if self._graph else 0))
        return self._h

    def load_state_dict(self, state_dict, strict=True):
        """Accepts the reference key names.  Returns (missing_keys, unexpected_keys) like torch."""
        missing = [k for k in self._schema if k not in state_dict and k not in self._loaded]
        unexpected = [k for k in state_dict if k not in self._schema and not k.endswith("pos_encoder.pe")]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}:\n\tMissing key(s): {missing[:8]}"
                               f"{'...' if len(missing) > 8 else ''}\n\tUnexpected key(s): {unexpected[:8]}")
        for k, v in state_dict.items():
            if k not in self._schema:
                continue
            if tuple(v.shape) != tuple(self._schema[k]):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)}, "
                                   f"the shape in current model is {tuple(self._schema[k])}.")
            self._pending[k] = v
            self._loaded.add(k)
        self._plan_key = None
        return missing, unexpected

    def _flush_weights(self):
        if not self._pending:
            return
        lib = _lib.load()
        h = self._handle()
        for k, v in self._pending.items():
            a = np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy())
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.nr_net_load_tensor(h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        self._pending = {}

    def _ensure_plan(self, batch, frames, h, w, ctx_len):
        self._flush_weights()
        key = (batch, frames, h, w, ctx_len)
        if key != self._plan_key:
            _lib.check(_lib.load().nr_net_plan(self._handle(), batch, frames, h, w, ctx_len))
            # The fp32 host copies (5 GB for the U-Net) are KEPT by default: which converted weights a plan builds depends on its GEMM
            # shapes (LayerNorm folding, row-panel / fused-kernel weight streams are chosen per M), so a later plan at another batch
            # (CFG off, another clip count, the synchronous controlnet(...) call next to the grouped schedule) may need one more.
            # A caller that drives ONE shape can drop them: auto_release_host_weights = True (or NR_RELEASE_HOST_WEIGHTS=1).
            if getattr(self, "auto_release_host_weights", os.environ.get("NR_RELEASE_HOST_WEIGHTS") == "1"):
                _lib.check(_lib.load().nr_net_release_host_weights(self._handle()))
            self._plan_key = key
            self._ctx_key = None         # _on_plan allocates fresh staging buffers: the cached context must be copied again
            self._on_plan()

    def _on_plan(self):
        pass

    def _set_context(self, ctx):
        """Copy the context into the fixed staging buffer only when it changed (tensor identity + in-place version
        counter); the engine then recomputes the cached K|V projections (nr_net_invalidate_context)."""
        key = (ctx.data_ptr(), tensor_version(ctx), tuple(ctx.shape), ctx.dtype)
        if getattr(self, "_ctx_key", None) != key or getattr(self, "_ctx_plan", None) != self._plan_key:
            self._io_ctx.copy_(ctx)
            _lib.check(_lib.load().nr_net_invalidate_context(self._handle()))
            self._ctx_key, self._ctx_plan = key, self._plan_key
            self._ctx_ref = ctx     # keep it alive: its address cannot be recycled for different contents while cached

    # -- converted-weight exchange (multi-GPU start-up: rank 0 converts once, the arena travels device to device) --------------
    @_on_device
    def export_weights(self):
        """(manifest bytes, packed uint8 CUDA tensor) of every converted device buffer.  Call after the first forward / plan."""
        lib = _lib.load()
        h = self._handle()
        nbytes = C.c_int64()
        n = lib.nr_net_export_manifest(h, None, 0, C.byref(nbytes))
        if n < 0:
            _lib.check(1)
        buf = C.create_string_buffer(int(n))
        lib.nr_net_export_manifest(h, buf, n, C.byref(nbytes))
        arena = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        _lib.check(lib.nr_net_export_weights(h, torch.cuda.current_stream().cuda_stream, arena.data_ptr(), arena.numel()))
        return bytes(buf.raw[:n]), arena

    @_on_device
    def import_weights(self, manifest: bytes, arena: torch.Tensor):
        """Adopt another handle's converted weights (same config, same plan shape): no state dict is ever loaded on this side."""
        if self._pending or self._loaded:
            raise RuntimeError("import_weights needs a fresh network (no load_state_dict before it)")
        if not arena.is_cuda or arena.dtype != torch.uint8:
            raise ValueError("arena must be the uint8 CUDA tensor export_weights() returned")
        _lib.check(_lib.load().nr_net_import_weights(self._handle(), torch.cuda.current_stream().cuda_stream, manifest, len(manifest),
                                                     arena.data_ptr(), arena.numel()))
        self._loaded = set(self._schema)
        self._plan_key = None

    @_on_device
    def op_descriptions(self):
        """One line per launch of the current plan ("igemm ks=... M=...", "tattn_head M=...", "cfg broadcast ..."; ``nr_net_op_desc``): tests assert
        WHICH kernel serves a layer."""
        lib = _lib.load()
        return [lib.nr_net_op_desc(self._h, i).decode() for i in range(lib.nr_net_num_ops(self._h))]

    def profile_last(self):
        """Per-kernel-class time / algorithmic work of the most recent forward (HIP events per launch)."""
        prof = _lib.NrProfile()
        _lib.check(_lib.load().nr_net_profile_last(self._handle(), torch.cuda.current_stream().cuda_stream, C.byref(prof)))
        return {name: dict(ms=prof.ms[i], flops=prof.flops[i], bytes=prof.bytes[i], launches=prof.launches[i])
                for i, name in enumerate(_lib.NR_PROF_NAMES)}

    def workspace_bytes(self):
        return int(_lib.load().nr_net_workspace_bytes(self._handle()))

    def weight_bytes(self):
        return int(_lib.load().nr_net_weight_bytes(self._handle()))

    @staticmethod
    def _timesteps_host(timestep, batch):
        if torch.is_tensor(timestep):
            t = timestep.detach().to("cpu", torch.float32).reshape(-1)   # sync only if the caller passed a device tensor
            vals = [float(x) for x in t]
        else:
            vals = [float(timestep)]
        if len(vals) == 1:
            vals = vals * batch
        if len(vals) != batch:
            raise ValueError(f"timestep has {len(vals)} entries for batch {batch}")
        return (C.c_float * batch)(*vals)

    def __del__(self):
        try:
            if self._h is not None:
                _lib.load().nr_net_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _as_nhwc_bf16(r, frames):
    """ControlNet residual (b, C, f, h, w) -> channels-last bf16 buffer; zero-copy for NativeSparseCtrl outputs."""
    if r.dim() == 4:            # (b, C, h, w) broadcast over frames  (unet.py:426-427)
        r = r.unsqueeze(2).expand(-1, -1, frames, -1, -1)
    v = r.permute(0, 2, 3, 4, 1)
    if v.dtype == torch.bfloat16 and v.is_contiguous():
        return v
    return v.to(torch.bfloat16).contiguous()


class NativeUNet3D(_NativeNet):
    _kind = _lib.NR_KIND_UNET3D

    @classmethod
    def from_pretrained_2d(cls, pretrained_model_name_or_path, unet_additional_kwargs=None, subfolder=None, **kwargs):
        """``UNet3DConditionModel.from_pretrained_2d`` (unet.py:477-572) for a LOCAL diffusers directory (there is no hub
        access): read ``<path>[/<subfolder>]/config.json`` of the 2-D SD U-Net, force the 3-D block types exactly as the
        reference does (:551-562), apply ``unet_additional_kwargs`` (inference-v3.yaml), then load
        ``diffusion_pytorch_model.safetensors`` (or ``.bin``) with ``strict=False`` — the motion-module keys stay missing
        until ``load_weights`` brings the motion checkpoint (util.py:106-121)."""
        import json
        import os
        root = os.path.join(pretrained_model_name_or_path, subfolder) if subfolder else pretrained_model_name_or_path
        with open(os.path.join(root, "config.json")) as f:
            config = json.load(f)
        config["down_block_types"] = ["CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"]
        config["up_block_types"] = ["UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"]
        config.update(unet_additional_kwargs or {})
        known = {f for f in UNet3DConfig.__dataclass_fields__}
        # 2-D switches the NEURONS configs leave at their defaults (rejected if set otherwise) and bookkeeping keys
        inert = {"_class_name": None, "_diffusers_version": None, "_name_or_path": None, "center_input_sample": False, "flip_sin_to_cos": True,
                 "freq_shift": 0, "downsample_padding": 1, "mid_block_scale_factor": 1, "act_fn": "silu", "dual_cross_attention": False,
                 "use_linear_projection": False, "class_embed_type": None, "num_class_embeds": None, "upcast_attention": False,
                 "resnet_time_scale_shift": "default", "only_cross_attention": False, "mid_block_type": "UNetMidBlock3DCrossAttn",
                 "unet_use_cross_frame_attention": False, "unet_use_temporal_attention": False}
        fields = {}
        for k, v in config.items():
            if k in known:
                fields[k] = tuple(v) if isinstance(v, list) else v
            elif k in inert:
                if inert[k] is not None and v is not None and v != inert[k]:
                    raise NotImplementedError(f"config.json: {k}={v!r} is not built (the NEURONS inference path uses {inert[k]!r})")
            else:
                raise NotImplementedError(f"config.json: unknown U-Net option {k!r}")
        model = cls(UNet3DConfig(**fields))
        print(f"loaded 3D unet's pretrained weights from {pretrained_model_name_or_path} ...")
        st = os.path.join(root, "diffusion_pytorch_model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            state_dict = load_file(st)
        else:
            state_dict = torch.load(os.path.join(root, "diffusion_pytorch_model.bin"), map_location="cpu")
        m, u = model.load_state_dict(state_dict, strict=False)
        print(f"### missing keys: {len(m)}; \n### unexpected keys: {len(u)};")
        params = [int(np.prod(shape)) if "motion_modules." in n else 0 for n, shape in model._schema.items()]
        print(f"### Motion Module Parameters: {sum(params) / 1e6} M")
        return model

    @_on_device
    def forward(self, sample, timestep, encoder_hidden_states, class_labels=None, attention_mask=None,
                down_block_additional_residuals: Optional[Sequence[torch.Tensor]] = None,
                mid_block_additional_residual: Optional[torch.Tensor] = None, return_dict: bool = True):
        if class_labels is not None or attention_mask is not None:
            raise NotImplementedError("class_labels / attention_mask are not used on the NEURONS path")
        if sample.dim() != 5:
            raise ValueError(f"Expected sample to have ndim=5 (b c f h w), got {sample.dim()}")
        if not sample.is_cuda:
            raise RuntimeError("NativeUNet3D.forward: CUDA (ROCm) tensors required; there is no CPU fallback")
        b, c, f, h, w = sample.shape
        if c != self.config.in_channels:
            raise ValueError(f"sample has {c} channels, expected {self.config.in_channels}")
        ctx = encoder_hidden_states
        if ctx.shape[0] != b or ctx.shape[2] != self.config.cross_attention_dim:
            raise ValueError(f"encoder_hidden_states shape {tuple(ctx.shape)} does not match batch {b} / cross_attention_dim")
        self._set_cfg_pair_identical(False)        # arbitrary batches: nothing is assumed about the two halves
        self._ensure_plan(b, f, h, w, ctx.shape[1])
        lib = _lib.load()
        # fixed I/O staging buffers: stable pointers let the engine replay one captured hipGraph
        self._io_sample.copy_(sample)
        self._set_context(ctx)
        sample_c, ctx_c, out = self._io_sample, self._io_ctx, self._io_out
        ts = self._timesteps_host(timestep, b)
        keep = []
        down_ptrs = None
        mid_ptr = None
        if (down_block_additional_residuals is None) != (mid_block_additional_residual is None):
            raise ValueError("down_block_additional_residuals and mid_block_additional_residual must be given together")
        if down_block_additional_residuals is not None:
            n = int(lib.nr_net_num_residuals(self._h))
            if len(down_block_additional_residuals) != n:
                raise ValueError(f"expected {n} down-block residuals, got {len(down_block_additional_residuals)}")
            keep = [_as_nhwc_bf16(r, f) for r in down_block_additional_residuals]
            mid = _as_nhwc_bf16(mid_block_additional_residual, f)
            keep.append(mid)
            down_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in keep[:n]])
            mid_ptr = mid.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.nr_unet3d_forward(self._h, stream, sample_c.data_ptr(), ts, ctx_c.data_ptr(), ctx.shape[1],
                                         down_ptrs, mid_ptr, out.data_ptr()))
        out = out.clone()
        if not return_dict:
            return (out,)
        return UNet3DConditionOutput(sample=out)

    __call__ = forward

    @_on_device
    def forward_with_controlnet(self, controlnet, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_mask,
                                conditioning_scale: float = 1.0, next_timestep=None, cfg_pair_identical: bool = False):
        """``controlnet(...)`` then ``self(..., down_block_additional_residuals=..., mid_block_additional_residual=...)``
        (pipeline_neuroclips.py:460-475) as ONE library call that overlaps SparseCtrl with the U-Net encoder
        (C ABI ``nr_denoise_step_forward``).  Returns the same ``.sample`` tensor as the two separate calls.
        ``next_timestep``: timestep of the following step of the same clip — SparseCtrl's evaluation for it (which does
        not depend on the latents) is then issued early and overlaps this step's decoder.  Same results."""
        if not sample.is_cuda:
            raise RuntimeError("forward_with_controlnet: CUDA (ROCm) tensors required; there is no CPU fallback")
        b, c, f, h, w = sample.shape
        ctx = encoder_hidden_states
        if ctx.shape[0] != b:
            raise ValueError("encoder_hidden_states batch must equal the sample batch")
        cb = controlnet_cond.shape[0]
        if b % cb != 0 or conditioning_mask.shape[0] != cb:
            raise ValueError("controlnet_cond batch must divide the sample batch")
        controlnet._check_condition(controlnet_cond, conditioning_mask, f, h, w)
        L = ctx.shape[1]
        if controlnet.device.type == "cuda" and controlnet.device != self.device:
            raise RuntimeError(f"U-Net on {self.device} but SparseCtrl on {controlnet.device}")
        controlnet.to(self.device)
        self._set_cfg_pair_identical(cfg_pair_identical and b % 2 == 0 and not torch.is_tensor(timestep))
        self._ensure_plan(b, f, h, w, L)
        controlnet._sync_condition_frames(controlnet_cond, conditioning_mask)
        controlnet._ensure_plan(b, f, h, w, L)
        self._io_sample.copy_(sample)
        self._set_context(ctx)
        controlnet._set_context(ctx)
        controlnet._stage_buffers(cb, f, h, w, sample.device)
        # copy the (step-invariant) condition only when it changed: a prefetched SparseCtrl evaluation may be reading it
        ckey = (controlnet_cond.data_ptr(), tensor_version(controlnet_cond), conditioning_mask.data_ptr(), tensor_version(conditioning_mask),
                tuple(controlnet_cond.shape), controlnet._plan_key)
        if getattr(controlnet, "_cond_key", None) != ckey:
            _lib.check(_lib.load().nr_net_invalidate_context(controlnet._handle()))     # drops any prefetched evaluation
            controlnet._io_cond.copy_(controlnet_cond)
            controlnet._io_mask.copy_(conditioning_mask)
            controlnet._cond_key = ckey
            controlnet._cond_ref = (controlnet_cond, conditioning_mask)
        ts = self._timesteps_host(timestep, b)
        ts_next = self._timesteps_host(next_timestep, b) if next_timestep is not None else None
        n = len(controlnet._out_bufs) - 1
        lib = _lib.load()
        _lib.check(lib.nr_denoise_step_forward(self._h, controlnet._h, torch.cuda.current_stream().cuda_stream,
                                               self._io_sample.data_ptr(), ts, self._io_ctx.data_ptr(), L,
                                               controlnet._io_cond.data_ptr(), controlnet._io_mask.data_ptr(), cb,
                                               float(conditioning_scale), controlnet._out_ptrs,
                                               controlnet._out_bufs[n].data_ptr(), self._io_out.data_ptr(), ts_next))
        return UNet3DConditionOutput(sample=self._io_out.clone())

    @_on_device
    def forward_after(self, controlnet, slot, residual_bufs, sample_index, sample, timestep, encoder_hidden_states, cfg_pair_identical: bool = False):
        """U-Net evaluation that consumes samples ``[sample_index, sample_index + b)`` of the SparseCtrl evaluation pending in ``slot``
        (``NativeSparseCtrl.forward_async``): C ABI ``nr_unet3d_forward_after``.  The encoder overlaps the pending evaluation; the
        residual adds wait for it."""
        if not sample.is_cuda:
            raise RuntimeError("forward_after: CUDA (ROCm) tensors required; there is no CPU fallback")
        b, c, f, h, w = sample.shape
        ctx = encoder_hidden_states
        if ctx.shape[0] != b:
            raise ValueError("encoder_hidden_states batch must equal the sample batch")
        L = ctx.shape[1]
        # cfg_pair_identical: the caller built `sample` as cat([x] * 2) and passes ONE scalar timestep (the denoising loop): CFG de-duplication
        self._set_cfg_pair_identical(cfg_pair_identical and b % 2 == 0 and not torch.is_tensor(timestep))
        self._ensure_plan(b, f, h, w, L)
        self._io_sample.copy_(sample)
        self._set_context(ctx)
        n = len(residual_bufs) - 1
        views = [t[sample_index:sample_index + b] for t in residual_bufs]
        if views[0].shape[0] != b:
            raise ValueError("the pending SparseCtrl evaluation does not contain the requested samples")
        ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in views[:n]])
        ts = self._timesteps_host(timestep, b)
        _lib.check(_lib.load().nr_unet3d_forward_after(self._h, controlnet._h, int(slot), torch.cuda.current_stream().cuda_stream,
                                                       self._io_sample.data_ptr(), ts, self._io_ctx.data_ptr(), L, ptrs,
                                                       views[n].data_ptr(), self._io_out.data_ptr()))
        return UNet3DConditionOutput(sample=self._io_out.clone())

    def _on_plan(self):
        b, f, h, w, L = self._plan_key
        dev = self.device
        self._io_sample = torch.empty(b, self.config.in_channels, f, h, w, dtype=torch.float32, device=dev)
        self._io_ctx = torch.empty(b, L, self.config.cross_attention_dim, dtype=torch.float32, device=dev)
        self._io_out = torch.empty(b, self.config.out_channels, f, h, w, dtype=torch.float32, device=dev)
