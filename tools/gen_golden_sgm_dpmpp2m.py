"""Golden vectors of the sgm DPM-Solver++ 2M sampler from the REFERENCE's own classes -> tests/golden/sgm_dpmpp2m_tiny.npz.

What runs is the reference's ``DPMPP2MSampler`` (generative_models/sgm/modules/diffusionmodules/sampling.py:292-367) + ``VanillaCFG(5.0)`` over its
``LegacyDDPMDiscretization``, ``DiscreteDenoiser`` / ``EpsScaling`` and ``OpenAIWrapper(UNetModel)`` at ``tiny_sgm_config`` (synthetic weights from
the Philox recipe, U-Net seed 71), in fp32 on the CPU; its ``do_img2img`` (sgm/inference/helpers.py:243-305) with ``skip_encode`` over the same
sampler on a pruned table; and both of its samplers (Euler, 2M) on a Gaussian toy model whose exact solution is known.  Nothing of the reference is
restated here: the classes are imported where they lie and called.  Stand-ins are those of tools/gen_golden_sgm_img2img.py (its ``load_helpers``,
``RecordingSampler``); the img2img model's ``decode_first_stage`` is the identity, since only the latents are kept.

The file holds
  sig_<n>, vars_<n>, mult_<n>     n in {1, 2, 10, 19, 38}: the sigma table (n + 1 entries), and per step get_variables' (h, r, t, t_next) and
                                  get_mult's (mult1 .. mult4) as fp32 rows; r / mult3 / mult4 are NaN on the first step (no previous sigma)
  ctx, uc_ctx, vec, x_in          conditioning and the start of the loops (2 samples of (4, 8, 8))
  loop<n>.xs / .dens / .final / .calls     n in {4, 10}: x and denoised after EVERY step, the final x, network evaluations
  z_init, noise, offset, i2i<s>.start / .z / .calls     s in {0.5, 1.0}: do_img2img(skip_encode=True), 10 steps, offset_noise_level 0.04
  gauss.x, gauss.exact, gauss.<euler|dpmpp2m>_<n>, gauss.err_<euler|dpmpp2m>_<n>     n in {10, 19, 20, 38}: data ~ N(0, 1), the exact denoiser
                                  x / (1 + sigma^2), finals, the exact end point and the relative end errors (fp64 norms)

Runs only where the reference sources are; the tests read the stored arrays only.

Usage:  python tools/gen_golden_sgm_dpmpp2m.py [output path]
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TABLES = (1, 2, 10, 19, 38)
LOOPS = (4, 10)
I2I_STRENGTHS = (0.5, 1.0)
I2I_STEPS = 10
GAUSS_STEPS = (10, 19, 20, 38)
N = 2
OFFSET_LEVEL = 0.04
DCFG = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
GCFG = {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}}


@torch.no_grad()
def main(path):
    from gen_golden_sgm_img2img import RecordingSampler, load_helpers, quiet
    from oracle import gen_golden as G
    from neurons_amd.sgm import sgm_random_state_dict
    from neurons_amd.synth import randn
    from tiny_configs import tiny_sgm_config
    helpers = load_helpers()
    from sgm.modules.diffusionmodules.denoiser import DiscreteDenoiser
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    from sgm.modules.diffusionmodules.sampling import DPMPP2MSampler, EulerEDMSampler
    from sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
    out = {}

    def sampler_2m(steps):
        return DPMPP2MSampler(num_steps=steps, discretization_config=DCFG, guider_config=GCFG, device="cpu")

    # ---- coefficient rows ----------------------------------------------------------------------------------------------------------
    nan = torch.tensor([float("nan")])
    for n in TABLES:
        s = sampler_2m(n)
        sig = LegacyDDPMDiscretization()(n)
        rows_v, rows_m = [], []
        for i in range(n):
            prev = None if i == 0 else sig[i - 1:i]
            h, r, t, t_next = s.get_variables(sig[i:i + 1], sig[i + 1:i + 2], prev)
            mult = s.get_mult(h, r, t, t_next, prev)
            rows_v.append(torch.cat([h, nan if r is None else r, t, t_next]))
            rows_m.append(torch.cat(list(mult) + [nan] * (4 - len(mult))))
        out[f"sig_{n}"] = sig.numpy()
        out[f"vars_{n}"] = torch.stack(rows_v).numpy()
        out[f"mult_{n}"] = torch.stack(rows_m).numpy()
        assert out[f"sig_{n}"].dtype == np.float32 and out[f"mult_{n}"].dtype == np.float32

    # ---- loops on the tiny network -------------------------------------------------------------------------------------------------
    cfg = tiny_sgm_config()
    net = G.build_reference_sgm(cfg, sgm_random_state_dict(cfg, seed=71))
    ctx = randn("d2m.ctx", (N, 24, cfg.context_dim), 181)
    uc_ctx = randn("d2m.uc_ctx", (N, 24, cfg.context_dim), 182)
    vec = randn("d2m.vec", (N, cfg.adm_in_channels), 183)
    x_in = randn("d2m.x_in", (N, 4, 8, 8), 184)
    c = {"crossattn": ctx, "vector": vec}
    uc = {"crossattn": uc_ctx, "vector": vec}
    calls = [0]

    class CountingWrapper(OpenAIWrapper):
        def forward(self, *a, **k):
            calls[0] += 1
            return super().forward(*a, **k)

    model = CountingWrapper(net)
    denoiser = DiscreteDenoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                                discretization_config=DCFG)
    out.update(ctx=ctx.numpy(), uc_ctx=uc_ctx.numpy(), vec=vec.numpy(), x_in=x_in.numpy())

    def denoise(xx, sigma, cc):
        return denoiser(model, xx, sigma, cc)

    for n in LOOPS:
        s = sampler_2m(n)
        xs, dens = [], []
        step = s.sampler_step

        def recording_step(*a, **k):
            x, den = step(*a, **k)
            xs.append(x.clone())
            dens.append(den.clone())
            return x, den

        s.sampler_step = recording_step
        calls[0] = 0
        final = s(denoise, x_in.clone(), cond=c, uc=uc)
        assert calls[0] == n and len(xs) == n and torch.equal(final, xs[-1]) and torch.equal(xs[-1], dens[-1])
        out[f"loop{n}.xs"] = torch.stack(xs).numpy()
        out[f"loop{n}.dens"] = torch.stack(dens).numpy()
        out[f"loop{n}.final"] = final.numpy()
        out[f"loop{n}.calls"] = np.array(calls[0])
        print(f"sgm_dpmpp2m: loop {n}: {calls[0]} network calls, final std {final.std().item():.3f}", flush=True)

    # ---- img2img (skip_encode) -----------------------------------------------------------------------------------------------------
    z_init = randn("d2m.z_init", (N, 4, 8, 8), 185) * 0.7
    i2i_model = types.SimpleNamespace(
        ema_scope=__import__("contextlib").nullcontext,
        conditioner=types.SimpleNamespace(embedders=[], get_unconditional_conditioning=lambda batch, batch_uc=None, force_uc_zero_embeddings=None:
                                          (dict(c), dict(uc))),
        denoiser=denoiser, model=model, decode_first_stage=lambda z: z)
    seed = 654
    torch.manual_seed(seed)                       # the draws in the order do_img2img makes them: noise = randn_like(z), offset = randn(n)
    noise = torch.randn(N, 4, 8, 8)
    offset = torch.randn(N)
    out.update(z_init=z_init.numpy(), noise=noise.numpy(), offset=offset.numpy(), i2i_steps=np.array(I2I_STEPS),
               offset_noise_level=np.array(OFFSET_LEVEL))
    for strength in I2I_STRENGTHS:
        s = sampler_2m(I2I_STEPS)
        s.discretization = helpers.Img2ImgDiscretizationWrapper(s.discretization, strength)
        rec = RecordingSampler(s)
        calls[0] = 0
        torch.manual_seed(seed)
        _, z = quiet(helpers.do_img2img, z_init, i2i_model, rec, {}, N, offset_noise_level=OFFSET_LEVEL, return_latents=True, skip_encode=True,
                     device="cpu")
        pruned = quiet(s.discretization, I2I_STEPS)
        assert calls[0] == len(pruned) - 1, (strength, calls[0], len(pruned))
        out[f"i2i{strength}.sig"] = pruned.numpy()
        out[f"i2i{strength}.start"] = rec.start.numpy()
        out[f"i2i{strength}.z"] = z.numpy()
        out[f"i2i{strength}.calls"] = np.array(calls[0])
        print(f"sgm_dpmpp2m: img2img {strength}: {calls[0]} network calls, z std {z.std().item():.3f}", flush=True)

    # ---- Gaussian model: data ~ N(0, 1), exact denoiser x / (1 + sigma^2) ------------------------------------------------------------
    from sgm.util import append_dims
    gx = torch.randn(torch.Size((N, 4, 8, 8)), generator=torch.Generator().manual_seed(186))
    gc = {"crossattn": torch.zeros(N, 1, 4), "vector": torch.zeros(N, 4)}
    out["gauss.x"] = gx.numpy()

    def gauss(xx, sigma, cc):
        return xx / (1.0 + append_dims(sigma, xx.ndim) ** 2)

    # the probability-flow solution keeps x / sqrt(1 + sigma^2) constant: the sampler starts from gx sqrt(1 + sigma0^2) at sigma0 (sampling.py:52),
    # so the exact end point at sigma = 0 is gx itself, whatever the table
    exact = gx.double()
    for n in GAUSS_STEPS:
        for name, s in (("euler", EulerEDMSampler(num_steps=n, discretization_config=DCFG, guider_config=GCFG, device="cpu")),
                        ("dpmpp2m", sampler_2m(n))):
            final = s(gauss, gx.clone(), cond=gc, uc=gc)
            err = ((final.double() - exact).norm() / exact.norm()).item()
            out[f"gauss.{name}_{n}"] = final.numpy()
            out[f"gauss.err_{name}_{n}"] = np.array(err)
            print(f"sgm_dpmpp2m: gaussian model, {name} {n} steps: relative end error {err:.4f}", flush=True)
    out["gauss.exact"] = exact.numpy()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sgm_dpmpp2m_tiny.npz"))
