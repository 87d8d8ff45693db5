"""GPU: the full DDIM update (eta, clip_sample, use_clipped_model_output, prediction types) at the op, the scheduler and the pipeline level.

The reference of every numeric check is ``ddim_ref`` below: the published rule (Song et al. 2021 eq. 12 / 16 in the form diffusers 0.11.1
ships, with the noise re-derived from x0 for ``sample`` / ``v_prediction``) restated in fp64.  It uses nothing of neurons_amd."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_engine_gpu import metrics  # noqa: E402

PREDS = ("epsilon", "sample", "v_prediction")
CLIPS = ((False, False), (True, False), (True, True))       # (clip_sample, use_clipped_model_output)
ETAS = (0.0, 0.5, 1.0)
A_T, A_PREV = 0.6, 0.8


def ddim_ref(model_output, x, a_t, a_prev, eta=0.0, prediction_type="epsilon", clip=False, clipped_output=False, noise=None, guidance=None):
    """fp64.  ``model_output``: [2B, ...] (uncond half first) when ``guidance`` is given, else [B, ...].  Returns (x_prev, x0, x0 before the clamp)."""
    m, x = model_output.double().cpu(), x.double().cpu()
    if guidance is not None:
        mu, mc = m.chunk(2)
        m = mu + guidance * (mc - mu)
    sa, sb = math.sqrt(a_t), math.sqrt(1.0 - a_t)
    if prediction_type == "epsilon":
        x0, e = (x - sb * m) / sa, m
    elif prediction_type == "sample":
        x0 = m
        e = (x - sa * x0) / sb
    else:
        x0 = sa * x - sb * m
        e = sa * m + sb * x
    raw = x0
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    if clipped_output:
        e = (x - sa * x0) / sb
    sigma = eta * math.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))
    out = math.sqrt(a_prev) * x0 + math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0)) * e
    if sigma > 0.0:
        out = out + sigma * noise.double().cpu()
    return out, x0, raw


def _close(name, got, ref):
    """fp32 arithmetic of a dozen operations on values of the size of ref: max abs error <= 1e-5 (1 + max|ref|)."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), name
    err, bound = (got - ref).abs().max().item(), 1e-5 * (1.0 + ref.abs().max().item())
    print(f"[{name}] max_err={err:.3e} bound={bound:.3e}")
    assert err <= bound, (name, err, bound)


_INPUTS = {}


def _inputs(n, cfg):
    """N(0, 1) * 1.5 on a fixed seed, made once per (n, cfg) and left unchanged.  Under guidance 7.5 the combined output has a standard
    deviation of 1.5 sqrt(6.5^2 + 7.5^2) = 14.9, so for ``sample`` prediction (x0 = e) the expected clamped share is 0.947, with a spread of
    0.007 at these sizes: the seeds are ones whose draws lie inside the 5 % .. 95 % window the op test asserts."""
    if (n, cfg) not in _INPUTS:
        g = torch.Generator().manual_seed(n + (1 if cfg else 0))
        shape = (4, 4, 8, 8) if n == 4 * 4 * 8 * 8 else (n,)
        eps = torch.randn((2 if cfg else 1,) + shape, generator=g) * 1.5
        x = torch.randn((1,) + shape, generator=g) * 1.5
        z = torch.randn((1,) + shape, generator=g) * 1.5
        _INPUTS[(n, cfg)] = tuple(t.cuda() for t in (eps, x, z))
    return _INPUTS[(n, cfg)]


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("clip,clipped", CLIPS)
@pytest.mark.parametrize("pred", PREDS)
def test_op_matches_fp64_restatement(cuda, pred, clip, clipped, eta):
    """n = 1024 takes the 16-byte path; n = 1031 (odd, no multiple of 4: a ragged last block) takes the 16-byte path with its scalar tail
    without guidance and the one-element-per-thread kernel with it (the text half of eps then starts off a 16-byte boundary)."""
    from neurons_amd import ops
    for n in (4 * 4 * 8 * 8, 1031):
        for cfg in (True, False):
            eps, x, z = _inputs(n, cfg)
            ref, ref0, raw = ddim_ref(eps, x, A_T, A_PREV, eta, pred, clip, clipped, z, 7.5 if cfg else None)
            if clip:
                frac = (raw.abs() > 1.0).double().mean().item()
                print(f"[{pred} n={n} cfg={cfg}] clamped share of x0: {frac:.3f}")
                assert 0.05 <= frac <= 0.95, frac
            out, x0 = ops.cfg_ddim_step(eps, x, 7.5, A_T, A_PREV, do_cfg=cfg, prediction_type=pred, clip_sample=clip,
                                        use_clipped_model_output=clipped, eta=eta, noise=z if eta > 0 else None, return_pred_original=True)
            assert out.shape == x.shape and x0.shape == x.shape
            _close(f"{pred} clip={clip}/{clipped} eta={eta} n={n} cfg={cfg}: x_prev", out, ref)
            _close(f"{pred} clip={clip}/{clipped} eta={eta} n={n} cfg={cfg}: x0", x0, ref0)
            # without the x0 output the same values come back
            only = ops.cfg_ddim_step(eps, x, 7.5, A_T, A_PREV, do_cfg=cfg, prediction_type=pred, clip_sample=clip,
                                     use_clipped_model_output=clipped, eta=eta, noise=z if eta > 0 else None)
            assert torch.equal(only, out)


@pytest.mark.parametrize("n", [4 * 4 * 8 * 8, 1031])
@pytest.mark.parametrize("cfg", [True, False])
def test_op_default_rule_through_keywords_is_the_positional_call(cuda, n, cfg):
    from neurons_amd import ops
    eps, x, z = _inputs(n, cfg)
    old = ops.cfg_ddim_step(eps, x, 7.5, A_T, A_PREV, cfg)
    new = ops.cfg_ddim_step(eps, x, 7.5, A_T, A_PREV, cfg, prediction_type="epsilon", clip_sample=False, use_clipped_model_output=False,
                            eta=0.0, noise=z)       # a keyword that is set routes the call through nr_cfg_ddim_step_ex
    assert torch.equal(old, new)
    _close("default rule vs restatement", new, ddim_ref(eps, x, A_T, A_PREV, guidance=7.5 if cfg else None)[0])


@pytest.mark.parametrize("pred", PREDS)
def test_op_last_step_is_finite_and_returns_x0(cuda, pred):
    """a_prev = 1 (set_alpha_to_one at the last step): sigma = 0 and the direction coefficient is 0 whatever eta is."""
    from neurons_amd import ops
    for n in (4 * 4 * 8 * 8, 1031):
        eps, x, z = _inputs(n, False)
        for eta in (0.0, 1.0):
            out, x0 = ops.cfg_ddim_step(eps, x, 1.0, A_T, 1.0, do_cfg=False, prediction_type=pred, clip_sample=True, eta=eta, noise=z,
                                        return_pred_original=True)
            assert torch.isfinite(out).all() and torch.equal(out, x0)
            _close(f"{pred} last step", out, ddim_ref(eps, x, A_T, 1.0, eta, pred, True, False, z)[1])


def test_op_argument_errors(cuda):
    from neurons_amd import _lib, ops
    eps, x, z = _inputs(1031, False)
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_ddim_step(eps, x, 1.0, A_T, A_PREV, do_cfg=False, eta=0.5)            # sigma > 0 without noise: NR_ERR_ARG
    with pytest.raises(ValueError, match="prediction_type"):
        ops.cfg_ddim_step(eps, x, 1.0, A_T, A_PREV, do_cfg=False, prediction_type="foo")
    lib = _lib.load()
    out = torch.empty_like(x)
    st = lib.nr_cfg_ddim_step_ex(torch.cuda.current_stream().cuda_stream, eps.data_ptr(), x.data_ptr(), out.data_ptr(), None, x.numel(), 1.0, 0,
                                 7, 0, 0, A_T, A_PREV, 0.0, math.sqrt(1 - A_PREV), None)
    assert st == 1 and b"prediction type" in lib.nr_last_error()                      # NR_ERR_ARG


# ---- scheduler level --------------------------------------------------------------------------------------------------------------------
def _walk(cuda, use_generator):
    from neurons_amd import DDIMScheduler
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=True)
    sched.set_timesteps(10)
    shape, eta = (1, 4, 4, 8, 8), 0.7
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(shape, generator=g) * 1.5).cuda()
    outs = [(torch.randn(shape, generator=g) * 1.5).cuda() for _ in range(10)]
    gen = torch.Generator(device="cuda").manual_seed(4242)
    twin = torch.Generator(device="cuda").manual_seed(4242)
    # the table as diffusers builds it: fp32 linspace, fp32 cumprod
    ac = torch.cumprod(1.0 - torch.linspace(0.00085, 0.012, 1000, dtype=torch.float32), 0)
    chain = x.double().cpu()                    # the restatement's own chain, never fed from the GPU result
    for i, t in enumerate(sched.timesteps_host):
        z = torch.randn(shape, generator=twin, device="cuda", dtype=torch.float32)     # what step() must draw: one tensor per step
        a_t, a_prev = float(ac[t]), (float(ac[t - 100]) if t - 100 >= 0 else 1.0)
        ref, ref0, _ = ddim_ref(outs[i], x, a_t, a_prev, eta, "epsilon", True, False, z)
        chain = ddim_ref(outs[i], chain, a_t, a_prev, eta, "epsilon", True, False, z)[0]
        if use_generator:
            res = sched.step(outs[i], t, x, eta=eta, generator=gen)
        else:
            res = sched.step(outs[i], t, x, eta=eta, variance_noise=z)
        _close(f"walk step {i} (t = {t}): prev_sample", res.prev_sample, ref)
        _close(f"walk step {i} (t = {t}): pred_original_sample", res.pred_original_sample, ref0)
        x = res.prev_sample
    assert torch.isfinite(x).all()
    # end of the walk against the fp64 chain: a step passes an input error on with d x_prev / d x <= sqrt(a_prev / a_t) (unclamped x0), whose
    # product over the walk is sqrt(1 / alphas_cumprod[901]) < 15, and each of the 10 steps adds its own 1e-5 (1 + max|ref|)
    err, bound = (x.double().cpu() - chain).abs().max().item(), 10 * 15 * 1e-5 * (1.0 + chain.abs().max().item())
    print(f"[walk end vs fp64 chain] max_err={err:.3e} bound={bound:.3e}")
    assert err <= bound


def test_scheduler_walk_with_variance_noise(cuda):
    _walk(cuda, use_generator=False)


def test_scheduler_walk_with_generator_pins_the_noise_order(cuda):
    _walk(cuda, use_generator=True)


# ---- pipeline level ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(cuda):
    from neurons_amd import DDIMScheduler, NeuroclipsPipeline
    from neurons_amd.synth import randn
    from test_shapes_gpu import _nets
    unet, ctrl, ucfg, ccfg, usd, csd = _nets()
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = NeuroclipsPipeline(None, None, None, unet, sched, ctrl).to("cuda")
    lat = randn("e.lat", (1, 4, 4, 8, 8), 1).cuda()
    noise = randn("e.noise", (1, 4, 4, 8, 8), 2)
    ctx = randn("e.ctx", (2, 77, 64), 3).cuda()
    cimg = (randn("e.cimg", (1, 4, 1, 8, 8), 4) * 0.18215).cuda()

    def run(**kw):
        return pipe("", video_length=4, height=64, width=64, num_inference_steps=4, low_strength=0.3, output_type="latent", latents=lat,
                    noise=noise, text_embeddings=ctx, controlnet_images=cimg, controlnet_image_index=[0], guidance_scale=7.5, **kw).videos
    return dict(pipe=pipe, sched=sched, run=run, lat=lat, noise=noise, ctx=ctx, cimg=cimg, ucfg=ucfg, ccfg=ccfg, usd=usd, csd=csd)


def test_pipeline_eta_one_vs_oracle_loop(tiny, monkeypatch):
    from oracle import animatediff_oracle as O
    calls = []
    real_step = tiny["sched"].step
    monkeypatch.setattr(tiny["sched"], "step", lambda *a, **k: (calls.append(1), real_step(*a, **k))[1])
    out = tiny["run"](eta=1.0, generator=torch.Generator(device="cuda").manual_seed(314))
    assert calls == []                          # the own-scheduler fused path: CFG + update in one kernel per step, no scheduler.step
    assert tiny["pipe"].last_controlnet_group >= 1

    twin = torch.Generator(device="cuda").manual_seed(314)
    shape = tuple(tiny["lat"].shape)
    torch.randn(shape, generator=twin, device="cuda", dtype=torch.float32)           # the unused keylatents draw comes first
    zs = [torch.randn(shape, generator=twin, device="cuda", dtype=torch.float32) for _ in range(4)]
    gu, gc = {k: v.cuda() for k, v in tiny["usd"].items()}, {k: v.cuda() for k, v in tiny["csd"].items()}
    ou, oc = O.OracleConfig.from_native(tiny["ucfg"]), O.OracleConfig.from_native(tiny["ccfg"])
    betas = torch.linspace(0.00085, 0.012, 1000, dtype=torch.float64)
    ac = torch.cumprod(1.0 - betas, 0)
    ts = [751, 501, 251, 1]
    lat, cimg, ctx = tiny["lat"], tiny["cimg"], tiny["ctx"]
    x = math.sqrt(float(ac[ts[0]])) * lat.double().cpu() + math.sqrt(1.0 - float(ac[ts[0]])) * tiny["noise"].double()
    cond = torch.zeros(1, 4, 4, 8, 8, device="cuda")
    mask = torch.zeros(1, 1, 4, 8, 8, device="cuda")
    cond[:, :, [0]] = cimg[:, :, :1]
    mask[:, :, [0]] = 1
    with torch.no_grad():
        for i, t in enumerate(ts):
            xin = torch.cat([x.float().cuda()] * 2)
            down, mid = O.sparse_controlnet_forward(gc, oc, xin, t, ctx, cond, mask, 1.0)
            eps = O.unet3d_forward(gu, ou, xin, t, ctx, down, mid)
            a_prev = float(ac[t - 250]) if t - 250 >= 0 else 1.0
            x = ddim_ref(eps, x, float(ac[t]), a_prev, 1.0, noise=zs[i], guidance=7.5)[0]
    rel, psnr = metrics("4-step eta = 1 loop vs oracle networks + fp64 update", out, x)
    assert psnr >= 40.0


def test_pipeline_eta_is_seeded_and_leaves_the_default_path_alone(tiny):
    run = tiny["run"]
    before = run()
    a = run(eta=1.0, generator=torch.Generator(device="cuda").manual_seed(9))
    b = run(eta=1.0, generator=torch.Generator(device="cuda").manual_seed(9))
    c = run(eta=1.0, generator=torch.Generator(device="cuda").manual_seed(10))
    after = run(eta=0.0)
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and not torch.equal(a, before)
    assert torch.equal(before, after)
