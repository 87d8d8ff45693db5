"""GPU: the fused CFG + DPM-Solver++ multistep update (nr_cfg_dpmpp_step) at the op, the scheduler and the pipeline level.

The reference of every numeric check is the fp64 restatement of tests/test_dpmpp_host.py (Lu et al. 2022, the 2M solver in the D0 / D1 form
diffusers 0.11.1 ships).  It uses nothing of neurons_amd."""
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_dpmpp_host import BETAS, SOLVERS, ref_m0, ref_orders, ref_step, ref_tables, ref_timesteps  # noqa: E402
from test_engine_gpu import metrics  # noqa: E402

PREDS = ("epsilon", "sample", "v_prediction")
RULES = (("first", "midpoint", 1), ("midpoint", "midpoint", 2), ("heun", "heun", 2))       # (name, solver_type, order)
SIZES = (4 * 4 * 8 * 8, 1031)
GUIDANCE = 7.5
N_TABLE, I_TABLE = 10, 3            # the coefficients of the op tests: step 3 of a 10-step walk (999, 899, 799, [699] -> 599)


def _close(name, got, ref, scale=1.0):
    """fp32 arithmetic of a dozen operations on values of the size of ref: max abs error <= scale * 1e-5 (1 + max|ref|), the bound of
    tests/test_ddim_full_gpu.py."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), name
    err, bound = (got - ref).abs().max().item(), scale * 1e-5 * (1.0 + ref.abs().max().item())
    print(f"[{name}] max_err={err:.3e} bound={bound:.3e}")
    assert err <= bound, (name, err, bound)


_INPUTS = {}


def _inputs(n, cfg):
    """(model output, x, m1): N(0, 1) * 1.5 on a fixed seed, made once per (n, cfg) and left unchanged."""
    if (n, cfg) not in _INPUTS:
        g = torch.Generator().manual_seed(2 * n + (1 if cfg else 0))
        shape = (4, 4, 8, 8) if n == 4 * 4 * 8 * 8 else (n,)
        out = torch.randn((2 if cfg else 1,) + shape, generator=g) * 1.5
        x = torch.randn((1,) + shape, generator=g) * 1.5
        m1 = torch.randn((1,) + shape, generator=g) * 1.5
        _INPUTS[(n, cfg)] = tuple(t.cuda() for t in (out, x, m1))
    return _INPUTS[(n, cfg)]


def _coef(solver_type, order):
    from neurons_amd import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_type=solver_type, **BETAS)
    s.set_timesteps(N_TABLE)
    k = s.step_coefficients(I_TABLE, history=I_TABLE if order == 2 else 0)
    assert k.order == order
    return k


def _op(out, x, m1, k, cfg, pred="epsilon", **kw):
    from neurons_amd import ops
    return ops.cfg_dpmpp_step(out, x, GUIDANCE, k.alpha_s, k.sigma_s, k.c_x, k.c_m0, k.c_m1, m1=m1 if k.order == 2 else None, do_cfg=cfg,
                              prediction_type=pred, **kw)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
@pytest.mark.parametrize("pred", PREDS)
def test_op_matches_fp64_restatement(cuda, pred, rule):
    """n = 1024 takes the 16-byte path; n = 1031 takes it with its scalar tail without guidance and the one-element form with guidance (the
    text half of the model output then starts off a 16-byte boundary).  Measured on an MI355X: at most 1.9 % of the bound (epsilon prediction
    under guidance: 7.5e-6 on x_out against 4.0e-4, 3.5e-5 on m0 against 2.6e-3)."""
    _, solver_type, order = rule
    k = _coef(solver_type, order)
    tabs, ts = ref_tables(), ref_timesteps(N_TABLE)
    for n in SIZES:
        for cfg in (True, False):
            out, x, m1 = _inputs(n, cfg)
            ref, ref0 = ref_step(out.double().cpu(), x.double().cpu(), m1.double().cpu(), tabs, ts, I_TABLE, order, solver_type, pred,
                                 GUIDANCE if cfg else None)
            got, got0 = _op(out, x, m1, k, cfg, pred, return_m0=True)
            assert got.shape == x.shape and got0.shape == x.shape
            _close(f"{pred} {rule[0]} n={n} cfg={cfg}: x_out", got, ref)
            _close(f"{pred} {rule[0]} n={n} cfg={cfg}: m0", got0, ref0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", [True, False])
def test_op_aliases_and_optional_output(cuda, n, cfg):
    out, x, m1 = _inputs(n, cfg)
    for _, solver_type, order in RULES[:2]:
        k = _coef(solver_type, order)
        base, base0 = _op(out, x, m1, k, cfg, return_m0=True)
        only = _op(out, x, m1, k, cfg)                                   # m0_out_dev = NULL
        assert torch.is_tensor(only) and torch.equal(only, base)
        xa = x.clone()
        got, got0 = _op(out, xa, m1, k, cfg, x_out=xa, return_m0=True)   # x_out aliases x
        assert got is xa and torch.equal(xa, base) and torch.equal(got0, base0)
        ma = m1.clone()
        got, got0 = _op(out, x, ma, k, cfg, m0_out=ma)                   # m0_out aliases m1: one history buffer
        assert got0 is ma and torch.equal(got, base) and torch.equal(ma, base0)
    assert torch.equal(x, _inputs(n, cfg)[1])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", [True, False])
def test_first_order_epsilon_step_is_the_merged_ddim_kernel(cuda, n, cfg):
    from neurons_amd import ops
    ac, ts = ref_tables()[0], ref_timesteps(N_TABLE)
    out, x, m1 = _inputs(n, cfg)
    got = _op(out, x, None, _coef("midpoint", 1), cfg)
    ddim = ops.cfg_ddim_step(out, x, GUIDANCE, ac[ts[I_TABLE]], ac[ts[I_TABLE + 1]], cfg)
    _close(f"first order vs nr_cfg_ddim_step n={n} cfg={cfg}", got, ddim.double().cpu())


def test_op_argument_errors(cuda):
    from neurons_amd import _lib, ops
    out, x, m1 = _inputs(1031, False)
    k = _coef("midpoint", 2)
    with pytest.raises(ValueError, match="prediction_type"):
        _op(out, x, m1, k, False, "foo")
    with pytest.raises(RuntimeError, match="m1_dev"):
        ops.cfg_dpmpp_step(out, x, 1.0, k.alpha_s, k.sigma_s, k.c_x, k.c_m0, k.c_m1, m1=None, do_cfg=False)
    lib = _lib.load()
    xo, mo = torch.full_like(x, 123.0), torch.full_like(x, 123.0)
    nan, inf = float("nan"), float("inf")
    good = dict(out=out.data_ptr(), x=x.data_ptr(), m1=m1.data_ptr(), x_out=xo.data_ptr(), m0_out=mo.data_ptr(), n=x.numel(), g=1.0, do_cfg=0,
                pred=0, alpha_s=k.alpha_s, sigma_s=k.sigma_s, c_x=k.c_x, c_m0=k.c_m0, c_m1=k.c_m1)
    bad = [dict(out=None), dict(x=None), dict(x_out=None), dict(n=0), dict(n=-4), dict(pred=3), dict(pred=-1), dict(m1=None),
           dict(alpha_s=0.0), dict(alpha_s=-0.5), dict(alpha_s=1.5), dict(sigma_s=-0.1), dict(sigma_s=1.0),
           dict(m0_out=x.data_ptr()), dict(m0_out=xo.data_ptr()), dict(m0_out=x.data_ptr() + 16)]
    bad += [{name: v} for name in ("g", "alpha_s", "sigma_s", "c_x", "c_m0", "c_m1") for v in (nan, inf)]
    for change in bad:
        a = dict(good, **change)
        st = lib.nr_cfg_dpmpp_step(torch.cuda.current_stream().cuda_stream, *a.values())
        assert st == 1 and len(lib.nr_last_error()) > 0, (change, st)              # NR_ERR_ARG, with a message
    assert lib.nr_cfg_dpmpp_step(torch.cuda.current_stream().cuda_stream, *dict(good, pred=7).values()) == 1
    assert b"prediction type" in lib.nr_last_error()
    torch.cuda.synchronize()
    assert (xo == 123.0).all() and (mo == 123.0).all()                             # refused before any launch
    # the ends of the ranges are valid: alpha_s = 1 with sigma_s = 0, and the history buffer handed in with c_m1 = 0
    assert lib.nr_cfg_dpmpp_step(torch.cuda.current_stream().cuda_stream, *dict(good, alpha_s=1.0, sigma_s=0.0, c_m1=0.0).values()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(xo).all()


# ---- scheduler level --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("solver_type", SOLVERS)
@pytest.mark.parametrize("n", [10, 20])
def test_scheduler_walk(cuda, n, solver_type, pred):
    from neurons_amd import DPMSolverMultistepScheduler
    sched = DPMSolverMultistepScheduler(solver_type=solver_type, prediction_type=pred, steps_offset=1, clip_sample=False, **BETAS)
    shape = (1, 4, 4, 8, 8)
    g = torch.Generator().manual_seed(1000 + n)
    x_start = (torch.randn(shape, generator=g) * 1.5).cuda()
    outs = [(torch.randn(shape, generator=g) * 1.5).cuda() for _ in range(n)]
    tabs, ts, orders = ref_tables(), ref_timesteps(n), ref_orders(n)
    walks = []
    for rep in range(2):
        sched.set_timesteps(n)
        assert sched.timesteps_host == ts
        x, seen = x_start, []
        chain, chain_m1 = x_start.double().cpu(), None          # the restatement's own chain, never fed from the GPU result
        fed_m1 = None                                           # the previous step's x0 prediction from the inputs that step had
        for i, t in enumerate(ts):
            ref, ref0 = ref_step(outs[i].double().cpu(), x.double().cpu(), fed_m1, tabs, ts, i, orders[i], solver_type, pred)
            chain, chain_m1 = ref_step(outs[i].double().cpu(), chain, chain_m1, tabs, ts, i, orders[i], solver_type, pred)
            res = sched.step(outs[i], t, x)
            if rep == 0:
                _close(f"walk N={n} {solver_type} {pred} step {i} (t = {t}, order {orders[i]})", res.prev_sample, ref)
            assert res.prev_sample.dtype == x.dtype
            fed_m1, x = ref0, res.prev_sample
            seen.append(x.clone())
        err, bound = (x.double().cpu() - chain).abs().max().item(), n * 1e-5 * (1.0 + chain.abs().max().item())
        print(f"[walk N={n} {solver_type} {pred} end vs fp64 chain] max_err={err:.3e} bound={bound:.3e} max|chain|={chain.abs().max().item():.1f}")
        assert err <= bound
        walks.append(seen)
    assert all(torch.equal(a, b) for a, b in zip(*walks))       # set_timesteps resets the history: the second walk is the first


# ---- pipeline level ---------------------------------------------------------------------------------------------------------------------
class _Hidden:
    """The same scheduler behind a plain object with only the diffusers surface the reference pipeline touches: no timesteps_host, no marker,
    so the pipeline drives it as a foreign scheduler (scale_model_input, nr_cfg_combine, step(...).prev_sample)."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, inner):
        self._inner = inner
        self.config = types.SimpleNamespace(**vars(inner.config))
        self.steps_seen = []

    @property
    def timesteps(self):
        return self._inner.timesteps

    def set_timesteps(self, n, device=None):
        self._inner.set_timesteps(n, device=device)

    def scale_model_input(self, sample, timestep=None):
        return self._inner.scale_model_input(sample, timestep)

    def add_noise(self, x, noise, t):
        return self._inner.add_noise(x, noise, t)

    def step(self, model_output, timestep, sample, return_dict=True):
        self.steps_seen.append(int(timestep))
        return self._inner.step(model_output, timestep, sample, return_dict=return_dict)


@pytest.fixture(scope="module")
def tiny(cuda):
    from neurons_amd import DDIMScheduler, DPMSolverMultistepScheduler, NeuroclipsPipeline
    from neurons_amd.synth import randn
    from test_shapes_gpu import _nets
    unet, ctrl, ucfg, ccfg, usd, csd = _nets()
    kwargs = dict(steps_offset=1, clip_sample=False, **BETAS)            # the reference's noise_scheduler_kwargs
    dpm, ddim = DPMSolverMultistepScheduler(**kwargs), DDIMScheduler(**kwargs)
    pipe = NeuroclipsPipeline(None, None, None, unet, dpm, ctrl).to("cuda")
    lat = randn("e.lat", (1, 4, 4, 8, 8), 1).cuda()
    noise = randn("e.noise", (1, 4, 4, 8, 8), 2)
    ctx = randn("e.ctx", (2, 77, 64), 3).cuda()
    cimg = (randn("e.cimg", (1, 4, 1, 8, 8), 4) * 0.18215).cuda()

    def run(scheduler=dpm, steps=4, **kw):
        pipe.scheduler = scheduler
        try:
            return pipe("", video_length=4, height=64, width=64, num_inference_steps=steps, low_strength=0.3, output_type="latent", latents=lat,
                        noise=noise, text_embeddings=ctx, controlnet_images=cimg, controlnet_image_index=[0], guidance_scale=GUIDANCE,
                        **kw).videos.clone()
        finally:
            pipe.scheduler = dpm
    return dict(pipe=pipe, dpm=dpm, ddim=ddim, run=run, lat=lat, noise=noise, ctx=ctx, cimg=cimg, ucfg=ucfg, ccfg=ccfg, usd=usd, csd=csd)


def test_pipeline_fused_loop_vs_oracle_networks(tiny, monkeypatch):
    from oracle import animatediff_oracle as O
    calls = []
    real_step = tiny["dpm"].step
    monkeypatch.setattr(tiny["dpm"], "step", lambda *a, **k: (calls.append(1), real_step(*a, **k))[1])
    seen = []
    out = tiny["run"](eta=0.7, generator=torch.Generator(device="cuda").manual_seed(5), callback=lambda i, t, lat: seen.append((i, t)))
    assert calls == []                          # one nr_cfg_dpmpp_step per step, no scheduler.step
    assert out.dtype == tiny["lat"].dtype and tuple(out.shape) == tuple(tiny["lat"].shape)
    ts = ref_timesteps(4)
    assert seen == list(enumerate(ts)) and tiny["pipe"].last_controlnet_group >= 1
    # eta and generator do not reach this scheduler
    assert torch.equal(out, tiny["run"]())

    gu, gc = {k: v.cuda() for k, v in tiny["usd"].items()}, {k: v.cuda() for k, v in tiny["csd"].items()}
    ou, oc = O.OracleConfig.from_native(tiny["ucfg"]), O.OracleConfig.from_native(tiny["ccfg"])
    tabs, orders = ref_tables(), ref_orders(4)
    lat, cimg, ctx = tiny["lat"], tiny["cimg"], tiny["ctx"]
    x = tabs[1][ts[0]] * lat.double().cpu() + tabs[2][ts[0]] * tiny["noise"].double()       # low_strength: noised to timesteps[0], all steps run
    cond = torch.zeros(1, 4, 4, 8, 8, device="cuda")
    mask = torch.zeros(1, 1, 4, 8, 8, device="cuda")
    cond[:, :, [0]] = cimg[:, :, :1]
    mask[:, :, [0]] = 1
    m1 = None
    with torch.no_grad():
        for i, t in enumerate(ts):
            xin = torch.cat([x.float().cuda()] * 2)
            down, mid = O.sparse_controlnet_forward(gc, oc, xin, t, ctx, cond, mask, 1.0)
            eps = O.unet3d_forward(gu, ou, xin, t, ctx, down, mid)
            x, m1 = ref_step(eps.double().cpu(), x, m1, tabs, ts, i, orders[i], "midpoint", "epsilon", GUIDANCE)
    rel, psnr = metrics("4-step DPM-Solver++ loop vs oracle networks + fp64 update", out, x)
    assert psnr >= 40.0


def test_pipeline_hidden_scheduler_takes_the_foreign_branch_and_agrees(tiny):
    fused = tiny["run"]()
    hidden = _Hidden(tiny["dpm"])
    assert not hasattr(hidden, "timesteps_host") and not hasattr(hidden, "native_rule") and not hasattr(hidden, "alpha_pair")
    out = tiny["run"](scheduler=hidden)
    assert hidden.steps_seen == ref_timesteps(4)
    err, bound = (out - fused).abs().max().item(), 4 * 1e-5 * (1.0 + fused.abs().max().item())
    print(f"[hidden scheduler vs fused path] max_err={err:.3e} bound={bound:.3e}")
    assert err <= bound


def test_pipeline_is_repeatable_and_leaves_ddim_alone(tiny):
    run = tiny["run"]
    before = run(scheduler=tiny["ddim"])
    a = run()
    b = run()
    after = run(scheduler=tiny["ddim"])
    assert torch.equal(a, b) and torch.equal(before, after)
    assert torch.isfinite(a).all() and not torch.equal(a, before)


def test_pipeline_20_steps_grouped_sparsectrl(tiny):
    """Four groups of 5 against one SparseCtrl evaluation per step: the group size only changes GEMM tile plans, the bar is that of
    test_pipeline_gpu.test_grouped_sparsectrl_schedule_matches_reference_and_per_step_schedule (>= 55 dB)."""
    pipe, outs = tiny["pipe"], []
    saved = pipe.controlnet_group
    try:
        for grp in (1, 5):
            pipe.controlnet_group = grp
            outs.append(tiny["run"](steps=20))
            assert pipe.last_controlnet_group == grp
    finally:
        pipe.controlnet_group = saved
    assert torch.isfinite(outs[1]).all()
    _, psnr = metrics("20 steps: group 5 vs per-step schedule", outs[1], outs[0])
    assert psnr >= 55.0
