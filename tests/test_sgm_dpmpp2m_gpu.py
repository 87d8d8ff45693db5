"""GPU: the sgm DPM-Solver++ 2M sampler.  The step kernel (nr_edm_cfg_dpmpp2m_step) against an fp64 restatement, its forms against each other and its
first-order step against the Euler kernel; the Gaussian toy model through the C entry point alone; the fused loop, img2img and the engine on the tiny
network against what the reference's own ``DPMPP2MSampler`` recorded (tests/golden/sgm_dpmpp2m_tiny.npz, tools/gen_golden_sgm_dpmpp2m.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLD = os.path.join(HERE, "golden", "sgm_dpmpp2m_tiny.npz")

from test_engine_gpu import metrics  # noqa: E402
from test_sgm_dpmpp2m_host import gauss_bound, refusals  # noqa: E402

U = 2.0 ** -24
# (sigma_prev | None, sigma, sigma_next): a mid-table step, a first step, a last step, a far history (r large), a long step (r small)
TRIPLES = ((3.4, 2.5, 1.8), (None, 14.6, 9.0), (0.06, 0.03, 0.0), (80.0, 2.5, 2.4), (2.6, 2.5, 0.5))
SCALE = 5.0


def _f32(v):
    return float(np.float32(v))


def _step(net, x, old, x_out, den_out, scale, sq, prev, s, nxt, n=None):
    """One nr_edm_cfg_dpmpp2m_step on the current stream; returns the status (the caller checks it)."""
    from neurons_amd import _lib
    return _lib.load().nr_edm_cfg_dpmpp2m_step(torch.cuda.current_stream().cuda_stream, net.data_ptr(), x.data_ptr(),
                                               old.data_ptr() if old is not None else None, x_out.data_ptr(), den_out.data_ptr(),
                                               x.numel() if n is None else n, scale, sq, 0.0 if prev is None else prev, s, nxt)


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(m, generator=g) * 1.5 for m in (2 * n, n, n))          # net [2][n], x, old


def _fp64(net, x, old, prev, s, nxt):
    """include/neurons_amd.h: nr_edm_cfg_dpmpp2m_step in fp64 on the fp32 inputs and the fp32 scalars."""
    from neurons_amd.sgm import dpmpp2m_coefficients
    n = x.numel()
    sq = _f32(0.985 * s)
    nu, nc, xd = net[:n].double(), net[n:].double(), x.double()
    du, dc = nu * (-sq) + xd, nc * (-sq) + xd
    den = du + _f32(SCALE) * (dc - du)
    c_x, c_d, c_o = dpmpp2m_coefficients(None if prev is None else _f32(prev), _f32(s), _f32(nxt))
    out = c_x * xd + c_d * den
    if c_o is not None:
        out = out + c_o * old.double()
    return out, den, sq


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "-".join(str(v) for v in t))
@pytest.mark.parametrize("n", (1024, 1031))
def test_step_matches_fp64(cuda, n, triple):
    """Both outputs within 1e-5 (1 + max |ref|) of fp64, the bound tests/test_sampler_steps_gpu.py applies to the other rules; n = 1031 takes the
    one-element form (the text half would start off a 16-byte boundary), n = 1024 the 16-byte one."""
    prev, s, nxt = triple
    net, x, old = _inputs(n, 7 * n + int(10 * s))
    want_x, want_den, sq = _fp64(net, x, old, prev, s, nxt)
    d = [t.to(cuda) for t in (net, x, old)]
    x_out, den_out = torch.empty(n, device=cuda), torch.empty(n, device=cuda)
    assert _step(d[0], d[1], None if prev is None else d[2], x_out, den_out, SCALE, sq, prev, s, nxt) == 0
    for name, got, want in (("x_out", x_out, want_x), ("denoised_out", den_out, want_den)):
        err = (got.double().cpu() - want).abs().max().item()
        bound = 1e-5 * (1.0 + want.abs().max().item())
        print(f"[dpmpp2m step {triple} n={n} {name}] max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert torch.isfinite(got).all() and err <= bound
    if nxt == 0.0:
        assert torch.equal(x_out, den_out)                      # c_x = 0, c_d = 1 exactly: the step returns the denoised estimate, bit for bit


def _shifted(v, dev):
    buf = torch.empty(v.numel() + 1, device=dev)
    buf[1:].copy_(v)
    out = buf[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("n", (1024, 1031, 3))
@pytest.mark.parametrize("hist", (True, False), ids=("second-order", "first-order"))
def test_forms_agree_bit_for_bit(cuda, n, hist):
    """Aligned bases (16-byte form at n % 4 == 0) and bases one float off alignment (one-element form) give identical bits; so do the ragged n;
    in place (x_out = x, denoised_out = old) equals out of place."""
    prev, s, nxt = (3.4 if hist else None), 2.5, 1.8
    net, x, old = _inputs(n, 31 * n)
    sq = _f32(0.985 * s)

    def run(place, inplace):
        dn, dx, do = place(net), place(x), place(old)
        x_out, den_out = (dx, do) if inplace else (place(torch.zeros(n)), place(torch.zeros(n)))
        assert _step(dn, dx, do if hist else None, x_out, den_out, SCALE, sq, prev, s, nxt) == 0
        return x_out.clone(), den_out.clone()

    aligned = run(lambda v: v.to(cuda).clone(), False)
    for place in (lambda v: v.to(cuda).clone(), lambda v: _shifted(v, cuda)):
        for inplace in (False, True):
            got = run(place, inplace)
            assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1])
    # only the input off alignment, only an output off alignment: every vector-loaded base is checked
    dn, dx, do = net.to(cuda), x.to(cuda), old.to(cuda)
    for which in range(5):
        bufs = [dn, dx, do, torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)]
        if which == 2 and not hist:
            continue
        bufs[which] = _shifted(bufs[which].cpu(), cuda)
        assert _step(bufs[0], bufs[1], bufs[2] if hist else None, bufs[3], bufs[4], SCALE, sq, prev, s, nxt) == 0
        assert torch.equal(bufs[3], aligned[0]) and torch.equal(bufs[4], aligned[1])


@pytest.mark.parametrize("n", (1024, 1031))
def test_first_order_step_is_the_euler_kernel_step(cuda, n):
    """NULL history: x' = (s'/s) x - expm1(-h) den is algebraically Euler's x + (x - den) / s (s' - s); within 1e-5 (1 + max |ref|) of
    nr_edm_cfg_euler_step.  A history buffer with sigma_next = 0 is first order too: x_out == denoised_out bit for bit, the history is not read."""
    from neurons_amd import _lib
    lib = _lib.load()
    net, x, _ = (t.to(cuda) for t in _inputs(n, 5 * n))
    for s, nxt in ((14.6, 9.0), (2.5, 1.8), (0.03, 0.0)):
        sq = _f32(0.985 * s)
        want = torch.empty(n, device=cuda)
        _lib.check(lib.nr_edm_cfg_euler_step(torch.cuda.current_stream().cuda_stream, net.data_ptr(), x.data_ptr(), want.data_ptr(), n, SCALE, sq,
                                             s, nxt))
        x_out, den_out = torch.empty(n, device=cuda), torch.empty(n, device=cuda)
        assert _step(net, x, None, x_out, den_out, SCALE, sq, None, s, nxt) == 0
        err = (x_out - want).abs().max().item()
        bound = 1e-5 * (1.0 + want.abs().max().item())
        print(f"[dpmpp2m first order vs euler kernel, sigma {s} -> {nxt}, n={n}] max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    nan_hist = torch.full((n,), float("nan"), device=cuda)
    x_out, den_out = torch.empty(n, device=cuda), torch.empty(n, device=cuda)
    assert _step(net, x, nan_hist, x_out, den_out, SCALE, _f32(0.03), float("nan"), 0.03, 0.0) == 0      # sigma_prev is not read either
    assert torch.equal(x_out, den_out) and torch.isfinite(x_out).all()


def test_entry_refuses_bad_arguments_with_nothing_launched(cuda):
    """Every refusal of include/neurons_amd.h: status and message, and the output buffers keep their fill."""
    from neurons_amd import _lib
    lib = _lib.load()
    p, q, r = torch.full((64,), 7.0, device=cuda), torch.full((64,), 8.0, device=cuda), torch.full((128,), 9.0, device=cuda)
    for args, status in refusals(p.data_ptr(), q.data_ptr(), r.data_ptr()):
        st = lib.nr_edm_cfg_dpmpp2m_step(torch.cuda.current_stream().cuda_stream, *args)
        assert st == status, (st, status, args)
        assert lib.nr_last_error()
    # partly overlapping buffers, and an output on top of an input other than its own
    big = torch.zeros(256, device=cuda)
    e = big.element_size()
    for args in ((r.data_ptr(), big.data_ptr(), q.data_ptr(), big.data_ptr() + 4 * e, q.data_ptr()),          # x_out half over x
                 (r.data_ptr(), p.data_ptr(), big.data_ptr(), p.data_ptr(), big.data_ptr() + 4 * e),          # denoised_out half over old
                 (r.data_ptr(), p.data_ptr(), q.data_ptr(), p.data_ptr(), p.data_ptr()),                      # denoised_out = x
                 (r.data_ptr(), p.data_ptr(), q.data_ptr(), r.data_ptr(), q.data_ptr())):                     # x_out = net
        assert lib.nr_edm_cfg_dpmpp2m_step(torch.cuda.current_stream().cuda_stream, *args, 64, 5.0, 2.4, 3.4, 2.5, 1.8) == 1
    torch.cuda.synchronize()
    assert (p == 7.0).all() and (q == 8.0).all() and (r == 9.0).all() and (big == 0.0).all()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_gaussian_model_through_the_entry_points_alone(cuda, gold):
    """No network: the exact denoiser x / (1 + sigma^2) of N(0, 1) data is handed in as the eps both halves would give, net = x sigma / (1 + sigma^2)
    with sigma_quantized = sigma.  Finals within ``gauss_bound`` (tests/test_sgm_dpmpp2m_host.py) of the reference's recorded finals; the end error
    against the exact solution orders as the reference's does: 2M at 19 steps <= Euler at 38."""
    from neurons_amd import _lib
    from neurons_amd.sgm import LegacyDDPMDiscretization
    lib = _lib.load()
    gx = torch.from_numpy(gold["gauss.x"]).to(cuda)
    exact = gold["gauss.exact"]
    n = gx.numel()
    err = {}
    for name, steps in (("euler", 38), ("dpmpp2m", 19), ("dpmpp2m", 38), ("dpmpp2m", 10), ("euler", 20)):
        sig = [float(v) for v in LegacyDDPMDiscretization()(steps)]
        x = (gx * torch.sqrt(1.0 + torch.tensor(sig[0]) ** 2.0).to(cuda)).contiguous()
        old = torch.empty_like(x)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(steps):
            s = sig[i]
            net = (x * (s / (1.0 + s * s))).repeat(2, 1, 1, 1)
            if name == "euler":
                x_new = torch.empty_like(x)
                _lib.check(lib.nr_edm_cfg_euler_step(stream, net.data_ptr(), x.data_ptr(), x_new.data_ptr(), n, SCALE, s, s, sig[i + 1]))
                x = x_new
            else:
                _lib.check(lib.nr_edm_cfg_dpmpp2m_step(stream, net.data_ptr(), x.data_ptr(), old.data_ptr() if i else None, x.data_ptr(),
                                                       old.data_ptr(), n, SCALE, s, sig[i - 1] if i else 0.0, s, sig[i + 1]))
        ref = gold[f"gauss.{name}_{steps}"]
        got = x.cpu().numpy().astype(np.float64)
        d = np.abs(got - ref).max()
        err[name, steps] = np.linalg.norm(got - exact) / np.linalg.norm(exact)
        print(f"[gaussian model on the GPU, {name} {steps} steps] max |got - reference| = {d:.2e} (bound {gauss_bound(steps, ref):.2e}), "
              f"end error {err[name, steps]:.4f} (reference {float(gold[f'gauss.err_{name}_{steps}']):.4f})")
        assert np.isfinite(got).all() and d <= gauss_bound(steps, ref)
    assert err["dpmpp2m", 19] <= err["euler", 38] and err["dpmpp2m", 10] <= err["euler", 20]


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop on the tiny network
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine(cuda, **kw):
    from neurons_amd.sgm import NativeDiffusionEngine, sgm_random_state_dict
    from neurons_amd.vae import vae_random_state_dict
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    cfg, vcfg = tiny_sgm_config(), tiny_vae_config()
    eng = NativeDiffusionEngine(network_config=cfg, first_stage_config=vcfg, scale=5.0, **kw)
    eng.eval().requires_grad_(False)
    eng.to(cuda)
    ck = {"model.diffusion_model." + k: v for k, v in sgm_random_state_dict(cfg, seed=71).items()}
    ck.update({"first_stage_model." + k: v for k, v in vae_random_state_dict(vcfg, seed=91).items()})
    eng.load_state_dict(ck)
    return eng


@pytest.fixture(scope="module")
def rig(cuda, gold):
    """One tiny engine (U-Net seed 71, decoder 91: the weights of the fixtures) with the default sampler, and the fixture's tensors on the GPU; tests
    bring their own sampler objects and leave the engine's as it is."""
    eng = _engine(cuda, num_steps=5)
    t = {k: torch.from_numpy(gold[k]).to(cuda) for k in ("ctx", "uc_ctx", "vec", "x_in", "z_init", "noise", "offset")}
    t["c"] = {"crossattn": t["ctx"], "vector": t["vec"]}
    t["uc"] = {"crossattn": t["uc_ctx"], "vector": t["vec"]}
    return eng, t


def _count_calls(monkeypatch, name):
    from neurons_amd import _lib
    lib = _lib.load()
    real, n = getattr(lib, name), [0]

    def counting(*a):
        n[0] += 1
        return real(*a)

    monkeypatch.setattr(lib, name, counting)
    return n


@pytest.mark.parametrize("steps", (4, 10))
def test_fused_loop_matches_reference_recording(rig, gold, monkeypatch, steps):
    """The fused loop on the tiny network against the reference's DPMPP2MSampler: final >= 40 dB (the loop bar of tests/test_sgm_gpu.py); x and
    denoised after step 1 (first order, writes the history) and step 2 (the first to read it, with sigma_prev) >= 40 dB too, so a history or
    sigma_prev slip shows where it happens.  One network evaluation and one step launch per step."""
    from neurons_amd.sgm import DPMPP2MSampler
    eng, t = rig
    evals, launches = _count_calls(monkeypatch, "nr_sgm_unet_forward"), _count_calls(monkeypatch, "nr_edm_cfg_dpmpp2m_step")
    rec = []
    x_in = t["x_in"].clone()
    final = DPMPP2MSampler(num_steps=steps, scale=5.0)(eng.native_denoiser(), x_in, cond=t["c"], uc=t["uc"], record=rec)
    assert evals[0] == launches[0] == steps == int(gold[f"loop{steps}.calls"]) == len(rec)
    assert torch.equal(x_in, t["x_in"])                          # the caller's start is not written
    for i in (0, 1):
        for j, name in enumerate(("xs", "dens")):
            _, psnr = metrics(f"dpmpp2m {steps} steps: {name[:-1]} after step {i + 1} vs reference", rec[i][j], gold[f"loop{steps}.{name}"][i])
            assert psnr >= 40.0, (i, name, psnr)
    _, psnr = metrics(f"dpmpp2m {steps} steps: final vs reference", final, gold[f"loop{steps}.final"])
    assert psnr >= 40.0
    assert torch.equal(final, rec[-1][0]) and torch.equal(rec[-1][0], rec[-1][1])        # the step to sigma = 0 returns the denoised estimate


def test_fused_agrees_with_generic_on_the_same_native_network(rig):
    """A closure the sampler cannot recognise runs the reference's loop in torch around the same HIP network.  Euler's fused-against-generic rel-L2 on
    the same inputs is the parent's path (its gate: 1e-3, tests/test_sgm_gpu.py); 2M may be at most 3x that: its update weights the two denoised
    estimates by 1 + 1/r, about 2 on these tables."""
    from neurons_amd.sgm import DPMPP2MSampler, EulerEDMSampler
    eng, t = rig
    box = {"den": eng.denoiser, "model": eng.model}

    def foreign(x, sigma, cc):
        return box["den"](box["model"], x, sigma, cc)

    rel = {}
    for cls in (EulerEDMSampler, DPMPP2MSampler):
        s = cls(num_steps=4, scale=5.0)
        assert s._native_network(foreign) is None
        a = s(foreign, t["x_in"], cond=t["c"], uc=t["uc"])
        b = s(eng.native_denoiser(), t["x_in"], cond=t["c"], uc=t["uc"])
        rel[cls.__name__], _ = metrics(f"{cls.__name__}: generic (foreign closure) vs fused, 4 steps", a, b)
    print(f"[fused vs generic rel-L2] Euler {rel['EulerEDMSampler']:.3e}, DPM++ 2M {rel['DPMPP2MSampler']:.3e}, "
          f"ratio {rel['DPMPP2MSampler'] / max(rel['EulerEDMSampler'], 1e-30):.2f}")
    assert rel["EulerEDMSampler"] < 1e-3
    assert rel["DPMPP2MSampler"] <= 3.0 * rel["EulerEDMSampler"]


class _Recording:
    """What do_img2img / unclip_sample touch of a sampler (.discretization, settable; .num_steps; the call), keeping the start it is handed."""

    def __init__(self, sampler):
        self.sampler, self.num_steps, self.start = sampler, sampler.num_steps, None

    @property
    def discretization(self):
        return self.sampler.discretization

    @discretization.setter
    def discretization(self, d):
        self.sampler.discretization = d

    def __call__(self, denoiser, x, cond=None, uc=None):
        self.start = x.clone()
        return self.sampler(denoiser, x, cond=cond, uc=uc)


def _check_start(got, gold, strength, sl=slice(None)):
    """The start is fp32 arithmetic on the recorded inputs: the kernel's rounding bound (6 roundings) plus that of the reference's fp32 evaluation (8),
    as tests/test_sgm_img2img_gpu.py derives them, plus 2 for a sigma0 that may differ from the recording's in its last bit (see the caller)."""
    z, nz, off = (gold[k][sl].astype(np.float64) for k in ("z_init", "noise", "offset"))
    s0, lvl = float(gold[f"i2i{strength}.sig"][0]), _f32(float(gold["offset_noise_level"]))
    den = (1.0 + s0 * s0) ** 0.5
    A = (np.abs(z) + (np.abs(nz) + np.abs(lvl * off)[:, None, None, None]) * s0) / den
    g = lambda k: k * U / (1 - k * U)                                                      # noqa: E731
    err = np.abs(got.double().cpu().numpy() - gold[f"i2i{strength}.start"][sl].astype(np.float64))
    assert (err <= (g(6) + g(8) + g(2)) * A + 1e-37).all(), (err / A).max()


@pytest.mark.parametrize("strength", (0.5, 1.0))
def test_img2img_matches_reference_recording(rig, gold, monkeypatch, strength):
    """The reference's do_img2img(skip_encode=True) with its DPMPP2MSampler on a pruned table, 10 steps: through do_img2img, and sample by sample
    through unclip_sample(init=<latent>, strength=) (it repeats one token set over its batch; the fixture's samples have their own).  Starts equal
    the recording's to rounding, final z >= 40 dB, len(pruned) - 1 network evaluations; the first step of the pruned table has no history."""
    from neurons_amd.sgm import DPMPP2MSampler, Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization, do_img2img, unclip_sample
    eng, t = rig
    steps, level = int(gold["i2i_steps"]), float(gold["offset_noise_level"])
    pruned = gold[f"i2i{strength}.sig"]
    # the table is fp32 pow of fp64 schedule values, formed on the host: between hosts an entry may differ in its last bit, no more
    table = Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), strength)(steps).double().numpy()
    dt = np.abs(table - pruned) / (2 * U * np.maximum(pruned, 1e-30))
    print(f"[pruned table at strength {strength} vs the recording] max difference {dt.max():.2f} ulp")
    assert table.shape == pruned.shape and dt.max() <= 1.0 and table[-1] == 0.0
    evals = _count_calls(monkeypatch, "nr_sgm_unet_forward")
    rec = _Recording(DPMPP2MSampler(num_steps=steps, scale=5.0, discretization=Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), strength)))
    img, z = do_img2img(t["z_init"], eng, rec, t["c"], t["uc"], t["noise"], offset_noise_level=level, offset=t["offset"], skip_encode=True,
                        return_latents=True)
    assert evals[0] == len(pruned) - 1 == int(gold[f"i2i{strength}.calls"])
    assert tuple(img.shape) == (2, 3, 64, 64) and img.min().item() >= 0.0 and img.max().item() <= 1.0
    _check_start(rec.start, gold, strength)
    _, psnr = metrics(f"dpmpp2m do_img2img strength {strength}: final z vs reference", z, gold[f"i2i{strength}.z"])
    assert psnr >= 40.0
    full = LegacyDDPMDiscretization()
    rec = _Recording(DPMPP2MSampler(num_steps=steps, scale=5.0, discretization=full))
    zs = []
    for k in range(2):
        evals[0] = 0
        sl = slice(k, k + 1)
        zs.append(unclip_sample(eng, t["ctx"][sl], t["vec"][sl], None, t["noise"][sl], t["uc_ctx"][sl], rec, offset_noise=t["offset"][sl],
                                offset_noise_level=level, init=t["z_init"][sl], strength=strength))
        assert evals[0] == len(pruned) - 1 and rec.discretization is full
        _check_start(rec.start, gold, strength, sl)
    _, psnr = metrics(f"dpmpp2m unclip_sample(init=, strength={strength}): final z vs reference", torch.cat(zs), gold[f"i2i{strength}.z"])
    assert psnr >= 40.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine, driven as utils.unclip_recon drives it
# ---------------------------------------------------------------------------------------------------------------------------------
def test_engine_option_runs_the_unclip_recon_call_sequence_and_leaves_euler_alone(cuda, monkeypatch):
    """NativeDiffusionEngine(sampler="dpmpp_2m") through the call sequence of utils.unclip_recon (oracle/unclip_harness.py, the draws of
    tests/golden/unclip_tiny.npz): runs on the fused path and is repeatable bit for bit.  On the same engine an Euler sampler gives the same bits
    before and after a 2M call, and a DPMPP2MSampler merely assigned to ``.sampler`` (its ``_engine`` left None) takes the fused path as well."""
    from neurons_amd.sgm import DPMPP2MSampler, EulerEDMSampler
    from oracle.unclip_harness import call_like_unclip_recon
    g = np.load(os.path.join(HERE, "golden", "unclip_tiny.npz"))
    steps = int(g["num_steps"])
    eng = _engine(cuda, num_steps=steps, sampler="dpmpp_2m")
    assert type(eng.sampler) is DPMPP2MSampler
    t = {k: torch.from_numpy(g[k]) for k in ("tokens", "vector_suffix", "z", "uc_tokens", "noise", "offset")}
    launches = _count_calls(monkeypatch, "nr_edm_cfg_dpmpp2m_step")
    euler_launches = _count_calls(monkeypatch, "nr_edm_cfg_euler_step")

    def run():
        return call_like_unclip_recon(t["tokens"].to(cuda), eng, t["vector_suffix"].to(cuda), t, num_samples=1, offset_noise_level=0.04, device=cuda)

    a = run()
    assert launches[0] == steps and euler_launches[0] == 0
    assert tuple(a.shape) == (1, 3, 768, 768) and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(run(), a) and launches[0] == 2 * steps
    eng.sampler = EulerEDMSampler(num_steps=steps, scale=5.0)
    e0 = run()
    assert launches[0] == 2 * steps and euler_launches[0] == steps
    eng.sampler = DPMPP2MSampler(num_steps=steps, scale=5.0)                 # plain assignment: _engine stays None, the closure is still recognised
    assert eng.sampler._engine is None
    assert torch.equal(run(), a) and launches[0] == 3 * steps
    eng.sampler = EulerEDMSampler(num_steps=steps, scale=5.0)
    assert torch.equal(run(), e0) and euler_launches[0] == 2 * steps and launches[0] == 3 * steps
    assert not torch.equal(e0, a)
