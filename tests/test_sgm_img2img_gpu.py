"""GPU: sgm img2img.  The start kernel (nr_edm_img2img_start) against an fp64 restatement of its three lines; the pruned-table Euler loop,
``do_img2img``, ``encode_first_stage`` and ``unclip_sample(init=, strength=)`` on the tiny network against what the reference's own
``do_img2img`` recorded (tests/golden/sgm_img2img_tiny.npz, tools/gen_golden_sgm_img2img.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLD = os.path.join(HERE, "golden", "sgm_img2img_tiny.npz")

from test_engine_gpu import metrics  # noqa: E402

U = 2.0 ** -24          # fp32 unit roundoff: one correctly rounded operation has relative error <= U; 1 ulp is at most 2 U


def _gamma(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel against fp64
# ---------------------------------------------------------------------------------------------------------------------------------
def _inputs(mode, batch, nps, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(noise=torch.randn(batch, nps, generator=g), offset=torch.randn(batch, generator=g))
    if mode == 0:
        t["z"] = torch.randn(batch, nps, generator=g)
    else:
        mom = torch.randn(batch, 2, nps, generator=g)
        mom[:, 1] *= 3.0
        # logvar beyond both clamp bounds (-30, 20), on the first / last elements so that the vector body and the tail both meet them
        lv = mom[:, 1]                                   # a view: [batch][nps]
        lv[:, 0::5] = 25.0
        lv[:, 1::7] = -41.0
        lv[:, -1] = 33.0
        t["moments"] = mom
        t["enc_noise"] = torch.randn(batch, nps, generator=g)
    return t


def _reference_and_bound(mode, t, sigma0, level, z_scale, use_offset):
    """fp64 restatement of include/neurons_amd.h: nr_edm_img2img_start on the fp32 inputs, and the rounding bound of the fp32 evaluation.

    Roundings on the way of the term that meets the most of them (each <= U relative to a partial result whose magnitude is at most the sum A of
    the absolute values of the terms; sigma0 = 0 and the clamp are exact, 0.5 * logvar is exact):
      mode 0:  level * o (1), noise + . (1), . * sigma0 (1), z + . (1), / den (1), den = fl(sqrt(1 + sigma0^2)) (1)                     = 6
      mode 1:  expf (1 ulp = 2 U), . * eps (1), mean + . (1), . * z_scale (1), z + . (1), / den (1), den (1)                            = 8
    so |got - want| <= gamma_k * A with gamma_k = k U / (1 - k U): "a few fp32 ulps" of the fp64 value wherever the terms do not cancel, and the
    honest bound where they do.  A contracted multiply-add rounds once less and stays inside."""
    d = {k: v.double() for k, v in t.items()}
    s = float(np.float32(sigma0))
    lvl = float(np.float32(level))
    zs = float(np.float32(z_scale))
    if mode == 0:
        z, az, k = d["z"], d["z"].abs(), 6
    else:
        mean, lv = d["moments"][:, 0], d["moments"][:, 1].clamp(-30.0, 20.0)
        std = torch.exp(0.5 * lv)
        z = (mean + std * d["enc_noise"]) * zs
        az, k = (mean.abs() + std * d["enc_noise"].abs()) * abs(zs), 8
    off = lvl * d["offset"][:, None] if use_offset else torch.zeros_like(d["noise"][:, :1])
    den = (1.0 + s * s) ** 0.5
    want = (z + (d["noise"] + off) * s) / den
    A = (az + (d["noise"].abs() + off.abs()) * s) / den
    return want, _gamma(k) * A + float(np.finfo(np.float32).tiny)


def _check(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    ratio = (err / bound).max().item()
    ulps = (err / (want.abs() * 2 * U + float(np.finfo(np.float32).tiny))).max().item()
    print(f"[{name}] max err / bound = {ratio:.3f}, max error {ulps:.2f} ulp of the fp64 value, max abs err {err.max().item():.3e}")
    assert torch.isfinite(got).all() and ratio <= 1.0, (name, ratio)


NPS = (1, 7, 4 * 8 * 8, 4 * 8 * 8 + 5)


@pytest.mark.parametrize("sigma0", (0.0, 0.03, 14.6))
@pytest.mark.parametrize("nps", NPS)
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("mode", (0, 1))
def test_start_kernel_matches_fp64(cuda, mode, batch, nps, sigma0):
    from neurons_amd.sgm import edm_img2img_start
    t = _inputs(mode, batch, nps, seed=1000 * mode + 100 * batch + nps)
    dev = {k: v.to(cuda) for k, v in t.items()}
    level, zs = 0.04, (0.18215 if mode else 1.0)
    src = dict(z=dev["z"]) if mode == 0 else dict(moments=dev["moments"], enc_noise=dev["enc_noise"], z_scale=zs)
    got = edm_img2img_start(dev["noise"], sigma0, offset=dev["offset"], offset_noise_level=level, **src)
    assert got.shape == (batch, nps) and got.dtype == torch.float32
    want, bound = _reference_and_bound(mode, t, sigma0, level, zs, True)
    _check(f"img2img start mode {mode} batch {batch} n {nps} sigma0 {sigma0}", got, want, bound)
    # offset_noise_level 0 / offset NULL: noise' = noise
    want0, bound0 = _reference_and_bound(mode, t, sigma0, 0.0, zs, False)
    for kw in (dict(offset=None, offset_noise_level=level), dict(offset=dev["offset"], offset_noise_level=0.0)):
        g0 = edm_img2img_start(dev["noise"], sigma0, **kw, **src)
        _check(f"  no offset ({'NULL' if kw['offset'] is None else 'level 0'})", g0, want0, bound0)
    if sigma0 == 0.0 and mode == 0:
        assert torch.equal(got, dev["z"])                                  # (z + n * 0) / 1
    if mode == 0:                                                          # in place: out = z_in
        zbuf = dev["z"].clone()
        r = edm_img2img_start(dev["noise"], sigma0, z=zbuf, out=zbuf, offset=dev["offset"], offset_noise_level=level)
        assert r is zbuf and torch.equal(zbuf, got)


@pytest.mark.parametrize("mode", (0, 1))
def test_start_kernel_unaligned_bases_take_the_scalar_form(cuda, mode):
    """Bases 4 bytes off a 16-byte boundary: the launcher must not issue 16-byte accesses; results equal the aligned call's bit for bit."""
    from neurons_amd.sgm import edm_img2img_start
    batch, nps = 3, 4 * 8 * 8 + 5
    t = _inputs(mode, batch, nps, seed=77)
    level, s0 = 0.04, 0.7

    def shifted(v):
        buf = torch.empty(v.numel() + 1, device=cuda)
        buf[1:].copy_(v.reshape(-1))
        out = buf[1:].view(v.shape)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out

    a = {k: v.to(cuda) for k, v in t.items()}
    b = {k: shifted(v) for k, v in t.items()}
    outs = []
    for d in (a, b):
        src = dict(z=d["z"]) if mode == 0 else dict(moments=d["moments"], enc_noise=d["enc_noise"], z_scale=0.18215)
        outs.append(edm_img2img_start(d["noise"], s0, offset=d["offset"], offset_noise_level=level, **src))
    want, bound = _reference_and_bound(mode, t, s0, level, 0.18215 if mode else 1.0, True)
    _check(f"img2img start mode {mode}, unaligned bases", outs[1], want, bound)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop on the tiny network
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def rig(cuda, gold):
    """One tiny engine (U-Net seed 71, decoder 91, encoder 94: the weights of the fixture) and the fixture's tensors on the GPU, shared by every test
    below; nothing here is modified by a test."""
    from neurons_amd.sgm import NativeDiffusionEngine, sgm_random_state_dict
    from neurons_amd.vae import vae_random_state_dict
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    cfg, vcfg = tiny_sgm_config(), tiny_vae_config()
    eng = NativeDiffusionEngine(network_config=cfg, first_stage_config=vcfg, num_steps=int(gold["num_steps"]), scale=5.0,
                                scale_factor=float(gold["scale_factor"]))
    eng.eval().requires_grad_(False)
    eng.to(cuda)
    ck = {"model.diffusion_model." + k: v for k, v in sgm_random_state_dict(cfg, seed=71).items()}
    ck.update({"first_stage_model." + k: v for k, v in vae_random_state_dict(vcfg, seed=91).items()})
    ck.update({"first_stage_model." + k: v for k, v in vae_random_state_dict(vcfg, seed=94, encoder=True).items()})
    eng.load_state_dict(ck)
    t = {k: torch.from_numpy(gold[k]).to(cuda) for k in ("img", "z_init", "ctx", "uc_ctx", "vec", "noise", "enc_noise", "offset")}
    t["c"] = {"crossattn": t["ctx"], "vector": t["vec"]}
    t["uc"] = {"crossattn": t["uc_ctx"], "vector": t["vec"]}
    return eng, t


def _sampler(eng, strength, steps=None):
    from neurons_amd.sgm import EulerEDMSampler, Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    return EulerEDMSampler(num_steps=steps or eng.sampler.num_steps, scale=5.0,
                           discretization=Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), strength))


def _run(eng, t, gold, skip, strength, **kw):
    from neurons_amd.sgm import do_img2img
    return do_img2img(t["z_init"] if skip else t["img"], eng, _sampler(eng, strength), t["c"], t["uc"], t["noise"],
                      offset_noise_level=float(gold["offset_noise_level"]), offset=t["offset"], skip_encode=skip, return_latents=True,
                      enc_noise=None if skip else t["enc_noise"], **kw)


def _count_calls(monkeypatch, name):
    from neurons_amd import _lib
    lib = _lib.load()
    real, n = getattr(lib, name), [0]

    def counting(*a):
        n[0] += 1
        return real(*a)

    monkeypatch.setattr(lib, name, counting)
    return n


def _psnr01(got, want):
    return 10 * np.log10(1.0 / (((got - want) ** 2).mean().item() + 1e-20))


@pytest.mark.parametrize("strength", (0.0, 0.5, 1.0))
@pytest.mark.parametrize("skip", (True, False), ids=("skip_encode", "encode"))
def test_do_img2img_matches_reference_recording(rig, gold, monkeypatch, skip, strength):
    """do_img2img on the tiny network, 8x8 latent (the encode case from a 64x64 image), 10 steps, 2 samples, against the reference's own
    do_img2img.  Gate: the one tests/test_sgm_gpu.py applies to unclip_tiny (image PSNR >= 35 dB on [0, 1], mean within 5e-3).  The network is
    evaluated exactly len(pruned table) - 1 times (counted at the C entry)."""
    eng, t = rig
    tag = f"{'skip' if skip else 'enc'}{strength}"
    calls = _count_calls(monkeypatch, "nr_sgm_unet_forward")
    img, z = _run(eng, t, gold, skip, strength)
    pruned = gold[f"sig_{int(gold['num_steps'])}_{strength}"]
    assert calls[0] == len(pruned) - 1 == int(gold[f"{tag}.calls"]), (calls[0], len(pruned))
    assert tuple(img.shape) == (2, 3, 64, 64) and tuple(z.shape) == (2, 4, 8, 8) and img.dtype == torch.float32
    metrics(f"img2img {tag}: final latents vs reference", z, gold[f"{tag}.z"])
    want = torch.from_numpy(gold[f"{tag}.img"].astype(np.float32))
    psnr = _psnr01(img.float().cpu(), want)
    dmean = abs(img.double().mean().item() - float(gold[f"{tag}.img_mean"]))
    print(f"[img2img {tag}: images vs reference] psnr={psnr:.1f} dB  |mean diff|={dmean:.2e}")
    assert psnr >= 35.0, psnr
    assert dmean < 5e-3, dmean
    assert img.min().item() >= 0.0 and img.max().item() <= 1.0


@pytest.mark.parametrize("strength", (0.0, 0.5, 1.0))
def test_noised_start_matches_reference_recording(rig, gold, strength):
    """The start handed to the sampler.  skip_encode: pure fp32 arithmetic on the recorded inputs, so the kernel's own rounding bound (6 roundings,
    see _reference_and_bound) plus the bound of the reference's fp32 evaluation.  encode: through the bf16 encoder, so the VAE encoder gate of
    tests/test_vae_gpu.py (PSNR >= 40 dB)."""
    from neurons_amd.sgm import edm_img2img_start
    eng, t = rig
    sig0 = float(gold[f"sig_{int(gold['num_steps'])}_{strength}"][0])
    level = float(gold["offset_noise_level"])
    got = edm_img2img_start(t["noise"], sig0, z=t["z_init"], offset=t["offset"], offset_noise_level=level)
    n = t["noise"].shape[0]
    host = dict(z=t["z_init"].cpu().reshape(n, -1), noise=t["noise"].cpu().reshape(n, -1), offset=t["offset"].cpu())
    want64, bound = _reference_and_bound(0, host, sig0, level, 1.0, True)
    rec = torch.from_numpy(gold[f"skip{strength}.start"]).reshape(n, -1).double()
    # the recording is torch's fp32 evaluation of the same lines, whose denominator sqrt(1 + sigma0 ** 2) is formed in fp32 (pow, add, sqrt: 3
    # roundings where the kernel's host-side double has 1): 8 roundings, gamma_8 A
    A = (bound - float(np.finfo(np.float32).tiny)) / _gamma(6)
    assert ((rec - want64).abs() <= _gamma(8) * A + 1e-37).all()
    _check(f"img2img start (skip_encode), strength {strength}, vs fp64", got.reshape(n, -1), want64, bound)
    assert ((got.cpu().reshape(n, -1).double() - rec).abs() <= (_gamma(6) + _gamma(8)) * A + 1e-37).all()
    moments = eng.encode_first_stage_moments(t["img"])
    got = edm_img2img_start(t["noise"], sig0, moments=moments, enc_noise=t["enc_noise"], z_scale=eng.scale_factor, offset=t["offset"],
                            offset_noise_level=level)
    rel, psnr = metrics(f"img2img start from the encoder's moments, strength {strength}", got, gold[f"enc{strength}.start"])
    assert psnr >= 40.0


def test_encode_first_stage_matches_reference_recording(rig, gold):
    """encode_first_stage = scale_factor * posterior SAMPLE (the regularizer's default), at the VAE encoder gate of tests/test_vae_gpu.py."""
    eng, t = rig
    lat = eng.encode_first_stage(t["img"], noise=t["enc_noise"])
    rel, psnr = metrics("encode_first_stage vs reference", lat, gold["enc_latent"])
    assert psnr >= 40.0
    assert torch.equal(lat, eng.encode_first_stage(t["img"], noise=t["enc_noise"]))
    # the variant that draws as the reference does: host randn(mean.shape) from the global generator, after the encoder ran
    torch.manual_seed(5)
    a = eng.encode_first_stage(t["img"])
    torch.manual_seed(5)
    eps = torch.randn(lat.shape)
    assert torch.equal(a, eng.encode_first_stage(t["img"], noise=eps.to(lat.device)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.encode_first_stage(t["img"].cpu())


def test_wrapper_at_strength_one_is_the_unwrapped_loop(rig, gold):
    """Wrapper(disc, 1.0) == disc on the GPU loop: same inputs, torch.equal with the unwrapped run."""
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper
    eng, t = rig
    x = t["z_init"]
    plain = eng.sampler(eng.native_denoiser(), x, cond=t["c"], uc=t["uc"])
    base = eng.sampler.discretization
    eng.sampler.discretization = Img2ImgDiscretizationWrapper(base, 1.0)
    try:
        wrapped = eng.sampler(eng.native_denoiser(), x, cond=t["c"], uc=t["uc"])
    finally:
        eng.sampler.discretization = base
    assert torch.equal(plain, wrapped)
    # zero steps: the one-entry table [0] hands the start back unchanged
    zero = _sampler(eng, 0.0)(eng.native_denoiser(), x, cond=t["c"], uc=t["uc"])
    assert torch.equal(zero, x)


def test_unclip_sample_defaults_change_nothing(rig, gold):
    """unclip_sample(init=None, strength=1.0) == the call that omits both: no existing behaviour changes."""
    from neurons_amd.sgm import unclip_sample
    eng, t = rig
    args = (eng, t["ctx"][:1], t["vec"][:1], t["z_init"], t["noise"], t["uc_ctx"][:1], eng.sampler)
    a = unclip_sample(*args, offset_noise=t["offset"], offset_noise_level=0.04)
    b = unclip_sample(*args, offset_noise=t["offset"], offset_noise_level=0.04, init=None, strength=1.0)
    assert torch.equal(a, b)


def test_unclip_sample_with_init_is_do_img2img(rig, gold):
    """unclip_sample(init=, strength=): the latents of do_img2img at the same strength, bit for bit, for a latent init and for an image init; the
    sampler's discretization is put back."""
    from neurons_amd.sgm import unclip_sample
    eng, t = rig
    level = float(gold["offset_noise_level"])
    c1 = {"crossattn": t["ctx"][:1].repeat(2, 1, 1), "vector": t["vec"][:1].repeat(2, 1)}
    u1 = {"crossattn": t["uc_ctx"][:1].repeat(2, 1, 1), "vector": t["vec"][:1].repeat(2, 1)}
    base = eng.sampler.discretization
    for init, enc_noise in ((t["z_init"], None), (t["img"], t["enc_noise"])):
        from neurons_amd.sgm import do_img2img
        skip = init is t["z_init"]
        _, want = do_img2img(init, eng, _sampler(eng, 0.5), c1, u1, t["noise"], offset_noise_level=level, offset=t["offset"], skip_encode=skip,
                             return_latents=True, enc_noise=enc_noise)
        got = unclip_sample(eng, t["ctx"][:1], t["vec"][:1], None, t["noise"], t["uc_ctx"][:1], eng.sampler, offset_noise=t["offset"],
                            offset_noise_level=level, init=init, strength=0.5, enc_noise=enc_noise)
        assert torch.equal(got, want)
        assert eng.sampler.discretization is base


def test_runs_are_bit_identical_graph_on_and_off_and_never_replan(rig, gold, monkeypatch):
    """Two runs are bit-identical; captured-graph replay and eager launches are bit-identical; a second call at another strength on the same handle
    plans nothing (the pruned table is a suffix of the full one: same shapes, and per step the same c_in the full schedule's graph slots hold)."""
    eng, t = rig
    net = eng.model.diffusion_model
    img1, z1 = _run(eng, t, gold, False, 1.0)
    plans = _count_calls(monkeypatch, "nr_net_plan")
    key = net._plan_key
    img2, z2 = _run(eng, t, gold, False, 1.0)
    assert torch.equal(z1, z2) and torch.equal(img1, img2)
    _, zh = _run(eng, t, gold, False, 0.5)
    _, zs = _run(eng, t, gold, True, 0.5)
    assert plans[0] == 0 and net._plan_key == key
    net.enable_graph(False)
    try:
        _, z_eager = _run(eng, t, gold, False, 1.0)
        _, zh_eager = _run(eng, t, gold, False, 0.5)
    finally:
        net.enable_graph(True)
    assert torch.equal(z_eager, z1) and torch.equal(zh_eager, zh)
    _, zh2 = _run(eng, t, gold, False, 0.5)
    assert torch.equal(zh2, zh) and plans[0] == 0
