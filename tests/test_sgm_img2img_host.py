"""CPU: the host side of sgm img2img.  ``Img2ImgDiscretizationWrapper`` against the sigma tables the reference's own wrapper produced
(tests/golden/sgm_img2img_tiny.npz, tools/gen_golden_sgm_img2img.py), the sampler's handling of a wrapped discretization on the generic loop,
and the argument checks that need no device."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sgm_img2img_tiny.npz")
STRENGTHS = (0.0, 0.02, 0.5, 0.75, 0.99, 1.0)
STEPS = (1, 10, 38, 50)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("strength", STRENGTHS)
def test_pruned_table_equals_the_reference_wrapper(gold, steps, strength):
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    got = Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), strength)(steps)
    want = torch.from_numpy(gold[f"sig_{steps}_{strength}"])
    assert got.dtype == torch.float32 and torch.equal(got, want), (got, want)
    # helpers.py:91-94: the last max(int(strength * len), 1) entries of the full table, appended zero included
    full = LegacyDDPMDiscretization()(steps)
    assert len(full) == steps + 1
    keep = max(int(strength * (steps + 1)), 1)
    assert len(got) == keep and torch.equal(got, full[len(full) - keep:]) and float(got[-1]) == 0.0


def test_floor_of_one_entry_and_the_one_entry_table(gold):
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    for steps, strength in ((1, 0.0), (1, 0.02), (1, 0.99), (10, 0.0), (10, 0.02), (38, 0.02), (50, 0.0)):     # int(strength * len) == 0
        t = Img2ImgDiscretizationWrapper(disc, strength)(steps)
        assert t.tolist() == [0.0], (steps, strength, t)
    assert len(Img2ImgDiscretizationWrapper(disc, 0.02)(50)) == 1 and len(Img2ImgDiscretizationWrapper(disc, 0.5)(1)) == 1
    assert len(Img2ImgDiscretizationWrapper(disc, 0.99)(50)) == 50


@pytest.mark.parametrize("strength", (-0.01, 1.01, -1.0, 2.0, float("nan")))
def test_strength_outside_unit_interval_asserts(strength):
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    with pytest.raises(AssertionError):
        Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), strength)


def test_wrapper_around_a_wrapper(gold):
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper as W, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    got = W(W(disc, 0.75), 0.5)(50)
    assert torch.equal(got, torch.from_numpy(gold["sigw_50"]))
    assert len(got) == int(0.5 * int(0.75 * 51)) and torch.equal(got, disc(50)[51 - len(got):])
    # keyword arguments travel to the wrapped discretization; the pruning applies to whatever comes back (no appended zero here)
    t = W(disc, 0.5)(10, do_append_zero=False)
    assert len(t) == 5 and torch.equal(t, disc(10, do_append_zero=False)[5:])


def test_strength_one_returns_the_wrapped_table():
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization

    class Fixed:
        def __init__(self):
            self.table = torch.tensor([3.0, 2.0, 1.0, 0.0])

        def __call__(self, n):
            return self.table

    f = Fixed()
    assert Img2ImgDiscretizationWrapper(f, 1.0)(4) is f.table
    for steps in STEPS:
        assert torch.equal(Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), 1.0)(steps), LegacyDDPMDiscretization()(steps))


def test_wrapper_prints_nothing(capsys):
    from neurons_amd.sgm import Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), 0.5)(10)
    cap = capsys.readouterr()
    assert cap.out == "" and cap.err == ""


def _toy_denoiser(seen):
    def denoiser(x, sigma, c):
        seen.append(float(sigma[0]))
        return x * 0.5
    return denoiser


def test_generic_loop_runs_the_pruned_table():
    """EulerEDMSampler accepts the wrapper as its discretization: a foreign denoiser (generic loop, CPU tensors) is evaluated exactly at the pruned
    table's non-final entries, and the host scalars of the fused path keep the full 1000-entry table."""
    from neurons_amd.sgm import EulerEDMSampler, Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    full = disc(10)
    x = torch.arange(8, dtype=torch.float32).reshape(1, 2, 2, 2)
    c = {"crossattn": torch.zeros(1, 1, 4), "vector": torch.zeros(1, 4)}
    for strength in (1.0, 0.5, 0.02):
        s = EulerEDMSampler(num_steps=10, discretization=Img2ImgDiscretizationWrapper(disc, strength))
        assert len(s.denoiser.sigmas) == 1000
        seen = []
        out = s(_toy_denoiser(seen), x, cond=c, uc=c)
        pruned = Img2ImgDiscretizationWrapper(disc, strength)(10)
        assert seen == [float(v) for v in pruned[:-1]] and len(seen) == len(pruned) - 1
        assert seen == [float(v) for v in full[len(full) - len(pruned):-1]]
        if len(pruned) == 1:                                  # the one-entry table [0]: zero steps, the start comes back unchanged
            assert torch.equal(out, x)
    # the reference's idiom: swap the discretization of an existing sampler
    s = EulerEDMSampler(num_steps=10, discretization=disc)
    seen_full, seen = [], []
    s(_toy_denoiser(seen_full), x, cond=c, uc=c)
    s.discretization = Img2ImgDiscretizationWrapper(s.discretization, 0.5)
    s(_toy_denoiser(seen), x, cond=c, uc=c)
    assert len(seen_full) == 10 and seen == seen_full[-4:]


def test_generic_loop_at_strength_one_is_bit_identical():
    from neurons_amd.sgm import EulerEDMSampler, Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    x = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(1))
    c = {"crossattn": torch.zeros(2, 1, 4), "vector": torch.zeros(2, 4)}
    a = EulerEDMSampler(num_steps=7, discretization=disc)(_toy_denoiser([]), x, cond=c, uc=c)
    b = EulerEDMSampler(num_steps=7, discretization=Img2ImgDiscretizationWrapper(disc, 1.0))(_toy_denoiser([]), x, cond=c, uc=c)
    assert torch.equal(a, b)


def test_cpu_tensors_raise_no_fallback():
    from neurons_amd.sgm import NativeDiffusionEngine, do_img2img, edm_img2img_start, unclip_sample
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edm_img2img_start(z, 1.0, z=z)
    with pytest.raises(ValueError):
        edm_img2img_start(z, 1.0)                              # neither a latent nor moments
    with pytest.raises(ValueError):
        edm_img2img_start(z, 1.0, z=z, moments=torch.zeros(1, 8, 8, 8))
    eng = NativeDiffusionEngine(network_config=tiny_sgm_config(), first_stage_config=tiny_vae_config(), num_steps=4)
    c = {"crossattn": torch.zeros(1, 2, 128), "vector": torch.zeros(1, 64)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        do_img2img(z, eng, eng.sampler, c, c, z, skip_encode=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unclip_sample(eng, c["crossattn"], c["vector"], None, z, c["crossattn"], eng.sampler, init=z, strength=0.5)
    assert not isinstance(eng.sampler.discretization, type(None)) and type(eng.sampler.discretization).__name__ == "LegacyDDPMDiscretization"
    # an engine whose checkpoint held no encoder cannot encode: an error, not a fallback
    with pytest.raises(RuntimeError, match="encoder"):
        eng.encode_first_stage(torch.zeros(1, 3, 64, 64))


def test_start_entry_refuses_bad_arguments_before_any_launch():
    """nr_edm_img2img_start: NR_ERR_ARG (1) with a message, checked on the host before any launch, so this needs no device.  The pointers are never
    dereferenced on these paths (a refused call launches nothing)."""
    import ctypes as C
    from neurons_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    L, M = _lib.NR_IMG2IMG_LATENT, _lib.NR_IMG2IMG_MOMENTS
    inf, nan = float("inf"), float("nan")
    #        z_in  mom   eps   noise off   out   batch nps  zs   sigma0 level mode
    bad = [(None, None, None, p, None, p, 1, 16, 1.0, 1.0, 0.0, L),        # mode 0 without z_in
           (p, None, None, None, None, p, 1, 16, 1.0, 1.0, 0.0, L),        # no noise
           (p, None, None, p, None, None, 1, 16, 1.0, 1.0, 0.0, L),        # no out
           (p, None, p, p, None, p, 1, 16, 1.0, 1.0, 0.0, M),              # mode 1 without moments
           (p, p, None, p, None, p, 1, 16, 1.0, 1.0, 0.0, M),              # mode 1 without the encoder draw
           (p, None, None, p, None, p, 1, 0, 1.0, 1.0, 0.0, L),            # n_per_sample <= 0
           (p, None, None, p, None, p, 1, -4, 1.0, 1.0, 0.0, L),
           (p, None, None, p, None, p, 0, 16, 1.0, 1.0, 0.0, L),           # batch <= 0
           (p, None, None, p, None, p, 1, 16, 1.0, -0.5, 0.0, L),          # sigma0 < 0
           (p, None, None, p, None, p, 1, 16, 1.0, inf, 0.0, L),           # non-finite sigma0
           (p, None, None, p, None, p, 1, 16, 1.0, nan, 0.0, L),
           (p, None, None, p, None, p, 1, 16, 1.0, 1.0, 0.0, 2),           # unknown mode
           (p, None, None, p, None, p, 2 ** 40, 2 ** 40, 1.0, 1.0, 0.0, L)]  # batch * n_per_sample overflows
    for args in bad:
        st = lib.nr_edm_img2img_start(None, *args)
        assert st == 1, (st, args)
        assert lib.nr_last_error()


def test_engine_state_dict_routes_the_encoder_half():
    """first_stage_model.encoder.* / quant_conv.* now reach the engine's encoder; a checkpoint without them still loads strictly (as before), one
    that holds only part of them reports the rest missing."""
    from neurons_amd.sgm import NativeDiffusionEngine, sgm_random_state_dict
    from neurons_amd.vae import vae_random_state_dict
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    cfg, vcfg = tiny_sgm_config(), tiny_vae_config()
    ck = {"model.diffusion_model." + k: v for k, v in sgm_random_state_dict(cfg, seed=71).items()}
    ck.update({"first_stage_model." + k: v for k, v in vae_random_state_dict(vcfg, seed=91).items()})
    eng = NativeDiffusionEngine(network_config=cfg, first_stage_config=vcfg)
    assert eng.load_state_dict(ck) == ([], [])
    assert not eng.first_stage_encoder._loaded
    enc = {"first_stage_model." + k: v for k, v in vae_random_state_dict(vcfg, seed=94, encoder=True).items()}
    eng = NativeDiffusionEngine(network_config=cfg, first_stage_config=vcfg)
    assert eng.load_state_dict({**ck, **enc}) == ([], [])
    assert set(eng.first_stage_encoder._loaded) == {k[len("first_stage_model."):] for k in enc}
    part = dict(list(enc.items())[:3])
    eng = NativeDiffusionEngine(network_config=cfg, first_stage_config=vcfg)
    with pytest.raises(RuntimeError, match="Missing key"):
        eng.load_state_dict({**ck, **part})
