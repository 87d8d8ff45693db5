"""CPU: the host side of the sgm DPM-Solver++ 2M sampler.  ``dpmpp2m_coefficients`` against an fp64 restatement and against the rows the reference's
own ``DPMPP2MSampler.get_variables`` / ``get_mult`` produced in fp32 (tests/golden/sgm_dpmpp2m_tiny.npz, tools/gen_golden_sgm_dpmpp2m.py); the
generic loop on the Gaussian toy model against the reference's recorded finals; the surface (engine option, ctypes stub, argument checks)."""
import math
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sgm_dpmpp2m_tiny.npz")
TABLES = (1, 2, 10, 19, 38)
U = 2.0 ** -24          # fp32 unit roundoff


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _rows(sig):
    """(sigma_prev | None, sigma, sigma_next) per step of a table, as Python floats of the fp32 entries."""
    s = [float(v) for v in sig]
    return [(None if i == 0 else s[i - 1], s[i], s[i + 1]) for i in range(len(s) - 1)]


@pytest.mark.parametrize("n", TABLES)
def test_tables_are_the_reference_tables(gold, n):
    from neurons_amd.sgm import LegacyDDPMDiscretization
    assert torch.equal(LegacyDDPMDiscretization()(n), torch.from_numpy(gold[f"sig_{n}"]))


@pytest.mark.parametrize("n", TABLES)
def test_coefficients_match_fp64_restatement(gold, n):
    """x' = (s'/s) x - expm1(-h) [(1 + 1/(2r)) den - 1/(2r) old], t = -log s, h = t' - t, r = (t - t_prev) / h, written out here in numpy fp64."""
    from neurons_amd.sgm import dpmpp2m_coefficients
    for prev, s, nxt in _rows(gold[f"sig_{n}"]):
        got = dpmpp2m_coefficients(prev, s, nxt)
        if nxt == 0.0:
            assert got == (0.0, 1.0, None)
            continue
        t, t_next = -np.log(np.float64(s)), -np.log(np.float64(nxt))
        h = t_next - t
        want = [np.float64(nxt) / np.float64(s), -np.expm1(-h), None]
        if prev is not None:
            r = (t + np.log(np.float64(prev))) / h
            want = [want[0], -np.expm1(-h) * (1 + 1 / (2 * r)), np.expm1(-h) / (2 * r)]
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if w is not None:
                assert abs(g - w) <= 1e-12 * abs(w), (n, s, g, w)


def test_coefficients_match_the_reference_fp32_rows(gold):
    """The reference forms t = -log sigma in fp32.  With |log sigma| < 4 on these tables (sigma in [0.029, 14.7]) one fp32 ``log`` is off by at most
    1 ulp of a value in [2, 4): e_t = 2^-22 = 2.4e-7, so h = t' - t and h_last carry 2 e_t + U h each, and relative to the fp64 value
        mult1 = exp(-t') / exp(-t)    2 e_t + 5 U            (two exps at 2 U, the quotient)
        mult2 = expm1(-h)             (2 e_t + U h) / h + 2 U     (|d expm1(-h)/dh| h / |expm1(-h)| <= 1)
        1/(2r) = h / (2 h_last)       (2 e_t + U h) / h + (2 e_t + U h_last) / h_last + 2 U      (mult4; mult3 = 1 + mult4 adds U)
    The products c_d = -mult2 mult3 and c_o = mult2 mult4 get the sum of their factors' bounds.  Derived worst bound over the five tables:
    1.73e-5 relative (c_d on the 38-step table, whose smallest h is 0.085); observed worst ratio error / bound: 0.34."""
    from neurons_amd.sgm import dpmpp2m_coefficients
    e_t = 2.0 ** -22
    worst_bound, worst_ratio = 0.0, 0.0
    for n in TABLES:
        sig, mult = gold[f"sig_{n}"], gold[f"mult_{n}"].astype(np.float64)
        assert np.abs(np.log(sig[:-1].astype(np.float64))).max() < 4.0
        for i, (prev, s, nxt) in enumerate(_rows(sig)):
            c_x, c_d, c_o = dpmpp2m_coefficients(prev, s, nxt)
            m1, m2, m3, m4 = mult[i]
            if nxt == 0.0:                                  # h = +inf in fp32 as well: exp(-inf) / exp(-t) = 0, expm1(-inf) = -1
                assert (m1, m2) == (0.0, -1.0) and (c_x, c_d, c_o) == (0.0, 1.0, None)
                continue
            h = math.log(s) - math.log(nxt)
            b1 = 2 * e_t + 5 * U
            b2 = (2 * e_t + U * h) / h + 2 * U
            checks = [("c_x", c_x, m1, b1)]
            if prev is None or i == n - 1:
                assert c_o is None
                checks.append(("c_d", c_d, -m2, b2))
                if prev is None:
                    assert np.isnan(m3) and np.isnan(m4)
            else:
                h_last = math.log(prev) - math.log(s)
                b4 = (2 * e_t + U * h) / h + (2 * e_t + U * h_last) / h_last + 2 * U
                checks += [("c_d", c_d, -m2 * m3, b2 + b4 + U), ("c_o", c_o, m2 * m4, b2 + b4)]
            for name, got, ref, bound in checks:
                ratio = abs(got - ref) / (bound * abs(got))
                worst_bound, worst_ratio = max(worst_bound, bound), max(worst_ratio, ratio)
                assert ratio <= 1.0, (n, i, name, got, ref, bound)
    print(f"[dpmpp2m coefficients vs the reference's fp32 rows] worst derived bound {worst_bound:.2e}, worst error / bound {worst_ratio:.3f}")


@pytest.mark.parametrize("n", TABLES)
def test_first_step_has_no_history_and_last_step_returns_denoised(gold, n):
    from neurons_amd.sgm import dpmpp2m_coefficients
    rows = _rows(gold[f"sig_{n}"])
    assert rows[0][0] is None and dpmpp2m_coefficients(*rows[0])[2] is None
    assert rows[-1][2] == 0.0
    assert dpmpp2m_coefficients(*rows[-1]) == (0.0, 1.0, None)
    assert dpmpp2m_coefficients(None, rows[-1][1], 0.0) == (0.0, 1.0, None)
    for row in rows[1:-1]:
        c_x, c_d, c_o = dpmpp2m_coefficients(*row)
        assert 0.0 < c_x < 1.0 and c_d > 0.0 and c_o is not None and c_o < 0.0


def test_first_order_step_is_the_euler_step():
    """x' = (s'/s) x - expm1(-h) den is algebraically x + (x - den) / s (s' - s): c_x + c_d == 1 and c_d == 1 - s'/s."""
    from neurons_amd.sgm import dpmpp2m_coefficients
    for s, nxt in ((14.6, 9.0), (2.5, 1.8), (0.06, 0.03)):
        c_x, c_d, c_o = dpmpp2m_coefficients(None, s, nxt)
        assert c_o is None and abs(c_x + c_d - 1.0) < 1e-15 and abs(c_d - (1.0 - nxt / s)) < 1e-15


def _gauss(x, sigma, c):
    from neurons_amd.sgm import append_dims
    return x / (1.0 + append_dims(sigma, x.ndim) ** 2)


GAUSS_STEPS = (10, 19, 20, 38)


def gauss_bound(steps, ref):
    """Rounding bound of one fp32 run of either sampler on the Gaussian model against another (the reference's fp32 run, or the kernel's).  The model
    is contractive: an error made at step i reaches the end scaled by 1 / sqrt(1 + sigma_i^2) <= |x_end| / |x_i|.  A step makes at most ~10 roundings
    relative to |x_i| (denoiser 3-4, coefficients and the update 6), so each run ends within 10 U steps |x_end|, two runs within 20 U steps |x_end|;
    taken elementwise against 1 + max |ref|."""
    return 20 * U * steps * (1.0 + float(np.abs(ref).max()))


@pytest.mark.parametrize("n", GAUSS_STEPS)
def test_generic_loop_on_gaussian_model_equals_reference_finals(gold, n):
    from neurons_amd.sgm import DPMPP2MSampler, EulerEDMSampler
    x = torch.from_numpy(gold["gauss.x"])
    c = {"crossattn": torch.zeros(x.shape[0], 1, 4), "vector": torch.zeros(x.shape[0], 4)}
    exact = gold["gauss.exact"]
    for name, cls in (("euler", EulerEDMSampler), ("dpmpp2m", DPMPP2MSampler)):
        rec = []
        got = cls(num_steps=n, scale=5.0)(_gauss, x.clone(), cond=c, uc=c, **({"record": rec} if name == "dpmpp2m" else {}))
        ref = gold[f"gauss.{name}_{n}"]
        err = np.abs(got.numpy().astype(np.float64) - ref).max()
        rel = np.linalg.norm(got.numpy().astype(np.float64) - exact) / np.linalg.norm(exact)
        print(f"[gaussian model, {name} {n} steps] max |got - reference| = {err:.2e} (bound {gauss_bound(n, ref):.2e}), end error {rel:.4f}")
        assert got.dtype == torch.float32 and err <= gauss_bound(n, ref)
        assert abs(rel - float(gold[f"gauss.err_{name}_{n}"])) < 1e-4
        if rec:
            assert len(rec) == n and torch.equal(rec[-1][0], got) and torch.equal(rec[-1][0], rec[-1][1])


def test_fixture_errors_order_as_measured(gold):
    """At unit data variance the reference's 2M at 19 steps ends closer to the exact solution than its Euler at 38, and 2M-10 closer than Euler-20."""
    e = {k: float(gold[f"gauss.err_{k}"]) for k in ("euler_20", "euler_38", "dpmpp2m_10", "dpmpp2m_19")}
    print(e)
    assert e["dpmpp2m_19"] <= e["euler_38"] and e["dpmpp2m_10"] <= e["euler_20"]


def test_generic_loop_calls_the_denoiser_once_per_step_on_a_pruned_table():
    from neurons_amd.sgm import DPMPP2MSampler, Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    x = torch.arange(8, dtype=torch.float32).reshape(1, 2, 2, 2)
    c = {"crossattn": torch.zeros(1, 1, 4), "vector": torch.zeros(1, 4)}
    for strength in (1.0, 0.5, 0.02):
        seen = []

        def denoiser(xx, sigma, cc):
            seen.append(float(sigma[0]))
            return xx * 0.5

        s = DPMPP2MSampler(num_steps=10, discretization=Img2ImgDiscretizationWrapper(disc, strength))
        assert len(s.denoiser.sigmas) == 1000
        out = s(denoiser, x, cond=c, uc=c)
        pruned = Img2ImgDiscretizationWrapper(disc, strength)(10)
        assert seen == [float(v) for v in pruned[:-1]]
        if len(pruned) == 1:
            assert torch.equal(out, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------------------
def _tiny_engine(**kw):
    from neurons_amd.sgm import NativeDiffusionEngine
    from tiny_configs import tiny_sgm_config, tiny_vae_config
    return NativeDiffusionEngine(network_config=tiny_sgm_config(), first_stage_config=tiny_vae_config(), num_steps=4, **kw)


def test_engine_sampler_option():
    from neurons_amd.sgm import DPMPP2MSampler, EulerEDMSampler
    eng = _tiny_engine()
    assert type(eng.sampler) is EulerEDMSampler and eng.sampler.num_steps == 4 and eng.sampler.scale == 5.0
    assert type(_tiny_engine(sampler="euler_edm").sampler) is EulerEDMSampler
    eng = _tiny_engine(sampler="dpmpp_2m", scale=3.0, sampler_config={"target": "anything"})
    assert type(eng.sampler) is DPMPP2MSampler and eng.sampler._engine is eng and eng.sampler.num_steps == 4 and eng.sampler.scale == 3.0
    assert eng.sampler.discretization is eng.denoiser.discretization
    for bad in ("heun", "dpmpp2m", "", None, "EULER_EDM"):
        with pytest.raises(ValueError, match="sampler"):
            _tiny_engine(sampler=bad)


def test_sampler_surface_matches_euler():
    from neurons_amd.sgm import DPMPP2MSampler, EulerEDMSampler, LegacyDDPMDiscretization
    disc = LegacyDDPMDiscretization()
    a, b = EulerEDMSampler(num_steps=7, scale=2.0, discretization=disc), DPMPP2MSampler(num_steps=7, scale=2.0, discretization=disc)
    for name in ("num_steps", "discretization", "guider", "scale", "denoiser", "prepare_sampling_loop", "_engine", "verbose", "device"):
        assert hasattr(b, name), name
    assert b.num_steps == 7 and b.discretization is disc and b.scale == 2.0 and b._engine is None
    b.scale = 4.0
    assert b.guider.scale == 4.0
    x = torch.ones(1, 2, 2, 2)
    for s in (a, b):
        xs, s_in, sigmas, num_sigmas, cond, uc = s.prepare_sampling_loop(x, {"k": 1})
        assert num_sigmas == 8 and uc is cond and torch.equal(xs, x * torch.sqrt(1.0 + sigmas[0] ** 2.0))
    assert not isinstance(b, EulerEDMSampler) and not isinstance(a, DPMPP2MSampler)
    # one recognition for both classes
    assert DPMPP2MSampler._native_network is EulerEDMSampler._native_network


def test_assigned_sampler_recognises_the_engine_closure_and_refuses_cpu_tensors():
    from neurons_amd.sgm import DPMPP2MSampler
    eng = _tiny_engine()
    eng.sampler = DPMPP2MSampler(num_steps=4, scale=5.0)
    assert eng.sampler._engine is None
    diffusion_engine = eng

    def denoiser(x, sigma, c):
        return diffusion_engine.denoiser(diffusion_engine.model, x, sigma, c)

    assert eng.sampler._native_network(denoiser) is eng.model.diffusion_model
    assert eng.sampler._native_network(eng.native_denoiser()) is eng.model.diffusion_model
    assert eng.sampler._native_network(lambda x, sigma, c: x) is None
    z = torch.zeros(1, 4, 8, 8)
    c = {"crossattn": torch.zeros(1, 2, 128), "vector": torch.zeros(1, 64)}
    with pytest.raises(RuntimeError, match="DPMPP2MSampler runs the HIP kernels.*no CPU fallback"):
        eng.sampler(denoiser, z, cond=c, uc=c)


def test_unclip_sample_restores_the_table_of_either_sampler():
    from neurons_amd.sgm import DPMPP2MSampler, do_img2img, unclip_sample
    eng = _tiny_engine(sampler="dpmpp_2m")
    z = torch.zeros(1, 4, 8, 8)
    c = {"crossattn": torch.zeros(1, 2, 128), "vector": torch.zeros(1, 64)}
    for sampler in (eng.sampler, DPMPP2MSampler(num_steps=10)):
        full = sampler.discretization
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            unclip_sample(eng, c["crossattn"], c["vector"], None, z, c["crossattn"], sampler, init=z, strength=0.5)
        assert sampler.discretization is full and type(full).__name__ == "LegacyDDPMDiscretization"
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            do_img2img(z, eng, sampler, c, c, z, skip_encode=True)


def test_ctypes_stub_has_the_header_arity():
    import ctypes as C
    from neurons_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "neurons_amd.h")).read()
    m = re.search(r"nr_status\s+nr_edm_cfg_dpmpp2m_step\s*\(([^)]*)\)\s*;", header)
    assert m, "include/neurons_amd.h does not declare nr_edm_cfg_dpmpp2m_step"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SYMBOLS["nr_edm_cfg_dpmpp2m_step"]
    assert res is C.c_int32 and len(args) == len(params) == 12
    for p, a in zip(params, args):
        want = C.c_void_p if ("*" in p or p.startswith("nr_stream")) else C.c_int64 if p.startswith("int64_t") else C.c_float
        assert a is want, (p, a)
    assert hasattr(_lib.load(), "nr_edm_cfg_dpmpp2m_step")


def refusals(p, q, r):
    """(arguments after the stream, expected status) of every refused call of nr_edm_cfg_dpmpp2m_step; p, q, r: three disjoint device (or host: a
    refused call dereferences nothing) buffers of >= 64 floats, r of >= 128."""
    inf, nan = float("inf"), float("nan")
    ok = dict(net=r, x=p, old=q, x_out=p, den=q, n=64, scale=5.0, sq=2.4, prev=3.4, s=2.5, nxt=1.8)

    def call(status=1, **kw):
        a = dict(ok, **kw)
        return (a["net"], a["x"], a["old"], a["x_out"], a["den"], a["n"], a["scale"], a["sq"], a["prev"], a["s"], a["nxt"]), status

    return [call(net=None), call(x=None), call(x_out=None), call(den=None),                   # null tensors
            call(n=0), call(n=-4), call(status=5, n=2 ** 40),                                 # n <= 0; a grid that does not fit (NR_ERR_UNSUPPORTED)
            call(s=0.0), call(s=-1.0),                                                        # sigma <= 0
            call(nxt=-0.5),                                                                   # sigma_next < 0
            call(nxt=2.5), call(nxt=3.0),                                                     # sigma_next >= sigma
            call(prev=2.5), call(prev=1.0), call(prev=0.0),                                   # sigma_prev <= sigma with history
            call(scale=nan), call(scale=inf), call(sq=nan), call(sq=-inf), call(s=nan), call(s=inf), call(nxt=nan), call(prev=nan),
            call(prev=inf)]                                                                   # non-finite scalars


def test_entry_refuses_bad_arguments_before_any_launch():
    """NR_ERR_ARG (1) / NR_ERR_UNSUPPORTED (5) with a message, decided on the host before any launch, so this needs no device."""
    import ctypes as C
    from neurons_amd import _lib
    lib = _lib.load()
    bufs = [(C.c_float * 128)() for _ in range(3)]
    p, q, r = (C.cast(b, C.c_void_p).value for b in bufs)
    for args, status in refusals(p, q, r):
        st = lib.nr_edm_cfg_dpmpp2m_step(None, *args)
        assert st == status, (st, status, args)
        assert lib.nr_last_error()
