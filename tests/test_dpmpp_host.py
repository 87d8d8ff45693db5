"""CPU: the host side of DPMSolverMultistepScheduler (tables, order selection, the coefficients of nr_cfg_dpmpp_step, refused options).

The reference of every numeric check is the restatement below: DPM-Solver++ (Lu et al. 2022, the multistep 2M solver, in the D0 / D1 form
diffusers 0.11.1 ships) in fp64.  It uses nothing of neurons_amd; tests/test_dpmpp_gpu.py imports it for the device checks."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BETAS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear")      # configs/inference/inference-v3.yaml of the reference
SOLVERS = ("midpoint", "heun")


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------------------
def ref_tables(beta_start=0.00085, beta_end=0.012, T=1000):
    """(alphas_cumprod, alpha_t, sigma_t, lambda_t) as lists of doubles from the table as diffusers builds it: fp32 linspace, fp32 cumprod."""
    ac = [float(v) for v in torch.cumprod(1.0 - torch.linspace(beta_start, beta_end, T, dtype=torch.float32), 0)]
    alpha, sigma = [math.sqrt(a) for a in ac], [math.sqrt(1.0 - a) for a in ac]
    return ac, alpha, sigma, [math.log(a / s) for a, s in zip(alpha, sigma)]


def ref_timesteps(n, T=1000):
    return [int(v) for v in np.linspace(0, T - 1, n + 1).round()[::-1][:-1]]


def ref_orders(n, solver_order=2, lower_order_final=True):
    """The order of every step of an n-step walk from step 0."""
    out = []
    for i in range(n):
        first = solver_order == 1 or i == 0 or (i == n - 1 and lower_order_final and n < 15)
        out.append(1 if first else 2)
    return out


def ref_m0(model_output, x, alpha_s, sigma_s, prediction_type, guidance=None):
    """The data prediction.  ``model_output`` holds the unconditional half first when ``guidance`` is given.  Tensors (fp64) or floats."""
    m = model_output
    if guidance is not None:
        mu, mc = m.chunk(2)
        m = mu + guidance * (mc - mu)
    if prediction_type == "epsilon":
        return (x - sigma_s * m) / alpha_s
    if prediction_type == "sample":
        return m
    return alpha_s * x - sigma_s * m


def ref_update(x, m0, m1, tabs, t, s0, s1, order, solver_type):
    """One multistep update from timestep s0 to t (s1: the timestep before s0), written with exp as the paper and diffusers write it."""
    _, alpha, sigma, lam = tabs
    h = lam[t] - lam[s0]
    if order == 1:
        return (sigma[t] / sigma[s0]) * x - (alpha[t] * (math.exp(-h) - 1.0)) * m0
    r0 = (lam[s0] - lam[s1]) / h
    d0, d1 = m0, (1.0 / r0) * (m0 - m1)
    if solver_type == "midpoint":
        return (sigma[t] / sigma[s0]) * x - (alpha[t] * (math.exp(-h) - 1.0)) * d0 - 0.5 * (alpha[t] * (math.exp(-h) - 1.0)) * d1
    return (sigma[t] / sigma[s0]) * x - (alpha[t] * (math.exp(-h) - 1.0)) * d0 + (alpha[t] * ((math.exp(-h) - 1.0) / h + 1.0)) * d1


def ref_step(model_output, x, m1, tabs, ts, i, order, solver_type, prediction_type="epsilon", guidance=None):
    """Step i of the walk over ``ts``: (x_out, m0)."""
    _, alpha, sigma, _ = tabs
    s0 = ts[i]
    m0 = ref_m0(model_output, x, alpha[s0], sigma[s0], prediction_type, guidance)
    t = ts[i + 1] if i + 1 < len(ts) else 0
    return ref_update(x, m0, m1, tabs, t, s0, ts[i - 1] if i > 0 else None, order, solver_type), m0


def ref_coefficients(tabs, ts, i, order, solver_type):
    """(c_x, c_m0, c_m1) read off the linear update."""
    t, s0, s1 = (ts[i + 1] if i + 1 < len(ts) else 0), ts[i], (ts[i - 1] if i > 0 else None)
    return tuple(ref_update(*basis, tabs, t, s0, s1, order, solver_type) for basis in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def _sched(**kw):
    from neurons_amd import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**dict(BETAS, **kw))


@pytest.mark.parametrize("n", [4, 10, 20, 25, 50])
def test_timestep_table(n):
    s = _sched()
    s.set_timesteps(n)
    ts = s.timesteps_host
    assert ts == ref_timesteps(n) and ts == [int(v) for v in s.timesteps]
    assert len(ts) == n and ts[0] == 999 and ts[-1] > 0
    assert all(a > b for a, b in zip(ts, ts[1:]))


def test_surface():
    s = _sched()
    assert s.order == 1 and s.init_noise_sigma == 1.0 and not hasattr(s, "alpha_pair") and s.native_rule == "dpmsolver++"
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x
    s.set_timesteps(10)
    ac = ref_tables()[0]
    noisy = s.add_noise(torch.ones(2, 4, 1, 2, 2), torch.full((2, 4, 1, 2, 2), 2.0), s.timesteps[:1].repeat(2))
    assert torch.allclose(noisy, torch.full_like(noisy, math.sqrt(ac[999]) + 2.0 * math.sqrt(1.0 - ac[999])), rtol=1e-6, atol=0)
    with pytest.raises(NotImplementedError, match="nr_cfg_dpmpp_step"):
        s.step(torch.zeros(1, 4), 999, torch.zeros(1, 4))                  # CPU tensors: refused as DDIMScheduler.step refuses them


@pytest.mark.parametrize("n,kw", [(4, {}), (14, {}), (15, {}), (20, {}), (14, dict(lower_order_final=False)), (4, dict(lower_order_final=False)),
                                  (10, dict(solver_order=1)), (20, dict(solver_order=1))])
def test_order_selection_over_a_walk(n, kw):
    s = _sched(**kw)
    s.set_timesteps(n)
    orders = [s.step_coefficients(i).order for i in range(n)]
    assert orders == ref_orders(n, **kw) and orders == [s.step_order(i) for i in range(n)]
    assert orders[0] == 1
    if kw.get("solver_order") == 1:
        assert orders == [1] * n
    else:
        assert orders[1:-1] == [2] * (n - 2)
        assert orders[-1] == (1 if (n < 15 and kw.get("lower_order_final", True)) else 2)
    for i, o in enumerate(orders):
        assert (s.step_coefficients(i).c_m1 != 0.0) == (o == 2)
    # without history a step is first order wherever it lies on the grid
    assert s.step_coefficients(2, history=0).order == 1 and s.step_order(0, history=2) == 1


def test_set_timesteps_resets_the_history():
    s = _sched()
    s.set_timesteps(10)
    s.lower_order_nums = 2                  # as after two calls of step
    assert s.step_coefficients(3, history=s.lower_order_nums).order == 2
    s.set_timesteps(10)
    assert s.lower_order_nums == 0 and s.step_coefficients(3, history=s.lower_order_nums).order == 1
    s.set_timesteps(4)
    assert len(s.timesteps_host) == 4


@pytest.mark.parametrize("solver_type", SOLVERS)
@pytest.mark.parametrize("n", [4, 10, 20, 50])
def test_coefficients_match_the_restatement(n, solver_type):
    tabs = ref_tables()
    s = _sched(solver_type=solver_type)
    s.set_timesteps(n)
    ts = ref_timesteps(n)
    for i, order in enumerate(ref_orders(n)):
        k = s.step_coefficients(i)
        assert k.alpha_s == tabs[1][ts[i]] and k.sigma_s == tabs[2][ts[i]]
        for name, got, ref in zip(("c_x", "c_m0", "c_m1"), (k.c_x, k.c_m0, k.c_m1), ref_coefficients(tabs, ts, i, order, solver_type)):
            assert abs(got - ref) <= 1e-12 * abs(ref), (n, i, name, got, ref)
    # the step after the last timestep goes to timestep 0 (alphas_cumprod[0]), not to alpha = 1
    assert s.step_coefficients(n - 1).c_x == tabs[2][0] / tabs[2][ts[-1]] > 0.0


@pytest.mark.parametrize("n", [10, 25])
def test_first_order_epsilon_step_is_the_ddim_update(n):
    """c_x x + c_m0 (x - sigma_s e) / alpha_s  =  sqrt(a_t) x0 + sqrt(1 - a_t) e: on x the coefficient sqrt(a_t / a_s), on e the DDIM direction
    coefficient minus sqrt(a_t) sigma_s / alpha_s."""
    from neurons_amd.scheduler import ddim_sigma_dir
    ac = ref_tables()[0]
    s = _sched(solver_order=1)
    s.set_timesteps(n)
    ts = s.timesteps_host
    for i in range(n):
        a_s, a_t = ac[ts[i]], ac[ts[i + 1] if i + 1 < n else 0]
        k = s.step_coefficients(i)
        sigma, direction = ddim_sigma_dir(a_s, a_t, 0.0)
        assert sigma == 0.0
        on_x, on_e = k.c_x + k.c_m0 / k.alpha_s, -k.c_m0 * k.sigma_s / k.alpha_s
        ref_x = math.sqrt(a_t) / math.sqrt(a_s)
        ref_e = direction - math.sqrt(a_t) * math.sqrt(1.0 - a_s) / math.sqrt(a_s)
        assert abs(on_x - ref_x) <= 1e-12 * ref_x, (i, on_x, ref_x)
        # the two terms of ref_e cancel in part: the error is that of the terms
        assert abs(on_e - ref_e) <= 1e-12 * (direction + abs(ref_e)), (i, on_e, ref_e)


def _analytic_errors(n, s_data=2.0):
    """Relative end error of a pure-Python walk under the exact noise prediction of N(0, s^2) data, e = sigma x / (alpha^2 s^2 + sigma^2), whose
    probability-flow solution is x sqrt(alpha^2 s^2 + sigma^2) up to the start constant: (DPM-Solver++ 2M midpoint, DDIM), each between its
    own end points."""
    from neurons_amd import DDIMScheduler, DPMSolverMultistepScheduler
    ac = ref_tables()[0]

    def scale(a):
        return math.sqrt(a * s_data * s_data + (1.0 - a))

    def eps(x, a):
        return math.sqrt(1.0 - a) * x / (a * s_data * s_data + (1.0 - a))

    dpm = DPMSolverMultistepScheduler(**BETAS)
    dpm.set_timesteps(n)
    ts = dpm.timesteps_host
    x, m1 = 1.0, 0.0
    for i, t in enumerate(ts):
        k = dpm.step_coefficients(i)
        m0 = (x - k.sigma_s * eps(x, ac[t])) / k.alpha_s
        x, m1 = k.c_x * x + k.c_m0 * m0 + k.c_m1 * m1, m0
    err_dpm = abs(x / (scale(ac[0]) / scale(ac[ts[0]])) - 1.0)

    ddim = DDIMScheduler(steps_offset=1, clip_sample=False, **BETAS)
    ddim.set_timesteps(n)
    ts = ddim.timesteps_host
    x = 1.0
    for t in ts:
        a_t, a_prev, _, direction = ddim.step_coefficients(t, 0.0)
        e = eps(x, a_t)
        x = math.sqrt(a_prev) * (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t) + direction * e
    a_end = ddim.alpha_pair(ts[-1])[1]
    err_ddim = abs(x / (scale(a_end) / scale(ac[ts[0]])) - 1.0)
    return err_dpm, err_ddim


@pytest.mark.parametrize("n", [10, 25, 50])
def test_second_order_beats_ddim_on_an_analytic_model(n):
    err_dpm, err_ddim = _analytic_errors(n)
    print(f"[analytic N={n}] 2M midpoint {err_dpm:.3e}  DDIM {err_ddim:.3e}  ratio {err_dpm / err_ddim:.3f}")
    assert err_dpm <= 0.5 * err_ddim


def test_refused_options():
    for kw in (dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(thresholding=True)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            _sched(**kw)
    for kw in (dict(algorithm_type="foo"), dict(solver_type="bh1"), dict(prediction_type="foo"), dict(solver_order=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            _sched(**kw)
    with pytest.raises(NotImplementedError, match="cosine"):
        _sched(beta_schedule="cosine")
    with pytest.raises(ValueError, match="set_timesteps"):
        _sched().step(torch.zeros(1), 999, torch.zeros(1))


def test_reference_config_keys_construct_the_class():
    """noise_scheduler_kwargs of the reference's configs/inference/inference-v3.yaml go to whichever scheduler class the script constructs."""
    kwargs = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    s = _sched(**kwargs)
    assert s.config.steps_offset == 1 and s.config.clip_sample is False and s.config.solver_order == 2
    assert s.config.algorithm_type == "dpmsolver++" and s.config.solver_type == "midpoint" and s.config.lower_order_final is True
    s.set_timesteps(20)
    assert s.timesteps_host == ref_timesteps(20)          # steps_offset is recorded, not applied


def test_pipeline_group_size_for_20_steps_has_no_tail():
    """The grouped SparseCtrl schedule depends on the timestep list only.  20 steps: sizes 4 and 5 both divide it and cost the same; the rule's
    tie goes to 4, and a forced 5 is taken as is."""
    from neurons_amd.pipeline import controlnet_group_plan, controlnet_group_size
    g = controlnet_group_size(20, 2, 16, 32, 32)
    assert g in (4, 5) and 20 % g == 0
    assert controlnet_group_size(20, 2, 16, 32, 32, 5) == 5
    groups, steps = controlnet_group_plan(ref_timesteps(20), 5)
    assert len(groups) == 4 and [t for grp in groups for t in grp["timesteps"]] == ref_timesteps(20)
