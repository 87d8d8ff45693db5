"""Host logic of the full DDIM step contract (no GPU): the cosine beta schedule, the sigma / direction-coefficient helper, what the
constructor accepts, and the argument errors of ``step``.  Every expected value is restated here in double from the published
formulas (Song et al. 2021 eq. 16; Nichol & Dhariwal 2021 eq. 17); nothing of neurons_amd is used but what is compared."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from neurons_amd.scheduler import DDIMScheduler  # noqa: E402


def _cosine_beta(i, T):
    def alpha_bar(s):
        return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
    return min(1.0 - alpha_bar((i + 1) / T) / alpha_bar(i / T), 0.999)


@pytest.mark.parametrize("T", [10, 1000])
def test_cosine_schedule_matches_closed_form(T):
    s = DDIMScheduler(num_train_timesteps=T, beta_schedule="squaredcos_cap_v2", clip_sample=False)
    assert s.betas.shape == (T,)
    for i in (0, T // 2, T - 1):
        assert abs(float(s.betas[i]) - _cosine_beta(i, T)) <= 1e-6, (T, i)
    assert float(s.betas[T - 1]) == pytest.approx(0.999, abs=1e-6)       # the cap: alpha_bar(1) = 0 would give beta = 1
    assert torch.allclose(s.alphas_cumprod, torch.cumprod(1.0 - s.betas, 0))


def _sched(**kw):
    return DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False, **kw)


def test_sigma_and_direction_helper():
    s = _sched()
    s.set_timesteps(10)
    for t in s.timesteps_host:
        a_t, a_prev, sigma, dirc = s.step_coefficients(t, 0.0)
        assert (a_t, a_prev) == s.alpha_pair(t)
        assert sigma == 0.0 and dirc == math.sqrt(1.0 - a_prev)          # exactly: the default path's coefficient
    for t in s.timesteps_host:
        a_t, a_prev, sigma, dirc = s.step_coefficients(t, 1.0)
        want = math.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))
        assert abs(sigma - want) <= 1e-15
        assert abs(sigma * sigma + dirc * dirc - (1.0 - a_prev)) <= 1e-12
        assert all(isinstance(v, float) for v in (a_t, a_prev, sigma, dirc))
    a_t, a_prev, sigma, dirc = s.step_coefficients(s.timesteps_host[-1], 1.0)     # last step: a_prev = 1
    assert a_prev == 1.0 and sigma == 0.0 and dirc == 0.0
    assert all(math.isfinite(v) for v in s.step_coefficients(s.timesteps_host[-1], 0.7))
    a_t, a_prev, sigma, dirc = s.step_coefficients(s.timesteps_host[3], 0.5)
    assert abs(sigma - 0.5 * math.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))) <= 1e-15


def test_constructor_accepts_the_published_prediction_types():
    for p in ("epsilon", "sample", "v_prediction"):
        assert _sched(prediction_type=p).config.prediction_type == p
    with pytest.raises(ValueError):
        _sched(prediction_type="foo")
    d = DDIMScheduler()                                                    # diffusers' defaults: clip_sample=True
    assert d.config.clip_sample is True and d.config.prediction_type == "epsilon" and d.config.beta_schedule == "linear"
    d.set_timesteps(10)
    # the only refusal left in step() for this object is the device check: clip_sample=True is served
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.step(torch.zeros(1, 4), d.timesteps_host[0], torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.step(torch.zeros(1, 4), d.timesteps_host[0], torch.zeros(1, 4), eta=0.5, use_clipped_model_output=True)
    assert not d.is_default_rule and _sched().is_default_rule


def test_generator_and_variance_noise_together_are_refused():
    s = _sched()
    s.set_timesteps(10)
    x = torch.zeros(1, 4)
    with pytest.raises(ValueError, match="Cannot pass both generator and variance_noise"):
        s.step(x, s.timesteps_host[0], x, eta=0.5, generator=torch.Generator().manual_seed(0), variance_noise=torch.zeros(1, 4))
