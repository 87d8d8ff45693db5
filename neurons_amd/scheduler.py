"""DDIM and DPM-Solver++ multistep schedulers with the surface the reference pipeline uses.

The reference imports ``DDIMScheduler`` from un-vendored ``diffusers==0.11.1`` (README.md:58;
constructed at scripts/neuroclips_video.py:219 from configs/inference/inference-v3.yaml:16-21; used at
animatediff/pipelines/pipeline_neuroclips.py:317,378-379,423,431,436,483).  That source is not under
/root/reference, so this is a restatement of the published DDIM algorithm (Song et al. 2020, eq. 12, eta
as in diffusers' ``step``) — parity for this class is *unpinned* by any reference test; it is cross-checked
against the in-repo sibling ``animatediff/utils/util.py:211-221`` (``next_step``) in tests/.

Only table construction / coefficient selection happens here (host logic).  The per-element update runs in
the HIP kernels behind ``nr_cfg_ddim_step`` / ``nr_cfg_ddim_step_ex`` (include/neurons_amd.h); ``step`` refuses CPU tensors.
``DPMSolverMultistepScheduler`` (below; ``nr_cfg_dpmpp_step``) is the second of the six classes the reference pipeline is written for
(pipeline_neuroclips.py:20-25,53-58), a second-order rule at one network evaluation per step, commonly run at 20 - 25 steps where DDIM runs 50.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


PREDICTION_TYPES = {"epsilon": 0, "sample": 1, "v_prediction": 2}      # NR_DDIM_* of include/neurons_amd.h


def betas_for_alpha_bar(num_diffusion_timesteps, max_beta=0.999):
    """The cosine schedule ("squaredcos_cap_v2"; Nichol & Dhariwal 2021 eq. 17): alpha_bar(s) = cos((s + 0.008) / 1.008 * pi / 2) ** 2,
    beta_i = min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), max_beta)."""
    def alpha_bar(s):
        return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
    T = num_diffusion_timesteps
    return torch.tensor([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), max_beta) for i in range(T)], dtype=torch.float32)


def make_betas(cls, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas):
    """The fp32 beta table as diffusers builds it, for every scheduler class of this module."""
    if trained_betas is not None:
        return torch.as_tensor(trained_betas, dtype=torch.float32)
    if beta_schedule == "linear":
        # diffusers "linear": linspace in beta (NOT SD's scaled_linear) — SURVEY.md F12
        return torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    if beta_schedule == "squaredcos_cap_v2":
        return betas_for_alpha_bar(num_train_timesteps)
    raise NotImplementedError(f"{beta_schedule} does is not implemented for {cls}")


def ddim_sigma_dir(a_t, a_prev, eta):
    """(sigma, dir_coeff) of one DDIM step in double: sigma = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)) (Song et al. 2021 eq. 16),
    dir_coeff = sqrt(1 - a_prev - sigma^2).  eta = 0 gives (0, sqrt(1 - a_prev)) exactly; the last step (a_prev = 1) gives (0, 0)."""
    if eta == 0.0:
        return 0.0, math.sqrt(1.0 - a_prev)
    variance = (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)
    sigma = float(eta) * math.sqrt(max(variance, 0.0))
    return sigma, math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0))


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon"):
        betas = make_betas(self.__class__, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, clip_sample=clip_sample,
                                      set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset,
                                      prediction_type=prediction_type)
        self._timesteps_host = [int(t) for t in self.timesteps]

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // num_inference_steps
        timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
        timesteps = timesteps + self.config.steps_offset
        self._timesteps_host = [int(t) for t in timesteps]          # no device sync inside the loop
        self.timesteps = torch.from_numpy(timesteps).to(device)

    @property
    def timesteps_host(self):
        return list(self._timesteps_host)

    def alpha_pair(self, timestep):
        """(alpha_prod_t, alpha_prod_t_prev) as python floats for integer ``timestep``."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def step_coefficients(self, timestep, eta=0.0):
        """(alpha_prod_t, alpha_prod_t_prev, sigma, dir_coeff) as python floats for integer ``timestep``: everything the fused CFG + DDIM kernel
        needs from the host, without a device sync (see ``ddim_sigma_dir``)."""
        a_t, a_prev = self.alpha_pair(timestep)
        sigma, dir_coeff = ddim_sigma_dir(a_t, a_prev, eta)
        return a_t, a_prev, sigma, dir_coeff

    @property
    def is_default_rule(self):
        """epsilon prediction without clipping: with eta = 0 the update the pipeline issues as plain ``nr_cfg_ddim_step``."""
        return self.config.prediction_type == "epsilon" and not self.config.clip_sample

    def add_noise(self, original_samples, noise, timesteps):
        ac = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        timesteps = timesteps.to(original_samples.device)
        sqrt_alpha_prod = ac[timesteps] ** 0.5
        sqrt_alpha_prod = sqrt_alpha_prod.flatten()
        while len(sqrt_alpha_prod.shape) < len(original_samples.shape):
            sqrt_alpha_prod = sqrt_alpha_prod.unsqueeze(-1)
        sqrt_one_minus = (1 - ac[timesteps]) ** 0.5
        sqrt_one_minus = sqrt_one_minus.flatten()
        while len(sqrt_one_minus.shape) < len(original_samples.shape):
            sqrt_one_minus = sqrt_one_minus.unsqueeze(-1)
        return sqrt_alpha_prod * original_samples + sqrt_one_minus * noise

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        """diffusers 0.11.1 ``DDIMScheduler.step``: eta, use_clipped_model_output, generator / variance_noise, config.clip_sample and
        config.prediction_type are honoured; ``pred_original_sample`` is returned.  The arithmetic runs in HIP (nr_cfg_ddim_step_ex)."""
        if generator is not None and variance_noise is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        if not (model_output.is_cuda and sample.is_cuda):
            # a RuntimeError by class (callers that catch the library's errors) that also says what it is: not implemented on the CPU
            raise NotImplementedError("DDIMScheduler.step runs in the HIP kernel nr_cfg_ddim_step: CUDA (ROCm) tensors required, "
                                      "there is no CPU fallback")
        from . import ops
        a_t, a_prev = self.alpha_pair(timestep)
        if eta > 0 and variance_noise is None:
            # drawn as diffusers draws it: once per step whenever eta > 0 (the last step, where sigma = 0, included), in the model output's
            # shape and dtype on its device
            variance_noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        noise = variance_noise.to(device=sample.device, dtype=torch.float32).contiguous() if variance_noise is not None else None
        prev, x0 = ops.cfg_ddim_step(model_output.float().contiguous(), sample.float().contiguous(), 1.0, a_t, a_prev, do_cfg=False,
                                     prediction_type=self.config.prediction_type, clip_sample=bool(self.config.clip_sample),
                                     use_clipped_model_output=bool(use_clipped_model_output), eta=eta, noise=noise,
                                     return_pred_original=True)
        prev, x0 = prev.to(sample.dtype), x0.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=x0)


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor


class DPMStepCoefficients(NamedTuple):
    """What one nr_cfg_dpmpp_step launch needs from the host: x_out = c_x x + c_m0 m0 + c_m1 m1, m0 formed from (alpha_s, sigma_s)."""
    alpha_s: float
    sigma_s: float
    c_x: float
    c_m0: float
    c_m1: float
    order: int


class DPMSolverMultistepScheduler:
    """DPM-Solver++ multistep, orders 1 and 2 (Lu et al. 2022, "DPM-Solver++", the 2M solver), with the surface of diffusers 0.11.1
    ``DPMSolverMultistepScheduler``.  Like DDIM above that source is not vendored with the reference: parity is *unpinned*, the paper governs.

    Host logic only: tables in double, order selection, and the coefficients of the linear form every update of order <= 2 has.  The
    per-element work (CFG, the x0 prediction, the update) runs in the HIP kernel behind ``nr_cfg_dpmpp_step``; ``step`` refuses CPU tensors.
    """
    order = 1
    native_rule = "dpmsolver++"         # the pipeline tells the class by this: one nr_cfg_dpmpp_step per step (``alpha_pair`` means DDIM)

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, steps_offset=0, clip_sample=False):
        # steps_offset / clip_sample: keys of the reference's noise_scheduler_kwargs (configs/inference/inference-v3.yaml:16-21), which go to
        # whichever class the script constructs; this rule has no use for them (diffusers keeps unexpected keys in the config the same way)
        betas = make_betas(self.__class__, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        if algorithm_type == "dpmsolver":
            raise NotImplementedError("algorithm_type='dpmsolver' (the noise-space solver) is not built: only 'dpmsolver++'")
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type given as {algorithm_type} must be one of `dpmsolver`, `dpmsolver++`")
        if solver_type not in ("midpoint", "heun"):
            raise ValueError(f"solver_type given as {solver_type} must be one of `midpoint`, `heun`")
        if solver_order == 3:
            raise NotImplementedError("solver_order=3 is not built: only orders 1 and 2 (the multistep 2M solver)")
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order given as {solver_order} must be one of 1, 2, 3")
        if thresholding:
            raise NotImplementedError("thresholding=True (dynamic thresholding: a per-sample quantile, meant for pixel-space models) is not built")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        # the fp32 table read back into host doubles
        ac = [float(v) for v in self.alphas_cumprod]
        self._alpha_t = [math.sqrt(a) for a in ac]
        self._sigma_t = [math.sqrt(1.0 - a) for a in ac]
        self._lambda_t = [math.log(a) - math.log(s) for a, s in zip(self._alpha_t, self._sigma_t)]
        self.init_noise_sigma = 1.0
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, solver_order=solver_order,
                                      prediction_type=prediction_type, thresholding=thresholding,
                                      dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
                                      algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                                      steps_offset=steps_offset, clip_sample=clip_sample)
        self.num_inference_steps = None
        self._timesteps_host = [int(t) for t in np.linspace(0, num_train_timesteps - 1, num_train_timesteps)[::-1]]
        self.timesteps = torch.tensor(self._timesteps_host, dtype=torch.int64)
        self._history = None            # the previous step's m0 (fp32, on the device), kept by ``step``
        self.lower_order_nums = 0

    scale_model_input = DDIMScheduler.scale_model_input
    add_noise = DDIMScheduler.add_noise
    timesteps_host = DDIMScheduler.timesteps_host

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, self.config.num_train_timesteps - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        self._timesteps_host = [int(t) for t in timesteps]          # no device sync inside the loop
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self._history = None
        self.lower_order_nums = 0

    def step_order(self, i, history=None):
        """1 or 2 for step index ``i`` with ``history`` earlier steps taken since ``set_timesteps`` (default: a walk from step 0, i.e. ``i``).
        First order: solver_order 1, no history yet, or the last step of a walk of fewer than 15 steps under lower_order_final.  Step 0 has no
        earlier timestep on the grid, so it is first order whatever the history."""
        n = len(self._timesteps_host)
        history = i if history is None else history
        final = i == n - 1 and self.config.lower_order_final and n < 15
        return 1 if (self.config.solver_order == 1 or history < 1 or i < 1 or final) else 2

    def step_coefficients(self, i, history=None):
        """``DPMStepCoefficients`` of step index ``i`` (from timesteps[i] to timesteps[i + 1]; after the last one to timestep 0), formed in
        double with expm1; ``history`` as in ``step_order``.  No device sync."""
        ts = self._timesteps_host
        if not 0 <= i < len(ts):
            raise IndexError(f"step index {i} outside the {len(ts)} timesteps")
        s0, t = ts[i], (ts[i + 1] if i + 1 < len(ts) else 0)
        lam, alpha, sigma = self._lambda_t, self._alpha_t, self._sigma_t
        h = lam[t] - lam[s0]
        a = -alpha[t] * math.expm1(-h)                       # -alpha_t (e^-h - 1) > 0
        c_x = sigma[t] / sigma[s0]
        order = self.step_order(i, history)
        if order == 1:
            return DPMStepCoefficients(alpha[s0], sigma[s0], c_x, a, 0.0, 1)
        r0 = (lam[s0] - lam[ts[i - 1]]) / h
        if self.config.solver_type == "midpoint":
            k = a / (2.0 * r0)                               # x_t = c_x x + a D0 + a / 2 D1,  D0 = m0, D1 = (m0 - m1) / r0
        else:
            k = alpha[t] * (math.expm1(-h) / h + 1.0) / r0   # heun: x_t = c_x x + a D0 + alpha_t ((e^-h - 1) / h + 1) D1
        return DPMStepCoefficients(alpha[s0], sigma[s0], c_x, a + k, -k, 2)

    def step(self, model_output, timestep, sample, return_dict=True):
        """diffusers 0.11.1 ``DPMSolverMultistepScheduler.step``: the history (the previous step's x0 prediction) and the lower-order counter
        live in the object and are reset by ``set_timesteps``.  The arithmetic runs in HIP (nr_cfg_dpmpp_step)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not (model_output.is_cuda and sample.is_cuda):
            raise NotImplementedError("DPMSolverMultistepScheduler.step runs in the HIP kernel nr_cfg_dpmpp_step: CUDA (ROCm) tensors required, "
                                      "there is no CPU fallback")
        from . import ops
        t = int(timestep)
        i = self._timesteps_host.index(t) if t in self._timesteps_host else len(self._timesteps_host) - 1
        k = self.step_coefficients(i, self.lower_order_nums)
        if self._history is None:
            self._history = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        prev, _ = ops.cfg_dpmpp_step(model_output.float().contiguous(), sample.float().contiguous(), 1.0, k.alpha_s, k.sigma_s, k.c_x, k.c_m0,
                                     k.c_m1, m1=self._history if k.order == 2 else None, do_cfg=False,
                                     prediction_type=self.config.prediction_type, m0_out=self._history)
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        prev = prev.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)
