"""Host-side schedules: the DDIM coefficient tables the HIP kernels consume and the RRG weight schedules.

``DDIMSchedule`` plays the role of the ``diffusers`` ``DDIMScheduler`` the reference loads at
/root/reference/elastic_diffusion.py:153 (diffusers==0.21.4 is not vendored; its eta=0 algorithm is restated).
Only *scalars* are produced here -- every per-element operation of ``scheduler.step`` / ``add_noise`` /
``undo_step`` runs in libelastic_hip.so.  Scalars are computed with fp32 torch ops in the same order diffusers uses
(``alphas_cumprod[t] ** 0.5`` etc.) so that the kernels reproduce the reference's torch-CPU results bit for bit.

What a ``scheduler_config.json`` may say and is honoured (DESIGN.md section 14 writes the definitions out):
``prediction_type`` epsilon / v_prediction, ``timestep_spacing`` leading / linspace / trailing and
``rescale_betas_zero_snr``.  ``clip_sample``, thresholding and ``sample`` prediction are refused.

``DPMSolverSchedule`` is the same schedule with the host scalars of the DPM-Solver++(2M) update; a snapshot's
``_class_name`` never selects it.

The stochastic samplers are the same updates with other scalars plus ``noise_coefficient(t) * noise``:
``DDIMSchedule(eta=...)`` ("Euler a" is eta = 1), ``DPMSolverSchedule(algorithm_type="sde-dpmsolver++")`` and ``LCMSchedule``.  A step
whose noise coefficient is 0.0 is not stochastic and draws nothing.
"""
from types import SimpleNamespace

import numpy as np
import torch


PREDICTION_TYPES = ("epsilon", "v_prediction")
TIMESTEP_SPACINGS = ("leading", "linspace", "trailing")


def rescale_zero_terminal_snr(betas):
    """diffusers' ``rescale_zero_terminal_snr`` (Lin et al. 2023, algorithm 1) in its fp32 operation order: shift and
    scale sqrt(alpha_bar) so that the last timestep has exactly zero SNR and the first keeps its value."""
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first = alphas_bar_sqrt[0].clone()
    last = alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= last
    alphas_bar_sqrt *= first / (first - last)
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1 - alphas


def check_eta(eta):
    """``eta`` of the DDIM step as a float in [0, 1] (0 = deterministic, 1 = the ancestral step); ValueError otherwise."""
    try:
        e = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta must be a number in [0, 1], got {eta!r}") from None
    if not 0.0 <= e <= 1.0:  # also refuses NaN
        raise ValueError(f"eta must be in [0, 1], got {eta!r}")
    return e


class DDIMSchedule:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon", timestep_spacing="leading",
                 clip_sample=False, rescale_betas_zero_snr=False, eta=0.0):
        self.eta = check_eta(eta)
        if prediction_type not in PREDICTION_TYPES:
            raise NotImplementedError(f"prediction_type {prediction_type!r}: the HIP DDIM kernels implement "
                                      f"{' / '.join(PREDICTION_TYPES)}")
        if clip_sample:
            raise NotImplementedError("clip_sample=True is not used by any SD / SDXL scheduler config")
        if timestep_spacing not in TIMESTEP_SPACINGS:
            raise NotImplementedError(f"timestep_spacing {timestep_spacing!r}: one of {' / '.join(TIMESTEP_SPACINGS)}")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, set_alpha_to_one=set_alpha_to_one,
                                      steps_offset=steps_offset, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, clip_sample=clip_sample,
                                      rescale_betas_zero_snr=bool(rescale_betas_zero_snr))
        if beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(beta_schedule)
        if rescale_betas_zero_snr:  # betas, alphas_cumprod and final_alpha_cumprod all come from the rescaled betas
            self.betas = rescale_zero_terminal_snr(self.betas)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = None

    @classmethod
    def from_config_dir(cls, model_dir, **overrides):
        """``DDIMScheduler.from_pretrained(model_key, subfolder="scheduler")`` (ED:153) for a local HF snapshot: reads
        ``<model_dir>/scheduler/scheduler_config.json`` when present (keys this class does not know are ignored, values
        it cannot honour -- clip_sample, sample prediction -- raise NotImplementedError), defaults otherwise.
        ``overrides`` replace single keys of the file / the defaults (the command line's --prediction_type etc.); None
        values are dropped."""
        import json
        import os
        path = None if model_dir is None else os.path.join(model_dir, "scheduler", "scheduler_config.json")
        overrides = {k: v for k, v in overrides.items() if v is not None}
        if model_dir is None or not os.path.isfile(path):
            return cls(**overrides)
        cfg = dict(json.load(open(path)), **overrides)
        known = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "set_alpha_to_one", "steps_offset",
                 "prediction_type", "timestep_spacing", "clip_sample", "rescale_betas_zero_snr", "eta")
        return cls(**{k: cfg[k] for k in known if k in cfg})

    def set_timesteps(self, num_inference_steps):
        n = self.config.num_train_timesteps
        if num_inference_steps > n:
            raise ValueError(f"num_inference_steps {num_inference_steps} > num_train_timesteps {n}")
        self.num_inference_steps = num_inference_steps
        spacing = self.config.timestep_spacing
        if spacing == "linspace":
            ts = np.linspace(0, n - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif spacing == "leading":
            ratio = n // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
            ts = ts + self.config.steps_offset
        else:  # trailing
            ts = np.round(np.arange(n, 0, -n / num_inference_steps)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts)  # int64: str(t) == "tensor(981)"
        return self.timesteps

    @staticmethod
    def img2img_window(num_inference_steps, strength):
        """diffusers' ``get_timesteps`` of the image-to-image pipelines: the index ``t_start`` of the first timestep an
        image-to-image run of this ``strength`` executes -- n = min(int(T * strength), T) steps, t_start = max(T - n, 0).
        ``strength`` outside (0, 1], or one that leaves no step (n < 1), raises ValueError."""
        T = int(num_inference_steps)
        try:
            s = float(strength)
        except (TypeError, ValueError):
            raise ValueError(f"strength must be a number in (0, 1], got {strength!r}") from None
        if not 0.0 < s <= 1.0:  # also refuses NaN
            raise ValueError(f"strength must be in (0, 1], got {strength!r}")
        n = min(int(T * s), T)
        if n < 1:
            raise ValueError(f"strength {strength!r} leaves no step of {T} to run (int({T} * strength) < 1)")
        return max(T - n, 0)

    # ---- scalar tables ---------------------------------------------------------------------------
    def step_coefficients(self, t):
        """(sqrt(1-abar_t), sqrt(abar_t), sqrt(abar_prev), sqrt(1-abar_prev)) as python floats holding fp32 values."""
        t = int(t)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps  # for every spacing, as diffusers
        a_t = self.alphas_cumprod[t]
        if self.config.prediction_type == "epsilon" and float(a_t) == 0.0:
            raise ValueError(
                f"timestep {t} has alpha_bar = 0 (rescale_betas_zero_snr) and the model predicts epsilon: the DDIM step "
                "divides by sqrt(alpha_bar_t) = 0.  A zero-terminal-SNR schedule needs prediction_type='v_prediction' "
                "(or a timestep spacing that does not visit the last training timestep)")
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        sqrt_beta_t = (1 - a_t) ** 0.5
        sqrt_alpha_t = a_t ** 0.5
        sqrt_alpha_prev = a_prev ** 0.5
        if self.eta != 0.0:  # the last scalar becomes (1 - abar_prev - c_n^2)^0.5
            c_n = self._eta_noise(a_t, a_prev)
            sd_eta = torch.clamp(1 - a_prev - c_n ** 2, min=0.0) ** 0.5
            return tuple(float(v) for v in (sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sd_eta))
        sqrt_1m_alpha_prev = (1 - a_prev - 0.0) ** 0.5
        return tuple(float(v) for v in (sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_1m_alpha_prev))

    def _abar_pair(self, t):
        t = int(t)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[t], self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod

    def _eta_noise(self, a_t, a_prev):
        var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        return self.eta * var ** 0.5

    def noise_coefficient(self, t):
        """c_n of the step at timestep ``t`` as a python float holding an fp32 value: the update is the deterministic one (with
        ``step_coefficients``' scalars) plus c_n * noise, and the step is stochastic -- draws a latent-sized normal sample on the
        host -- iff c_n != 0.0.  DDIM: eta * (((1 - abar_prev) / (1 - abar_t)) * (1 - abar_t / abar_prev)) ** 0.5, diffusers'
        ``eta * variance ** 0.5``; 0.0 at eta = 0."""
        if self.eta == 0.0:
            return 0.0
        return float(self._eta_noise(*self._abar_pair(t)))

    def add_noise_coefficients(self, t):
        a = self.alphas_cumprod[int(t)]
        return float(a ** 0.5), float((1 - a) ** 0.5)

    def undo_coefficients(self, t_next):
        """[(sqrt(1-beta_{t'+k}), sqrt(beta_{t'+k}))] for the n_train // n_steps forward sub-steps of undo_step
        (elastic_diffusion.py:692-704)."""
        n_sub = self.config.num_train_timesteps // self.num_inference_steps
        b = self.betas[int(t_next): int(t_next) + n_sub]
        if len(b) != n_sub:
            raise IndexError("undo_step would index betas past num_train_timesteps (the reference raises too)")
        return torch.stack([(1 - b) ** 0.5, b ** 0.5], dim=1).contiguous()  # fp32 [n_sub, 2]


SAMPLERS = ("ddim", "euler_a", "dpmsolver++", "dpmsolver++sde", "lcm")
ALGORITHM_TYPES = ("dpmsolver++", "sde-dpmsolver++")


class DPMSolverSchedule(DDIMSchedule):
    """DPM-Solver++(2M) (arXiv 2211.01095; diffusers' ``DPMSolverMultistepScheduler`` with ``algorithm_type="dpmsolver++"``,
    ``solver_type="midpoint"``, no Karras sigmas, no thresholding) on ``DDIMSchedule``'s timestep grid: the timesteps,
    ``prev_t = t - n // k``, ``final_alpha_cumprod``, ``add_noise`` and ``undo_step`` scalars are the parent's for every spacing, so
    everything around the sample update is unchanged.  It accepts and refuses what ``DDIMSchedule`` does.

    ``solver_order`` 1 or 2; ``lower_order_final``: the last step of a run of fewer than 15 steps is first order."""

    def __init__(self, *args, solver_order=2, lower_order_final=True, algorithm_type="dpmsolver++", **kwargs):
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        if algorithm_type not in ALGORITHM_TYPES:
            raise ValueError(f"algorithm_type must be one of {ALGORITHM_TYPES}, got {algorithm_type!r}")
        if kwargs.get("eta", 0.0) != 0.0:
            raise ValueError("eta belongs to the DDIM step; the stochastic multistep solver is algorithm_type='sde-dpmsolver++'")
        super().__init__(*args, **kwargs)
        self.solver_order = int(solver_order)
        self.lower_order_final = bool(lower_order_final)
        self.algorithm_type = algorithm_type

    def _second_order(self, t, t_hist, is_last, a_prev):
        second = t_hist is not None and self.solver_order == 2
        if second and is_last and self.lower_order_final and self.num_inference_steps < 15:
            second = False
        if second and (float(a_prev) == 1.0 or float(self.alphas_cumprod[int(t_hist)]) == 0.0):
            second = False
        return second

    def multistep_coefficients(self, t, t_hist=None, is_last=False):
        """(sqrt(1-abar_t), sqrt(abar_t), c_x, b, 0.5 * b, r_inv) as python floats holding fp32 values, for the update
        ``prev = (c_x * x - b * x0) - (0.5 * b) * (r_inv * (x0 - x0_hist))``: with alpha = abar ** 0.5, sigma = (1 - abar) ** 0.5 and
        lambda = log(alpha) - log(sigma),  h = lambda_prev - lambda_t,  c_x = sigma_prev / sigma_t,  b = alpha_prev * (exp(-h) - 1),
        r_inv = 1 / ((lambda_t - lambda_{t_hist}) / h).  ``t_hist``: the timestep the history x0 was taken at, None without one.
        ``r_inv == 0.0`` says that the step is FIRST order (the history is not to be passed): no history, ``solver_order == 1``,
        the last step (``is_last``) of fewer than 15 under ``lower_order_final``, or abar_prev == 1 / abar_{t_hist} == 0, where
        h / h0 is infinite.  Under ``algorithm_type="sde-dpmsolver++"`` c_x = (sigma_prev / sigma_t) * exp(-h)
        and b = alpha_prev * (exp(-2 h) - 1); ``noise_coefficient`` is the scalar of the noise term that update adds."""
        sqrt_beta_t, sqrt_alpha_t = self.step_coefficients(t)[:2]  # raises for an epsilon model at abar_t = 0, as the DDIM step
        a_t, a_prev = self._abar_pair(t)

        def lam(a):
            return torch.log(a ** 0.5) - torch.log((1 - a) ** 0.5)

        h = lam(a_prev) - lam(a_t)
        c_x = (1 - a_prev) ** 0.5 / (1 - a_t) ** 0.5
        if self.algorithm_type == "sde-dpmsolver++":
            c_x = c_x * torch.exp(-h)
            b = a_prev ** 0.5 * (torch.exp(-2.0 * h) - 1.0)
        else:
            b = a_prev ** 0.5 * (torch.exp(-h) - 1.0)
        r_inv = torch.zeros_like(b)
        if self._second_order(t, t_hist, is_last, a_prev):
            h0 = lam(a_t) - lam(self.alphas_cumprod[int(t_hist)])
            r_inv = 1.0 / (h0 / h)
        return (sqrt_beta_t, sqrt_alpha_t) + tuple(float(v) for v in (c_x, b, 0.5 * b, r_inv))

    def noise_coefficient(self, t):
        """c_n = sigma_prev * (1 - exp(-2 h)) ** 0.5 under ``algorithm_type="sde-dpmsolver++"`` (0.0 at abar_prev == 1, where the step
        returns x0), 0.0 for the deterministic solver; the same for both orders."""
        if self.algorithm_type != "sde-dpmsolver++":
            return 0.0
        a_t, a_prev = self._abar_pair(t)
        h = (torch.log(a_prev ** 0.5) - torch.log((1 - a_prev) ** 0.5)) - (torch.log(a_t ** 0.5) - torch.log((1 - a_t) ** 0.5))
        return float((1 - a_prev) ** 0.5 * (1.0 - torch.exp(-2.0 * h)) ** 0.5)


class LCMSchedule(DPMSolverSchedule):
    """The scheduler an LCM-LoRA is sampled with (diffusers' ``LCMScheduler``: ``timestep_scaling = 10``, ``sigma_data = 0.5``, no
    guidance embedding), on ``DDIMSchedule``'s timestep grid like everything else.  With s = 10 t,
    c_skip = 0.25 / (s^2 + 0.25) and c_out = s / (s^2 + 0.25)^0.5 the denoised sample is d = c_out * x0 + c_skip * x, and the step is
    prev = alpha_prev * d + sigma_prev * noise, on the last timestep prev = d.  It is the first-order multistep form with its own
    scalars and never a history: ``multistep_coefficients`` returns c_x = alpha_prev * c_skip, b = -(alpha_prev * c_out) (last
    timestep: c_skip, -c_out) and r_inv = 0.  It accepts and refuses what ``DDIMSchedule`` does."""

    def __init__(self, *args, **kwargs):
        for k in ("solver_order", "lower_order_final", "algorithm_type"):
            if k in kwargs:
                raise ValueError(f"LCMSchedule takes no {k}")
        super().__init__(*args, solver_order=1, **kwargs)

    def _lcm(self, t):
        a_t, a_prev = self._abar_pair(t)
        s = 10.0 * torch.tensor(float(int(t)), dtype=torch.float32)
        c_skip = 0.25 / (s ** 2 + 0.25)
        c_out = s / (s ** 2 + 0.25) ** 0.5
        if int(t) == int(self.timesteps[-1]):
            return c_skip, -c_out, torch.zeros(())
        return a_prev ** 0.5 * c_skip, -(a_prev ** 0.5 * c_out), (1 - a_prev) ** 0.5

    def multistep_coefficients(self, t, t_hist=None, is_last=False):
        sqrt_beta_t, sqrt_alpha_t = self.step_coefficients(t)[:2]
        c_x, b, _ = self._lcm(t)
        return (sqrt_beta_t, sqrt_alpha_t) + tuple(float(v) for v in (c_x, b, 0.5 * b, torch.zeros(())))

    def noise_coefficient(self, t):
        return float(self._lcm(t)[2])


class CosineScheduler:
    """RRG weight: factor * (0.5 (1 + cos(pi i / steps))) ** cosine_scale, zero from ``steps`` on
    (elastic_diffusion.py:96-107)."""

    def __init__(self, steps, cosine_scale, factor=0.01):
        self.steps = steps
        self.cosine_scale = cosine_scale
        self.factor = factor

    def __call__(self, t, *args, **kwargs):
        if t >= self.steps:
            return 0
        return self.factor * ((0.5 * (1 + np.cos(np.pi * t / self.steps))) ** self.cosine_scale)


class LinearScheduler:
    """elastic_diffusion.py:73-82"""

    def __init__(self, steps, start_val, stop_val):
        self.steps = steps
        self.start_val = start_val
        self.stop_val = stop_val

    def __call__(self, t, *args, **kwargs):
        if t >= self.steps:
            return self.stop_val
        return self.start_val + (self.stop_val - self.start_val) / self.steps * t


class ConstScheduler:
    """elastic_diffusion.py:85-94"""

    def __init__(self, steps, start_val, stop_val):
        self.steps = steps
        self.start_val = start_val
        self.stop_val = stop_val

    def __call__(self, t, *args, **kwargs):
        return self.stop_val if t >= self.steps else self.start_val
