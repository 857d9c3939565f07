"""Test-side specification of the stochastic samplers (test infrastructure, never shipped; torch on the CPU): DDIM with ``eta``
("Euler a" is its ``eta = 1``), SDE-DPM-Solver++(2M) and the LCM scheduler, restated on top of ``tests/dpm_solver_cpu.py`` /
``tests/ddim_variants.py`` in the manner of DESIGN.md section 25.1.  Section 29 writes the definitions out.

PARITY NOTE: "parity unpinned" to diffusers itself (not installed, not installable here): the formulas are written out from the
published ones -- ``DDIMScheduler.step`` with ``eta``, ``DPMSolverMultistepScheduler`` with ``algorithm_type="sde-dpmsolver++"`` /
``solver_type="midpoint"``, ``LCMScheduler`` with ``timestep_scaling = 10`` / ``sigma_data = 0.5`` and no guidance embedding.  The first-
order steps are stateless, so the REAL reference can run them: the glue parity, the order of the random draws included, is pinned
by driving the reference with this object (tests/golden/g18_stochastic.npz).

Everything is stated on THIS PROJECT'S timestep grid (the DDIM restatement's timesteps, ``prev_t = t - n // k``,
``final_alpha_cumprod``), so ``undo_step``, the pad frames, ``add_noise`` and the img2img window are untouched.  Notation as in
tests/dpm_solver_cpu.py: alpha = abar ** 0.5, sigma = (1 - abar) ** 0.5, lambda = log(alpha) - log(sigma), h = lambda_prev - lambda_t;
all 0-d tensors of ``alphas_cumprod``'s dtype (fp32 unless a test converts the tables), every product rounded on its own, left to right.
x0 is the DDIM step's pred_original_sample of the (guided, rescaled) model output.

    DDIM with eta:     var = ((1 - abar_prev) / (1 - abar_t)) * (1 - abar_t / abar_prev),   c_n = eta * var ** 0.5
                       sd_eta = (1 - abar_prev - c_n ** 2) ** 0.5       (the radicand clamped at 0: at abar_t = 0 and eta = 1 it is
                                                                          0 in exact arithmetic and may round below it)
                       prev = (alpha_prev * x0 + sd_eta * eps) + c_n * noise
    "euler_a":         DDIM at eta = 1
    SDE-DPM++ (2M):    c_x = (sigma_prev / sigma_t) * exp(-h),  b = alpha_prev * (exp(-2 h) - 1),  hb = 0.5 * b,  r_inv = 1 / (h0 / h)
                       c_n = sigma_prev * (1 - exp(-2 h)) ** 0.5
                       prev = ((c_x * x - b * x0) - hb * (r_inv * (x0 - x0_h))) + c_n * noise      (first order: without the hb term)
                       first order is forced exactly where DPMSolverCPU forces it
    LCM:               s = 10 t,  c_skip = 0.25 / (s ** 2 + 0.25),  c_out = s / (s ** 2 + 0.25) ** 0.5
                       not the last timestep:  c_x = alpha_prev * c_skip,  b = -(alpha_prev * c_out),  c_n = sigma_prev
                       the last timestep:      c_x = c_skip,               b = -c_out,                 c_n = 0
                       prev = (c_x * x - b * x0) + c_n * noise           (first order, no history ever)

DRAW RULE: a step is stochastic iff its c_n != 0.0, and a stochastic step draws ``torch.randn(sample.shape)`` (fp32, the default CPU
generator) inside ``step`` -- that is, wherever the loop calls ``scheduler.step``: both phases of a timestep, the plain loop of
``generate()``, and the reduced-resolution step inside RRG (at the reduced shape; its prev_sample is unused, the draw is made and
discarded).  A step that is not stochastic draws nothing.

It shares no code with elasticdiffusion_official_amd/.
"""
import torch

from oracle.ddim import StepOutput
from tests.dpm_solver_cpu import GAUSS_S, DPMSolverCPU, SolverOracle, gauss_var

SAMPLERS = ("ddim", "euler_a", "dpmsolver++", "dpmsolver++sde", "lcm")
STATELESS = {  # the three stateless stochastic steps the real reference can run (tests/golden/make_stochastic.py)
    "eta1": dict(sampler="ddim", eta=1.0),
    "sde1": dict(sampler="dpmsolver++sde", solver_order=1),
    "lcm": dict(sampler="lcm"),
}


class StochasticCPU(DPMSolverCPU):
    def __init__(self, sampler="ddim", eta=0.0, solver_order=2, lower_order_final=True, **overrides):
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta must be in [0, 1], got {eta!r}")
        if float(eta) != 0.0 and sampler != "ddim":
            raise ValueError(f"eta belongs to sampler='ddim', got sampler={sampler!r}")
        base = "ddim" if sampler in ("ddim", "euler_a") else "dpmsolver++"
        super().__init__(sampler=base, solver_order=solver_order, lower_order_final=lower_order_final, **overrides)
        self.kind = sampler
        self.eta = 1.0 if sampler == "euler_a" else float(eta)

    @property
    def deterministic(self):
        return self.kind == "dpmsolver++" or (self.kind in ("ddim", "euler_a") and self.eta == 0.0)

    # ---- scalars ------------------------------------------------------------------------------------------------------
    def ddim_eta_coefficients(self, t):
        """-> (sigma_t, alpha_t, alpha_prev, sd_eta, c_n) as 0-d tensors"""
        a_t, a_p = self.alphas_cumprod[int(t)], self._abar_prev(t)
        var = ((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)
        c_n = self.eta * var ** 0.5
        sd = torch.clamp(1 - a_p - c_n ** 2, min=0.0) ** 0.5
        return (1 - a_t) ** 0.5, a_t ** 0.5, a_p ** 0.5, sd, c_n

    def sde_coefficients(self, t, t_hist=None, is_last=None):
        """-> (sigma_t, alpha_t, c_x, b, 0.5 * b, r_inv, c_n) as 0-d tensors; r_inv is 0 where first order is forced"""
        a_t, a_p = self.alphas_cumprod[int(t)], self._abar_prev(t)
        sigma_t, alpha_t = (1 - a_t) ** 0.5, a_t ** 0.5
        sigma_p, alpha_p = (1 - a_p) ** 0.5, a_p ** 0.5
        lam_t, lam_p = self._lambda(a_t), self._lambda(a_p)
        h = lam_p - lam_t
        c_x = (sigma_p / sigma_t) * torch.exp(-h)
        e2 = torch.exp(-2.0 * h)
        b = alpha_p * (e2 - 1.0)
        c_n = sigma_p * (1.0 - e2) ** 0.5
        r_inv = torch.zeros_like(b)
        if self.second_order(t, t_hist, is_last):
            h0 = lam_t - self._lambda(self.alphas_cumprod[int(t_hist)])
            r_inv = 1.0 / (h0 / h)
        return sigma_t, alpha_t, c_x, b, 0.5 * b, r_inv, c_n

    def lcm_coefficients(self, t):
        """-> (sigma_t, alpha_t, c_x, b, c_n) as 0-d tensors; "last" is keyed by the timestep"""
        a_t, a_p = self.alphas_cumprod[int(t)], self._abar_prev(t)
        s = 10.0 * torch.tensor(float(int(t)), dtype=a_t.dtype)
        c_skip = 0.25 / (s ** 2 + 0.25)
        c_out = s / (s ** 2 + 0.25) ** 0.5
        if self.is_last(t):
            c_x, b, c_n = c_skip, -c_out, torch.zeros_like(c_skip)
        else:
            c_x, b, c_n = a_p ** 0.5 * c_skip, -(a_p ** 0.5 * c_out), (1 - a_p) ** 0.5
        return (1 - a_t) ** 0.5, a_t ** 0.5, c_x, b, c_n

    def noise_coefficient(self, t):
        """the c_n of the step at timestep ``t`` (0-d tensor; it does not depend on the order): != 0 <=> the step draws"""
        if self.deterministic:
            return torch.zeros((), dtype=self.alphas_cumprod.dtype)
        if self.kind in ("ddim", "euler_a"):
            return self.ddim_eta_coefficients(t)[4]
        if self.kind == "lcm":
            return self.lcm_coefficients(t)[4]
        return self.sde_coefficients(t)[6]

    # ---- the step -----------------------------------------------------------------------------------------------------
    def _x0_eps(self, m, t, x):
        a_t = self.alphas_cumprod[int(t)]
        if self.config.prediction_type == "epsilon":
            return (x - (1 - a_t) ** 0.5 * m) / a_t ** 0.5, m
        return (a_t ** 0.5) * x - ((1 - a_t) ** 0.5) * m, (a_t ** 0.5) * m + ((1 - a_t) ** 0.5) * x

    def step(self, model_output, timestep, sample, eta=0.0, history=None, is_last=None, noise=None, **_):
        """``history`` as in DPMSolverCPU.step.  ``noise``: the draw of a stochastic step when the caller has made it (the kernel
        tests); None draws ``torch.randn(sample.shape)`` here, where the reference calls ``scheduler.step``."""
        if self.deterministic:
            return super().step(model_output, timestep, sample, history=history, is_last=is_last)
        x0, eps = self._x0_eps(model_output, timestep, sample)
        if self.kind in ("ddim", "euler_a"):
            _, _, sp, sd, c_n = self.ddim_eta_coefficients(timestep)
            prev = sp * x0 + sd * eps
        elif self.kind == "lcm":
            _, _, c_x, b, c_n = self.lcm_coefficients(timestep)
            prev = c_x * sample - b * x0
        else:
            t_hist = None if history is None else history[1]
            _, _, c_x, b, hb, r_inv, c_n = self.sde_coefficients(timestep, t_hist, is_last)
            prev = c_x * sample - b * x0
            if self.second_order(timestep, t_hist, is_last):
                prev = prev - hb * (r_inv * (x0 - history[0]))
        if float(c_n) != 0.0:
            if noise is None:
                noise = torch.randn(sample.shape, dtype=sample.dtype)
            prev = prev + c_n * noise
        return StepOutput(prev_sample=prev, pred_original_sample=x0)


class StochasticOracle(SolverOracle):
    """``SolverOracle`` with a ``StochasticCPU`` scheduler.  The oracle chain calls ``self.scheduler.step`` where the reference does
    -- the resampling phase, the RePaint second phase, the reduced-resolution step inside RRG (without a history: its
    pred_original_sample is all that is used), the plain loop -- and a stochastic step draws right there, so the draws fall in the
    reference's order by construction.  With nothing stochastic every expression and every draw is ``SolverOracle``'s."""

    def __init__(self, unet, vae, scheduler, *args, **kwargs):
        assert isinstance(scheduler, StochasticCPU)
        super().__init__(unet, vae, scheduler, *args, **kwargs)


# ---- the Gaussian toy problem (DESIGN.md sections 25.5 / 29.4): data ~ N(0, s^2) per element, exact predictor ----------------------
def gauss_predictor(sched, s=GAUSS_S):
    """the exact noise predictor eps*(x, t) = (sigma_t / var(abar_t)) x with the scalar formed first: ONE product per element, which
    a device evaluates to the same bits as the CPU (a division by a scalar need not be)"""
    def predictor(x, t):
        abar = sched.alphas_cumprod[int(t)]
        return float((1 - abar) ** 0.5 / gauss_var(abar, s)) * x
    return predictor


def gauss_start(sched, n, seed, s=GAUSS_S):
    """x_T drawn from the exact marginal N(0, var(abar_T)) of the first timestep; seeds the default generator"""
    torch.manual_seed(seed)
    a_T = sched.alphas_cumprod[int(sched.timesteps[0])]
    return torch.randn(n) * float(gauss_var(a_T, s) ** 0.5)


def gauss_std_error(sched, x_end, s=GAUSS_S):
    """|std(x_end) / sqrt(var(abar_end)) - 1|"""
    a_end = sched._abar_prev(sched.timesteps[-1]).double()
    return abs(float(x_end.double().std() / gauss_var(a_end, s) ** 0.5) - 1.0)


TOY_N, TOY_SEED = 1 << 20, 0
TOY_SAMPLERS = {  # LCM is not a consistent solver of this problem and is left out
    "eta1": dict(sampler="ddim", eta=1.0),
    "sde1": dict(sampler="dpmsolver++sde", solver_order=1),
    "sde2": dict(sampler="dpmsolver++sde", solver_order=2),
}


def toy_chain(name, steps, record=None):
    """The toy problem through the restatement in fp32 -> (scheduler, x_end).  ``record`` (a list) receives (t, t_hist or None,
    is_last, noise or None) per step, what a device loop needs to repeat the chain on the same noise."""
    sched = StochasticCPU(**TOY_SAMPLERS[name])
    sched.set_timesteps(steps)
    x = gauss_start(sched, TOY_N, TOY_SEED)
    pred = gauss_predictor(sched)
    hist = None
    for t in sched.timesteps:
        noise = torch.randn(x.shape) if float(sched.noise_coefficient(t)) != 0.0 else None
        out = sched.step(pred(x, t), t, x, history=hist, noise=noise)
        if record is not None:
            record.append((int(t), None if hist is None else int(hist[1]), sched.is_last(t), noise))
        hist = (out["pred_original_sample"], t)
        x = out["prev_sample"]
    return sched, x


_TOY_CACHE = {}


def toy_error(name, steps):
    """std error of ``toy_chain`` (computed once per process)"""
    if (name, steps) not in _TOY_CACHE:
        sched, x = toy_chain(name, steps)
        _TOY_CACHE[name, steps] = gauss_std_error(sched, x)
    return _TOY_CACHE[name, steps]


# ---- the end-to-end cases of tests/golden/g18_stochastic.npz: dpm_solver_cpu.SOLVER_CASES' four geometries -------------------------
def run_reference_case(name, sampler_kw):
    """Drive the REAL reference's generate_image with a stateless stochastic step injected (needs the reference checkout).
    -> (final latent, torch.rand(4) drawn right after)"""
    from tests import dpm_solver_cpu as D
    from tests.ddim_variants import embed_fn
    from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
    from tests.golden.ref_loader import make_reference_pipeline
    c = D.SOLVER_CASES[name]
    xl = c["sd"].startswith("XL")
    cn = bool(c.get("controlnet"))
    pipe, ref = make_reference_pipeline(FakeUNet(c["sample"], xl=xl), FakeVAE(), StochasticCPU(**sampler_kw, **c["sched"]),
                                        embed_fn(xl), sd_version=c["sd"], view_batch_size=D.VBS,
                                        controlnet=FakeControlNet() if cn else None)
    pipe.random_downasmple_pre = {}
    pipe.seed_everything(D.SEED)
    cap = {}
    orig = pipe.decode_latents

    def grab(z):
        cap["z"] = z.clone()
        return orig(z)

    pipe.decode_latents = grab
    kw = D.case_kwargs(name)
    if cn:  # as dpm_solver_cpu.run_reference_case: VaeImageProcessor.preprocess is the identity for a float tensor
        pipe.control_image_processor = type("P", (), {"preprocess": staticmethod(lambda image, height, width: image)})()
        kw.update(D.condition_kwargs(name))
    pipe.generate_image(prompts="p", negative_prompts="", progress=lambda it: it, rrg_scherduler_cls=ref.CosineScheduler, **kw)
    return cap["z"], torch.rand(4)


def run_oracle_case(name, sampler_kw, **extra):
    """The same case through StochasticOracle -> (final latent, torch.rand(4) tail)"""
    from tests import dpm_solver_cpu as D
    from tests.ddim_variants import embed_fn
    from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
    c = D.SOLVER_CASES[name]
    xl = c["sd"].startswith("XL")
    orc = StochasticOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), StochasticCPU(**sampler_kw, **c["sched"]), embed_fn(xl),
                           sd_version=c["sd"], view_batch_size=D.VBS, pooled_dim=16 if xl else None,
                           controlnet=FakeControlNet() if c.get("controlnet") else None)
    orc.seed_everything(D.SEED)
    z = orc.generate_latent(["p"], "", **D.case_kwargs(name), **D.condition_kwargs(name), **extra)
    return z, torch.rand(4)
