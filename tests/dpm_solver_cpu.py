"""Test-side specification of DPM-Solver++(2M) sampling (test infrastructure, never shipped; torch on the CPU).

``DPMSolverCPU`` restates the arithmetic of diffusers' ``DPMSolverMultistepScheduler`` with ``algorithm_type="dpmsolver++"``,
``solver_type="midpoint"``, orders 1 and 2, no Karras sigmas and no thresholding (Lu et al., arXiv 2211.01095, the multistep 2M
update in its data-prediction form), as a subclass of ``oracle.ddim.DDIMOracle`` through ``tests/ddim_variants.py::DDIMVariants``.
It is stated on THIS PROJECT'S timestep grid, not on diffusers' own DPM grid: the timesteps, ``prev_t = t - n // k`` and
``final_alpha_cumprod`` are the DDIM restatement's for every spacing, zero-SNR betas included, so that the RePaint ``undo_step``
(n // k forward sub-steps from ``betas``) still returns to ``t`` exactly.  DESIGN.md section 25 writes the definitions out.

PARITY NOTE: as for oracle/ddim.py, "parity unpinned" to diffusers itself (not installed, not installable here): the formulas are
written out from the published ones.  The first-order step is stateless, so the REAL reference can run it: the glue parity is
pinned by driving the reference with this object at ``solver_order=1`` (tests/golden/g16_dpm_solver.npz).

With alpha = abar ** 0.5, sigma = (1 - abar) ** 0.5, lambda = log(alpha) - log(sigma), all 0-d tensors of ``alphas_cumprod``'s dtype
(fp32 unless a test converts the tables):

    x0    = the DDIM step's pred_original_sample of the model output            (epsilon: (x - sigma_t m) / alpha_t;  v: alpha_t x - sigma_t m)
    h     = lambda_prev - lambda_t,   c_x = sigma_prev / sigma_t,   b = alpha_prev * (exp(-h) - 1)
    order 1:   prev = c_x * x - b * x0
    order 2:   h0 = lambda_t - lambda_{t_h},  r_inv = 1 / (h0 / h),  D1 = r_inv * (x0 - x0_h)
               prev = (c_x * x - b * x0) - (0.5 * b) * D1
    left to right, every product rounded on its own.

First order is forced when there is no history, when ``solver_order == 1``, on the last step if ``lower_order_final`` and
``num_inference_steps < 15``, and when abar_prev == 1 or abar_{t_h} == 0 (h or h0 infinite: r_inv would be inf or the difference
term 0 * inf).

``step`` is stateless: the history is an argument.  ``SolverOracle`` places it in the ElasticDiffusion loop with the history rule
of section 25: both phases of timestep index i use the x0 written by the last full-resolution phase of index i - 1; the
reduced-resolution step inside RRG only consumes ``pred_original_sample`` and is unchanged.

It shares no code with elasticdiffusion_official_amd/.
"""
import numpy as np
import torch

from oracle.ddim import StepOutput
from oracle.elastic_oracle import CosineScheduler
from tests.ddim_variants import DDIMVariants
from tests.img2img_cpu import Img2ImgOracle, blend, init_latent, latent_mask, to_vae_input, window

SAMPLERS = ("ddim", "dpmsolver++")


class DPMSolverCPU(DDIMVariants):
    def __init__(self, sampler="dpmsolver++", solver_order=2, lower_order_final=True, **overrides):
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        super().__init__(**overrides)
        self.sampler, self.solver_order, self.lower_order_final = sampler, int(solver_order), bool(lower_order_final)

    # ---- scalars ------------------------------------------------------------------------------------------------------
    def _abar_prev(self, t):
        prev_t = int(t) - self.config.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod

    @staticmethod
    def _lambda(abar):
        return torch.log(abar ** 0.5) - torch.log((1 - abar) ** 0.5)

    def is_last(self, t):
        return int(t) == int(self.timesteps[-1])

    def second_order(self, t, t_hist, is_last=None):
        """does the step at timestep ``t`` with a history taken at ``t_hist`` (None = no history) run at second order?"""
        if t_hist is None or self.solver_order == 1:
            return False
        if is_last is None:
            is_last = self.is_last(t)
        if is_last and self.lower_order_final and self.num_inference_steps < 15:
            return False
        return bool(self._abar_prev(t) != 1) and bool(self.alphas_cumprod[int(t_hist)] != 0)

    def coefficients(self, t, t_hist=None, is_last=None):
        """-> (sigma_t, alpha_t, c_x, b, 0.5 * b, r_inv) as 0-d tensors; r_inv is 0 where first order is forced"""
        a_t, a_p = self.alphas_cumprod[int(t)], self._abar_prev(t)
        sigma_t, alpha_t = (1 - a_t) ** 0.5, a_t ** 0.5
        sigma_p, alpha_p = (1 - a_p) ** 0.5, a_p ** 0.5
        lam_t, lam_p = self._lambda(a_t), self._lambda(a_p)
        h = lam_p - lam_t
        c_x = sigma_p / sigma_t
        b = alpha_p * (torch.exp(-h) - 1.0)
        r_inv = torch.zeros_like(b)
        if self.second_order(t, t_hist, is_last):
            h0 = lam_t - self._lambda(self.alphas_cumprod[int(t_hist)])
            r_inv = 1.0 / (h0 / h)
        return sigma_t, alpha_t, c_x, b, 0.5 * b, r_inv

    # ---- the step -----------------------------------------------------------------------------------------------------
    def step(self, model_output, timestep, sample, eta=0.0, history=None, is_last=None, **_):
        """``history`` = (x0 of the previous timestep, that timestep) or None.  Stateless: nothing is kept between calls."""
        ddim = super().step(model_output, timestep, sample, eta=eta)
        if self.sampler == "ddim":
            return ddim
        x0 = ddim["pred_original_sample"]
        t_hist = None if history is None else history[1]
        _, _, c_x, b, hb, r_inv = self.coefficients(timestep, t_hist, is_last)
        prev = c_x * sample - b * x0
        if self.second_order(timestep, t_hist, is_last):
            d1 = r_inv * (x0 - history[0])
            prev = prev - hb * d1
        return StepOutput(prev_sample=prev, pred_original_sample=x0)


def solve_chain(sched, x, predictor):
    """The plain sampling loop over ``sched.timesteps`` with the previous iteration's x0 as history:
    ``predictor(x, t)`` -> model output.  -> final sample"""
    hist = None
    for t in sched.timesteps:
        out = sched.step(predictor(x, t), t, x, history=hist)
        hist = (out["pred_original_sample"], t)
        x = out["prev_sample"]
    return x


# ---- the Gaussian ODE: data ~ N(0, s^2) per element has an exact predictor and an exact solution --------
GAUSS_S = 2.0


def gauss_var(abar, s=GAUSS_S):
    return abar * s * s + 1 - abar


def gauss_eps(sched, s=GAUSS_S):
    """the exact noise predictor eps*(x, t) = sigma_t x / var(abar_t)"""
    def predictor(x, t):
        abar = sched.alphas_cumprod[int(t)]
        return (1 - abar) ** 0.5 * x / gauss_var(abar, s)
    return predictor


def gauss_exact_end(sched, x_T, s=GAUSS_S):
    """x at the last abar_prev of the chain, from x_T at the first timestep"""
    a_T = sched.alphas_cumprod[int(sched.timesteps[0])].double()
    a_end = sched._abar_prev(sched.timesteps[-1]).double()
    return x_T.double() * (gauss_var(a_end, s) / gauss_var(a_T, s)) ** 0.5


def gauss_error(steps, sampler, dtype=torch.float32, seed=0, **kw):
    """relative L2 error at the end of a ``steps``-step chain on the Gaussian ODE"""
    sched = DPMSolverCPU(sampler=sampler, **kw)
    if dtype == torch.float64:
        sched.alphas_cumprod = sched.alphas_cumprod.double()
        sched.final_alpha_cumprod = sched.final_alpha_cumprod.double()
    sched.set_timesteps(steps)
    x_T = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(seed)).to(dtype)
    got = solve_chain(sched, x_T, gauss_eps(sched))
    want = gauss_exact_end(sched, x_T)
    return float((got.double() - want).norm() / want.norm())


# ---- the loop -----------------------------------------------------------------------------------------------------------
class SolverOracle(Img2ImgOracle):
    """``Img2ImgOracle.generate_latent`` with the multistep history made explicit.  ``self.scheduler`` is a ``DPMSolverCPU``; with
    ``sampler="ddim"`` every expression is the parent's."""

    @torch.no_grad()
    def generate_latent(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                        guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                        rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                        progress=lambda it: it, condition_image=None, controlnet_conditioning_scale=1.0,
                        trace=None, logs=None, guidance_rescale=0.0, init_image=None, strength=1.0, mask_image=None):
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
        t_start = window(num_inference_steps, strength)
        if init_image is None and (strength != 1.0 or mask_image is not None):
            raise ValueError("strength / mask_image need init_image")
        self.guidance_rescale = guidance_rescale
        downsample_size = self.get_downsample_size(height, width)
        self.default_size = (4 * height, 4 * width)
        vc = self.view_config
        n_rrg = num_inference_steps - int(num_inference_steps * rrg_stop_t)
        if rrg_scherduler_cls is CosineScheduler:
            rrg = CosineScheduler(steps=n_rrg, cosine_scale=cosine_scale, factor=rrg_init_weight)
        else:
            rrg = rrg_scherduler_cls(steps=n_rrg, start_val=rrg_init_weight, stop_val=0)
        if isinstance(prompts, str):
            prompts = [prompts]
        if isinstance(negative_prompts, str):
            negative_prompts = [negative_prompts] * len(prompts)
        un, pun = self.get_text_embeds(negative_prompts)
        co, pco = self.get_text_embeds(prompts)
        text_embeds = torch.cat([un, co])
        add_text_embeds = torch.cat([pun, pco], dim=0)
        s = self.vae_scale_factor
        shape = (len(prompts), self.unet.config.in_channels, height // s, width // s)
        self.scheduler.set_timesteps(num_inference_steps)
        ts = self.scheduler.timesteps
        z0 = noise = m = None
        if init_image is None:
            x = torch.randn(shape, dtype=self.torch_dtype)
        else:
            assert tuple(init_image.shape) == (height, width, 3) and init_image.dtype == np.uint8
            dist = self.vae.encode(to_vae_input(init_image)).latent_dist
            eps_p = torch.randn(shape, dtype=self.torch_dtype)
            noise = torch.randn(shape, dtype=self.torch_dtype)
            a, b = self.add_noise_coefficients(ts[t_start])
            z0, x = init_latent(dist.mean.expand(shape), dist.std.expand(shape), eps_p, noise,
                                self.vae.config.scaling_factor, a, b)
            if mask_image is not None:
                if isinstance(mask_image, torch.Tensor):
                    assert tuple(mask_image.shape) == shape[2:]
                    m = latent_mask(mask_image.to(torch.uint8).numpy(), 1)
                else:
                    assert tuple(mask_image.shape) == (height, width)
                    m = latent_mask(mask_image, s)
        self.last_init_latents, self.last_mask = z0, m
        cn = {}
        if condition_image is not None:
            cn = dict(condition_image=self.prepare_condition(condition_image),
                      controlnet_conditioning_scale=controlnet_conditioning_scale)
        hist = None   # (x0 of the last full-resolution phase of the previous timestep index, its timestep); None at t_start
        for i in progress(range(t_start, len(ts))):
            t = ts[i]
            last = i == len(ts) - 1
            direction, info = self.approximate_latent_direction_w_resampling(
                x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=resampling_steps,
                drop_p=1 - new_p, **cn)
            if logs is not None and logs.get("init_downsampled_latent") is None:
                logs["init_downsampled_latent"] = info["init_downsampled_latent"]
            local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
            out = self.scheduler.step(self.guided(local, direction, guidance_scale), t, x, history=hist, is_last=last)
            x0, nxt, cfg = out["pred_original_sample"], out["prev_sample"], guidance_scale
            if repaint_sampling and resampling_steps > 0 and i < len(ts) - 1:
                if m is not None:
                    nxt = blend(nxt, m, z0, noise, **self.known(z0, noise, ts, i + 1))
                x = self.undo_step(nxt, ts[i + 1])
                cfg = guidance_scale / 3
                direction, info = self.approximate_latent_direction_w_resampling(
                    x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=0, drop_p=1 - new_p, **cn)
                local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
                out = self.scheduler.step(self.guided(local, direction, cfg), t, x, history=hist, is_last=last)  # the SAME history
                x0, nxt = out["pred_original_sample"], out["prev_sample"]
            hist = (x0, t)
            cascade = torch.zeros_like(nxt)
            if rrg(i) > 10:
                cascade, _ = self.reduced_resolution_guidance(
                    t, x0, guidance_scale=cfg, rrg_scale=rrg(i),
                    donwsampled_scores={"latent": info["downsampled_latent"],
                                        "uncond_score": info["scores"]["uncond_score"],
                                        "direction": info["downsampled_direction"]})
            x = nxt + cascade
            if m is not None:
                x = blend(x, m, z0, noise, **self.known(z0, noise, ts, i + 1))
            if trace is not None:
                trace.append(x.clone())
        return x

    def plain_cfg_generate(self, latent, text, pooled, guidance_scale, guidance_rescale=0.0):
        """``generate()``'s plain CFG loop with the previous iteration's x0 as history -> (final latent, [x0 per step])"""
        from tests.guidance_rescale_cpu import rescale_guided
        inter, hist = [], None
        for t in self.scheduler.timesteps:
            uncond, cond = self.unet_step(torch.cat([latent] * 2), t, text, pooled).chunk(2)
            m = uncond + guidance_scale * (cond - uncond)
            if guidance_rescale:
                m = rescale_guided(m, cond, guidance_rescale)
            out = self.scheduler.step(m, t, latent, history=hist)
            hist = (out["pred_original_sample"], t)
            latent = out["prev_sample"]
            inter.append(out["pred_original_sample"])
        return latent, inter


# ---- the four end-to-end cases of tests/golden/g16_dpm_solver.npz (fake UNet / VAE, seed 3, view_batch_size 4, cases.E2E_KW) ----
SEED, VBS = 3, 4
SOLVER_CASES = {
    # epsilon / leading on a padded RePaint geometry: latent 64 x 96, the reduced latent 42 x 64 sits padded in the 64 x 64 model
    "eps_leading_repaint": dict(sched=dict(), sd="1.5", sample=64, H=512, W=768, steps=4, R=3),
    "eps_norepaint": dict(sched=dict(), sd="1.5", sample=64, H=256, W=512, steps=4, R=2, kw=dict(repaint_sampling=False)),
    "v_trailing": dict(sched=dict(prediction_type="v_prediction", timestep_spacing="trailing"), sd="1.5", sample=64,
                       H=512, W=512, steps=5, R=2),
    "controlnet": dict(sched=dict(), sd="1.5", sample=64, H=256, W=512, steps=3, R=2, controlnet=True),
}


def case_kwargs(name):
    """the loop keywords of a case (without the ControlNet condition)"""
    from tests.golden import cases
    c = SOLVER_CASES[name]
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)
    kw.update(c.get("kw", {}))
    return kw


def condition_kwargs(name):
    from oracle.elastic_oracle import get_downsample_size
    from tests.golden import cases
    c = SOLVER_CASES[name]
    if not c.get("controlnet"):
        return {}
    ds = get_downsample_size(c["H"], c["W"], c["sd"])
    return dict(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)


def run_reference_case(name):
    """Drive the REAL reference's generate_image with the first-order restatement injected (needs the reference checkout).
    -> (final latent, torch.rand(4) drawn right after)"""
    from tests.ddim_variants import embed_fn
    from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
    from tests.golden.ref_loader import make_reference_pipeline
    c = SOLVER_CASES[name]
    xl = c["sd"].startswith("XL")
    cn = bool(c.get("controlnet"))
    pipe, ref = make_reference_pipeline(FakeUNet(c["sample"], xl=xl), FakeVAE(), DPMSolverCPU(solver_order=1, **c["sched"]),
                                        embed_fn(xl), sd_version=c["sd"], view_batch_size=VBS,
                                        controlnet=FakeControlNet() if cn else None)
    pipe.random_downasmple_pre = {}
    pipe.seed_everything(SEED)
    cap = {}
    orig = pipe.decode_latents

    def grab(z):
        cap["z"] = z.clone()
        return orig(z)

    pipe.decode_latents = grab
    kw = case_kwargs(name)
    if cn:
        # the reference's prepare_image goes through diffusers' VaeImageProcessor (absent); for a float tensor with do_normalize=False
        # it is the identity (as tests/golden/make_golden.py injects it)
        pipe.control_image_processor = type("P", (), {"preprocess": staticmethod(lambda image, height, width: image)})()
        kw.update(condition_kwargs(name))
    pipe.generate_image(prompts="p", negative_prompts="", progress=lambda it: it, rrg_scherduler_cls=ref.CosineScheduler, **kw)
    return cap["z"], torch.rand(4)


def run_oracle_case(name, solver_order):
    """The same case through SolverOracle at ``solver_order`` -> (final latent, torch.rand(4) tail)"""
    from tests.ddim_variants import embed_fn
    from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
    c = SOLVER_CASES[name]
    xl = c["sd"].startswith("XL")
    orc = SolverOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), DPMSolverCPU(solver_order=solver_order, **c["sched"]),
                       embed_fn(xl), sd_version=c["sd"], view_batch_size=VBS, pooled_dim=16 if xl else None,
                       controlnet=FakeControlNet() if c.get("controlnet") else None)
    orc.seed_everything(SEED)
    z = orc.generate_latent(["p"], "", **case_kwargs(name), **condition_kwargs(name))
    return z, torch.rand(4)
