"""Test-side restatement of the scheduler settings beyond the SD defaults (test infrastructure, never shipped).

``oracle/ddim.py::DDIMOracle`` restates diffusers 0.21.4's ``DDIMScheduler`` for the SD / SDXL default config and
already has the ``v_prediction`` branch of ``step``; it refuses the other two timestep spacings and knows no zero-SNR
rescale.  ``DDIMVariants`` adds exactly those, from diffusers' published definitions, as a
subclass -- it is the scheduler object injected into the real reference (tests/golden/make_scheduler_variants.py) and
into ``ElasticOracle`` when the product's ``DDIMSchedule`` is tested.  It shares no code with
``elasticdiffusion_official_amd/schedule.py``.

PARITY NOTE: as for oracle/ddim.py, "parity unpinned" to diffusers itself (not installed, not installable here); the glue
parity is pinned by driving the real reference with THIS scheduler (tests/golden/g13_scheduler_variants.npz).
"""
import numpy as np
import torch

from oracle.ddim import DDIMOracle


class DDIMVariants(DDIMOracle):
    def __init__(self, rescale_betas_zero_snr=False, **overrides):
        super().__init__(**overrides)
        self.config.rescale_betas_zero_snr = bool(rescale_betas_zero_snr)
        if rescale_betas_zero_snr:  # diffusers' rescale_zero_terminal_snr (Lin et al. 2023, algorithm 1)
            s = self.alphas_cumprod.sqrt()
            s0, sT = s[0].clone(), s[-1].clone()
            s = (s - sT) * (s0 / (s0 - sT))
            abar = s ** 2
            alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
            self.betas = 1 - alphas
            self.alphas = 1.0 - self.betas
            self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
            self.final_alpha_cumprod = torch.tensor(1.0) if self.config.set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, num_inference_steps, device=None):
        n = self.config.num_train_timesteps
        spacing = self.config.timestep_spacing
        if spacing == "leading":
            return super().set_timesteps(num_inference_steps, device)
        if num_inference_steps > n:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        if spacing == "linspace":
            ts = np.linspace(0, n - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif spacing == "trailing":
            ts = np.round(np.arange(n, 0, -n / num_inference_steps)).astype(np.int64) - 1
        else:
            raise NotImplementedError(spacing)
        self.timesteps = torch.from_numpy(ts)


# The six end-to-end fixture cases of tests/golden/g13_scheduler_variants.npz: fake UNet / VAE, seed 3, view_batch_size 4,
# cases.E2E_KW.  ``timesteps`` is what the restatement must produce (asserted by the writer and by the CPU test).
SEED, VBS = 3, 4
VARIANT_CASES = {
    "v_leading": dict(sched=dict(prediction_type="v_prediction"), sd="1.5", sample=64, H=512, W=1024, steps=4, R=3,
                      timesteps=[751, 501, 251, 1]),
    "v_trailing": dict(sched=dict(prediction_type="v_prediction", timestep_spacing="trailing"), sd="1.5", sample=64,
                       H=512, W=1024, steps=4, R=2, timesteps=[999, 749, 499, 249]),
    "v_trailing_zsnr": dict(sched=dict(prediction_type="v_prediction", timestep_spacing="trailing",
                                       rescale_betas_zero_snr=True), sd="1.5", sample=64, H=512, W=768, steps=5, R=2,
                            timesteps=[999, 799, 599, 399, 199]),
    "eps_trailing": dict(sched=dict(timestep_spacing="trailing"), sd="XL1.0", sample=128, H=512, W=1024, steps=4, R=1,
                         timesteps=[999, 749, 499, 249]),
    "eps_linspace": dict(sched=dict(timestep_spacing="linspace"), sd="1.5", sample=64, H=512, W=768, steps=4, R=2,
                         timesteps=[999, 666, 333, 0]),
    "v_trailing_7": dict(sched=dict(prediction_type="v_prediction", timestep_spacing="trailing"), sd="1.5", sample=64,
                         H=512, W=768, steps=7, R=1, timesteps=[999, 856, 713, 570, 428, 285, 142]),
}


def embed_fn(xl, B=1):
    """The alternating (negative, positive) synthetic text embeddings the end-to-end tests use."""
    from tests.fakes import synthetic_text_embeds
    (un, pun), (co, pco) = synthetic_text_embeds(B, xl=xl)
    state = {"n": 0}

    def fn(_):
        state["n"] += 1
        return (un, pun) if state["n"] % 2 == 1 else (co, pco)

    return fn


def run_reference_case(name):
    """Drive the REAL reference's generate_image with the variant scheduler injected (needs the reference checkout).
    -> (final latent, torch.rand(4) drawn right after, the timesteps the scheduler produced)"""
    from tests.fakes import FakeUNet, FakeVAE
    from tests.golden import cases
    from tests.golden.ref_loader import make_reference_pipeline
    c = VARIANT_CASES[name]
    xl = c["sd"].startswith("XL")
    pipe, ref = make_reference_pipeline(FakeUNet(c["sample"], xl=xl), FakeVAE(), DDIMVariants(**c["sched"]), embed_fn(xl),
                                        sd_version=c["sd"], view_batch_size=VBS)
    pipe.random_downasmple_pre = {}
    pipe.seed_everything(SEED)
    cap = {}
    orig = pipe.decode_latents

    def grab(z):
        cap["z"] = z.clone()
        return orig(z)

    pipe.decode_latents = grab
    pipe.generate_image(prompts="p", negative_prompts="", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                        resampling_steps=c["R"], progress=lambda it: it, rrg_scherduler_cls=ref.CosineScheduler,
                        **cases.E2E_KW)
    tail = torch.rand(4)
    return cap["z"], tail, pipe.scheduler.timesteps.tolist()


def run_oracle_case(name):
    """The same case through ElasticOracle -> (final latent, torch.rand(4) tail)."""
    from oracle.elastic_oracle import ElasticOracle
    from tests.fakes import FakeUNet, FakeVAE
    from tests.golden import cases
    c = VARIANT_CASES[name]
    xl = c["sd"].startswith("XL")
    orc = ElasticOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), DDIMVariants(**c["sched"]), embed_fn(xl),
                        sd_version=c["sd"], view_batch_size=VBS, pooled_dim=16 if xl else None)
    orc.seed_everything(SEED)
    z = orc.generate_latent(["p"], "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                            resampling_steps=c["R"], **cases.E2E_KW)
    return z, torch.rand(4)
