"""Test-side restatement of image-to-image and masked inpainting (test infrastructure, never shipped; torch on the CPU).

The semantics are DESIGN.md section 18: diffusers' ``StableDiffusionImg2ImgPipeline`` (``get_timesteps``, ``VaeImageProcessor``'s
normalisation, ``latent_dist.sample() * scaling_factor``, ``scheduler.add_noise``) and the 4-channel-UNet branch of
``StableDiffusionInpaintPipeline`` (the kept region re-noised with the SAME initial noise and put back after every step), placed in
the ElasticDiffusion loop.  ``diffusers`` is not installed here, so the five rules are written out from its published formulas, as
oracle/ddim.py does for the scheduler.  The functions below are what the HIP kernels are compared with bit for bit;
``Img2ImgOracle`` is the loop of ``tests/guidance_rescale_cpu.py::RescaleOracle`` with them.

It shares no code with elasticdiffusion_official_amd/.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.elastic_oracle import CosineScheduler
from tests.guidance_rescale_cpu import RescaleOracle


def window(T, strength):
    """diffusers ``get_timesteps``: -> t_start, the index of the first timestep that runs."""
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength!r}")
    n = min(int(T * strength), T)
    if n < 1:
        raise ValueError(f"strength {strength!r} leaves no step of {T}")
    return max(T - n, 0)


def to_vae_input(u8, dtype=torch.float32):
    """uint8 [H,W,3] numpy -> (1,3,H,W) ``dtype``: ``np.float32(v) / 255`` (VaeImageProcessor.pil_to_numpy), then
    ``2 * x - 1`` (normalize), HWC -> NCHW."""
    x = torch.from_numpy(np.float32(u8) / 255)
    x = 2 * x - 1
    return x.permute(2, 0, 1)[None].contiguous().to(dtype)


def init_latent(mean, std, eps_p, noise, sf, a, b):
    """-> (z0, x): the sampled, scaled posterior and its noised version; mean / std in any float dtype, the rest fp32"""
    z0 = (mean.float() + std.float() * eps_p) * sf
    return z0, a * z0 + b * noise


def latent_mask(u8, s):
    """uint8 [H,W] numpy (255 = repaint) -> uint8 (H // s, W // s) tensor: the mask binarised at 0.5, then torch's nearest
    ``interpolate`` to the latent size.  ``s == 1``: a mask that is already at latent resolution, non-zero = repaint."""
    m = torch.from_numpy(np.ascontiguousarray(u8))
    if s == 1:
        return (m != 0).to(torch.uint8)
    m = (m.float() / 255 >= 0.5).float()[None, None]
    return F.interpolate(m, size=(u8.shape[0] // s, u8.shape[1] // s), mode="nearest")[0, 0].to(torch.uint8)


def blend(x, m, z0, noise, a, b, clean):
    """where(m, x, known): known = a * z0 + b * noise, or a copy of z0 after the last timestep (``clean``)"""
    known = z0.clone() if clean else a * z0 + b * noise
    return torch.where(m.bool(), x, known)


class Img2ImgOracle(RescaleOracle):
    """``init_image``: uint8 [height, width, 3] numpy (already at the run's size); ``mask_image``: uint8 [height, width] numpy
    or a (Hl, Wl) uint8 / bool tensor.  ``last_init_latents`` / ``last_mask`` keep z0 and the latent mask of the last run."""
    last_init_latents = None
    last_mask = None

    def add_noise_coefficients(self, t):
        ac = self.scheduler.alphas_cumprod[int(t)]
        return ac ** 0.5, (1 - ac) ** 0.5

    def known(self, z0, noise, ts, j):
        """the kept region at the noise level of timestep index j (the clean latent after the last one)"""
        if j >= len(ts):
            return dict(a=1.0, b=0.0, clean=True)
        a, b = self.add_noise_coefficients(ts[j])
        return dict(a=a, b=b, clean=False)

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
            eps_p = torch.randn(shape, dtype=self.torch_dtype)      # the posterior's noise first ...
            noise = torch.randn(shape, dtype=self.torch_dtype)      # ... then the initial noise
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
        for i in progress(range(t_start, len(ts))):     # the ABSOLUTE index: coefficients, pad frames, rrg(i), i < T - 1
            t = ts[i]
            direction, info = self.approximate_latent_direction_w_resampling(
                x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=resampling_steps,
                drop_p=1 - new_p, **cn)
            if logs is not None and logs.get("init_downsampled_latent") is None:
                logs["init_downsampled_latent"] = info["init_downsampled_latent"]
            local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
            out = self.scheduler.step(self.guided(local, direction, guidance_scale), t, x)
            x0, nxt, cfg = out["pred_original_sample"], out["prev_sample"], guidance_scale
            if repaint_sampling and resampling_steps > 0 and i < len(ts) - 1:
                if m is not None:       # the re-noised latent carries the known region into the second phase
                    nxt = blend(nxt, m, z0, noise, **self.known(z0, noise, ts, i + 1))
                x = self.undo_step(nxt, ts[i + 1])
                cfg = guidance_scale / 3
                direction, info = self.approximate_latent_direction_w_resampling(
                    x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=0, drop_p=1 - new_p, **cn)
                local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
                out = self.scheduler.step(self.guided(local, direction, cfg), t, x)
                x0, nxt = out["pred_original_sample"], out["prev_sample"]
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
