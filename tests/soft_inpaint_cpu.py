"""Test-side restatement of soft-edged inpainting (test infrastructure, never shipped; numpy / torch on the CPU).

DESIGN.md section 19: the Gaussian blur of an 8-bit mask with Pillow's bytes (``ImageFilter.GaussianBlur`` on an ``L`` image:
three integer box-blur passes per direction), graded masks (a latent pixel of level L is held to the known region while
``L <= thr(j)``), ``Image.composite`` fused with the float -> 8-bit conversion, and the edge-replicated outpainting canvas.
The functions below are what the HIP kernels are compared with bit for bit; ``SoftInpaintOracle`` is the loop of
``tests/img2img_cpu.py::Img2ImgOracle`` with the per-step level test.

It shares no code with elasticdiffusion_official_amd/.
"""
import math

import numpy as np
import torch

from oracle.elastic_oracle import CosineScheduler
from tests import img2img_cpu as I


# ---- Gaussian blur, Pillow's bytes ------------------------------------------------------------------------------------
def box_parameters(radius):
    """``ImageFilter.GaussianBlur(radius)`` -> (r, ww, fw) of each of its three box passes: the integer box radius, the
    24-bit fixed-point weight of a pixel inside the box and of the two pixels at its fractional edge."""
    sigma2 = float(radius) * float(radius) / 3
    Lw = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((Lw - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)))
    fr = np.float32(l + a)
    r = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / (np.float32(2) * fr + np.float32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass_rows(img, r, ww, fw):
    """one box pass along the rows of a uint8 [H,W] array -> uint8 [H,W]; indices clamp to the line"""
    H, W = img.shape
    src = img.astype(np.uint32)
    x = np.arange(W)
    acc = np.zeros((H, W), np.uint32)
    for d in range(-r, r + 1):
        acc += src[:, np.clip(x + d, 0, W - 1)]
    far = src[:, np.clip(x - r - 1, 0, W - 1)] + src[:, np.clip(x + r + 1, 0, W - 1)]
    out = (acc * np.uint32(ww) + far * np.uint32(fw) + np.uint32(1 << 23)) >> np.uint32(24)
    assert int(out.max(initial=0)) <= 255
    return out.astype(np.uint8)


def gaussian_blur(img, radius):
    """uint8 [H,W] numpy -> uint8 [H,W]: three passes along the rows, three along the columns, each on the previous one's bytes"""
    r, ww, fw = box_parameters(radius)
    out = np.ascontiguousarray(img)
    for _ in range(3):
        out = box_pass_rows(out, r, ww, fw)
    out = np.ascontiguousarray(out.T)
    for _ in range(3):
        out = box_pass_rows(out, r, ww, fw)
    return np.ascontiguousarray(out.T)


# ---- compositing ------------------------------------------------------------------------------------------------------
def to_bytes(decoded):
    """float [..] in [0,1] -> uint8: the fp32 product with 255, truncated (``imgs.mul(255).byte()``)"""
    return (decoded.float() * 255).to(torch.uint8)


def composite_bytes(u, init, m):
    """``Image.composite(u, init, m)`` per byte on integer arrays: u where m = 255, init where m = 0"""
    u, init, m = (np.asarray(v).astype(np.uint32) for v in (u, init, m))
    t = u * m + init * (255 - m) + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def composite(decoded, init, mask):
    """decoded f32 (1,3,H,W) tensor in [0,1], init uint8 [H,W,3], mask uint8 [H,W] (numpy) -> uint8 [H,W,3] numpy"""
    u = to_bytes(decoded)[0].permute(1, 2, 0).numpy()
    return composite_bytes(u, init, np.asarray(mask)[:, :, None])


# ---- outpainting canvas -----------------------------------------------------------------------------------------------
def canvas_pad(img, left, top, right, bottom):
    """uint8 [H,W,3] -> (canvas [H',W',3] with the border replicated from the edge, mask [H',W']: 255 on the border, 0 inside)"""
    H, W = img.shape[:2]
    ys = np.clip(np.arange(-top, H + bottom), 0, H - 1)
    xs = np.clip(np.arange(-left, W + right), 0, W - 1)
    mask = np.full((H + top + bottom, W + left + right), 255, np.uint8)
    mask[top:top + H, left:left + W] = 0
    return img[ys][:, xs], mask


# ---- graded masks -----------------------------------------------------------------------------------------------------
def thr(j, T):
    """a latent pixel of level L is held to the known region at target index j iff L <= thr(j)"""
    return (255 * (T - j)) // T


def level_map(u8, s):
    """uint8 [H,W] numpy -> uint8 (H // s, W // s) tensor: the byte at the top-left pixel of every latent cell"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(u8)[::s, ::s]))


def blend_level(x, level, t, z0, noise, a, b, clean):
    """where(level > t, x, known): ``img2img_cpu.blend`` with the level test in place of the mask byte"""
    return I.blend(x, (level > t).to(torch.uint8), z0, noise, a, b, clean)


class SoftInpaintOracle(I.Img2ImgOracle):
    """The loop of ``Img2ImgOracle`` with ``mask_blur`` / ``mask_mode``.  ``mask_image``: uint8 [height, width] numpy (blurred
    first when ``mask_blur`` > 0), or a (Hl, Wl) tensor -- uint8: the level map itself in graded mode; bool: 0 / 255.
    ``last_pixel_mask`` keeps the (blurred) pixel mask, ``last_levels`` the level map of a graded run.  Binary mode is the
    parent's ``generate_latent`` on the blurred bytes."""
    last_pixel_mask = None
    last_levels = None

    @torch.no_grad()
    def generate_latent(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                        guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                        rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                        progress=lambda it: it, condition_image=None, controlnet_conditioning_scale=1.0,
                        trace=None, logs=None, guidance_rescale=0.0, init_image=None, strength=1.0, mask_image=None,
                        mask_blur=0.0, mask_mode="binary"):
        if mask_mode not in ("binary", "graded"):
            raise ValueError(f"mask_mode must be 'binary' or 'graded', got {mask_mode!r}")
        if mask_image is None and (mask_blur or mask_mode != "binary"):
            raise ValueError("mask_blur / mask_mode need mask_image")
        self.last_pixel_mask = self.last_levels = None
        if isinstance(mask_image, np.ndarray):
            if mask_blur:
                mask_image = gaussian_blur(mask_image, mask_blur)
            self.last_pixel_mask = mask_image
        elif mask_blur:
            raise ValueError("mask_blur needs a picture mask")
        if mask_mode == "binary":
            return super().generate_latent(
                prompts, negative_prompts, height, width, num_inference_steps, guidance_scale, resampling_steps, new_p,
                rrg_stop_t, rrg_init_weight, rrg_scherduler_cls, cosine_scale, repaint_sampling, progress, condition_image,
                controlnet_conditioning_scale, trace, logs, guidance_rescale, init_image, strength, mask_image)
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
        t_start = I.window(num_inference_steps, strength)
        if init_image is None:
            raise ValueError("mask_image needs init_image")
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
        T = len(ts)
        assert tuple(init_image.shape) == (height, width, 3) and init_image.dtype == np.uint8
        dist = self.vae.encode(I.to_vae_input(init_image)).latent_dist
        eps_p = torch.randn(shape, dtype=self.torch_dtype)      # the posterior's noise first ...
        noise = torch.randn(shape, dtype=self.torch_dtype)      # ... then the initial noise; graded masks draw nothing more
        a, b = self.add_noise_coefficients(ts[t_start])
        z0, x = I.init_latent(dist.mean.expand(shape), dist.std.expand(shape), eps_p, noise, self.vae.config.scaling_factor, a, b)
        if isinstance(mask_image, torch.Tensor):
            assert tuple(mask_image.shape) == shape[2:]
            level = mask_image.to(torch.uint8) * 255 if mask_image.dtype == torch.bool else mask_image.clone()
        else:
            assert tuple(mask_image.shape) == (height, width)
            level = level_map(mask_image, s)
        self.last_init_latents, self.last_mask, self.last_levels = z0, None, level

        def held(xx, j):       # the level test at target index j, absolute like every other index of the loop
            return blend_level(xx, level, thr(j, T), z0, noise, **self.known(z0, noise, ts, j))

        cn = {}
        if condition_image is not None:
            cn = dict(condition_image=self.prepare_condition(condition_image),
                      controlnet_conditioning_scale=controlnet_conditioning_scale)
        for i in progress(range(t_start, T)):
            t = ts[i]
            direction, info = self.approximate_latent_direction_w_resampling(
                x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=resampling_steps,
                drop_p=1 - new_p, **cn)
            if logs is not None and logs.get("init_downsampled_latent") is None:
                logs["init_downsampled_latent"] = info["init_downsampled_latent"]
            local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
            out = self.scheduler.step(self.guided(local, direction, guidance_scale), t, x)
            x0, nxt, cfg = out["pred_original_sample"], out["prev_sample"], guidance_scale
            if repaint_sampling and resampling_steps > 0 and i < T - 1:
                nxt = held(nxt, i + 1)
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
            x = held(nxt + cascade, i + 1)
            if trace is not None:
                trace.append(x.clone())
        return x
