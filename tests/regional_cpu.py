"""Test-side specification of regional prompts (test infrastructure, never shipped; torch and Pillow on the CPU).

DESIGN.md section 28 in code.  A run carries a base prompt (the ordinary ``prompts`` argument) and n regions, 1 <= n <= 7, each a
prompt, a mask and a weight > 0; P = n + 1 conditional rows per resampling step and sample.

Masks (``latent_mask``).  A box (x0, y0, x1, y1) in pixels is a 255 rectangle at the picture's size; a picture mask is an 8-bit
image at the picture's size; either is optionally feathered with ``PIL.ImageFilter.GaussianBlur(region_blur)`` and then reduced to
the latent grid with ``Image.resize(BILINEAR)``.  A uint8 array already at the latent size is used as is.

Weights (``region_weights``), fp32, every operation rounded on its own:
    r_p = weight_p * (m_p / 255)  (p = 1..n),   s = r_1 + .. + r_n in order,   r_0 = max(0, 1 - s),   tot = r_0 + s,   w_p = r_p / tot

Direction (``blend``).  With u the unconditional row and c_p the conditional rows of a pixel's covering resampling step,
    d = sum_p w_p * (c_p - u)
where a term whose weight is 0 is skipped (its row is never read, so a NaN there does not spread), the first term that is not
skipped starts the sum and the later ones are added in order of p; d = 0 where every weight is 0.  With one-hot weights d is that
region's own c_p - u bit for bit.  Everything downstream of d is unchanged.

``RegionalOracle`` places this in the ElasticDiffusion loop on top of ``tests/dpm_solver_cpu.py::SolverOracle`` (which carries the
DDIM / v-prediction / guidance-rescale / DPM-Solver++ restatements): ``obtain_latent_direction`` evaluates one model batch of
1 + P rows per sample and returns the P directions stacked on the channel axis, the oracle's own gathers carry them to full
resolution, and they are blended there (and, for the reduced-resolution guidance, at the nearest-downsample points with the
weights sampled at the same points).  No RNG draw depends on the regions.

It shares no code with elasticdiffusion_official_amd/.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.dpm_solver_cpu import SolverOracle

MAX_REGIONS = 7


# ---- masks ------------------------------------------------------------------------------------------------------------------
def box_mask(box, height, width):
    """(x0, y0, x1, y1) in pixels, x1 / y1 exclusive -> uint8 [height, width], 255 inside"""
    x0, y0, x1, y1 = box
    m = np.zeros((height, width), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def latent_mask(mask, height, width, scale=8, region_blur=0.0):
    """one region's mask -> uint8 [height // scale, width // scale] (numpy)"""
    from PIL import Image, ImageFilter
    Hl, Wl = height // scale, width // scale
    if isinstance(mask, (tuple, list)):
        mask = box_mask(mask, height, width)
    elif hasattr(mask, "convert"):
        mask = np.array(mask.convert("L"))
    elif isinstance(mask, torch.Tensor):
        mask = mask.cpu().numpy()
    mask = np.ascontiguousarray(mask).reshape(mask.shape[0], mask.shape[1])
    assert mask.dtype == np.uint8
    if mask.shape == (Hl, Wl):
        return mask
    if mask.shape != (height, width):
        raise ValueError(f"mask is {mask.shape}; it must be {(height, width)} or {(Hl, Wl)}")
    img = Image.fromarray(mask)
    if region_blur > 0:
        img = img.filter(ImageFilter.GaussianBlur(region_blur))
    return np.array(img.resize((Wl, Hl), resample=Image.BILINEAR))


# ---- weights ------------------------------------------------------------------------------------------------------------------
def region_weights(masks, weights):
    """masks uint8 [n, Hl, Wl], n weights > 0 -> f32 [n + 1, Hl, Wl], plane 0 the base prompt's"""
    masks = torch.as_tensor(np.asarray(masks) if not isinstance(masks, torch.Tensor) else masks)
    n = masks.shape[0]
    assert masks.dtype == torch.uint8 and 1 <= n <= MAX_REGIONS and len(weights) == n and all(float(v) > 0 for v in weights)
    m = masks.to(torch.float32)
    c255 = torch.full_like(m[0], 255.0)
    r = [torch.full_like(m[0], float(np.float32(weights[p]))) * (m[p] / c255) for p in range(n)]
    s = r[0]
    for p in range(1, n):
        s = s + r[p]
    r0 = torch.maximum(torch.zeros_like(s), torch.ones_like(s) - s)
    tot = r0 + s
    return torch.stack([r0 / tot] + [rp / tot for rp in r])


# ---- direction ------------------------------------------------------------------------------------------------------------------
def blend(dirs, w):
    """dirs f32 [P, B, C, H, W] (the P directions c_p - u), w f32 [P, H, W] -> f32 [B, C, H, W]"""
    P = dirs.shape[0]
    assert tuple(w.shape) == (P,) + tuple(dirs.shape[-2:])
    d = torch.zeros_like(dirs[0])
    started = torch.zeros(w.shape[1:], dtype=torch.bool)
    for p in range(P):
        on = w[p] != 0
        term = w[p] * dirs[p]
        d = torch.where(on & started, d + term, torch.where(on, term, d))
        started = started | on
    return d


# ---- prompts ------------------------------------------------------------------------------------------------------------------
def prompt_embeds(xl=False, cross_dim=32, pooled_dim=16):
    """A stateless text encoder keyed by the prompt string: "" and "p" are the two embeddings the other end-to-end tests alternate
    between (tests/fakes.py::synthetic_text_embeds), any other string a fixed pseudo-random embedding of its own."""
    from tests.fakes import synthetic_text_embeds
    (un, pun), (co, pco) = synthetic_text_embeds(1, cross_dim, pooled_dim, xl=xl)

    def one(p):
        if p == "":
            return un, pun
        if p == "p":
            return co, pco
        g = torch.Generator().manual_seed(int(hashlib.md5(p.encode()).hexdigest()[:8], 16))
        e = torch.randn(1, 77, cross_dim, generator=g)
        return e, (torch.randn(1, pooled_dim, generator=g) if xl else e)

    def fn(prompts):
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        pairs = [one(p) for p in prompts]
        return torch.cat([e for e, _ in pairs]), torch.cat([q for _, q in pairs])

    return fn


# ---- the loop -----------------------------------------------------------------------------------------------------------------
class RegionalOracle(SolverOracle):
    """``SolverOracle`` with ``regions=[(prompt, mask[, weight]), ...]`` / ``region_blur``; without them every expression is the
    parent's.  ``get_text_embeds`` must be stateless (``prompt_embeds``)."""
    _region = None  # (region_w f32 [P,Hl,Wl], [cond embeddings of the n regions], [their pooled embeddings])

    def obtain_latent_direction(self, latent, t, text_embeds, add_text_embeds, **cn):
        if self._region is None:
            return super().obtain_latent_direction(latent, t, text_embeds, add_text_embeds, **cn)
        _, cos, pcos = self._region
        B = latent.shape[0]
        P = 1 + len(cos)
        text = torch.cat([text_embeds] + cos)            # [uncond, base cond, region conds], each x B
        pooled = torch.cat([add_text_embeds] + pcos)
        if "condition_image" in cn:                      # one condition row per model row (the reference doubles it for its pair)
            cn = dict(cn, condition_image=cn["condition_image"][:1].repeat((1 + P) * B, 1, 1, 1))
        rows = self.unet_step(torch.cat([latent] * (1 + P)), t, text, pooled, **cn).chunk(1 + P)
        uncond = rows[0]
        return torch.cat([c - uncond for c in rows[1:]], dim=1), {"uncond_score": uncond, "cond_score": rows[1]}

    def approximate_latent_direction_w_resampling(self, latent, t, text_embeds, add_text_embeds, downsample_size,
                                                  resampling_steps=6, drop_p=0.7, **cn):
        if self._region is None:
            return super().approximate_latent_direction_w_resampling(latent, t, text_embeds, add_text_embeds, downsample_size,
                                                                     resampling_steps=resampling_steps, drop_p=drop_p, **cn)
        w = self._region[0]
        P = w.shape[0]
        B, C, H, W = latent.shape
        # the parent's loop on a target of P * C channels: picks, masks and fills are per pixel, so the channels ride along
        target = torch.full((B, P * C, H, W), float("nan")).half()
        exclude, prev, info = None, None, {"init_downsampled_latent": None}
        for step in range(resampling_steps + 1):
            low, mask, prev = self.random_nearest_downsample(latent, downsample_size, prev_random_indices=prev,
                                                             exclude_mask=exclude, drop_p=drop_p, nearest=(step == 0))
            if exclude is None:
                exclude = torch.zeros(len(prev), 4, dtype=torch.bool)
            exclude[torch.arange(len(prev)), prev] = True
            if info["init_downsampled_latent"] is None:
                info["init_downsampled_latent"] = low.clone()
            direction, scores = self.obtain_latent_direction(low, t, text_embeds, add_text_embeds, **cn)
            target = self.fill_in_from_downsampled_direction(target, direction, mask, fill_all=(step == resampling_steps))
        info["downsampled_latent"] = low
        info["scores"] = scores
        low_stack = F.interpolate(target, size=downsample_size, mode="nearest")
        w_low = F.interpolate(w[None], size=downsample_size, mode="nearest")[0]
        h, w_ = downsample_size
        info["downsampled_direction"] = blend(low_stack.view(B, P, C, h, w_).transpose(0, 1), w_low)
        return blend(target.view(B, P, C, H, W).transpose(0, 1), w), info

    @torch.no_grad()
    def generate_latent(self, prompts, negative_prompts="", regions=None, region_blur=0.0, **kw):
        self._region = None
        self.last_region_weights = None
        if regions:
            if not 1 <= len(regions) <= MAX_REGIONS:
                raise ValueError(f"1 to {MAX_REGIONS} regions, got {len(regions)}")
            B = 1 if isinstance(prompts, str) else len(prompts)
            H, W = kw.get("height", 768), kw.get("width", 768)
            masks = np.stack([latent_mask(r[1], H, W, self.vae_scale_factor, region_blur) for r in regions])
            w = region_weights(torch.from_numpy(masks), [r[2] if len(r) == 3 else 1.0 for r in regions])
            embeds = [self.get_text_embeds([r[0]] * B) for r in regions]
            self._region = (w, [e for e, _ in embeds], [q for _, q in embeds])
            self.last_region_weights = w
        try:
            return super().generate_latent(prompts, negative_prompts, **kw)
        finally:
            self._region = None
