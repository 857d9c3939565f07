"""Test-side restatement of inpainting with a 9-channel UNet (test infrastructure, never shipped; torch on the CPU).

The semantics are DESIGN.md section 22: the ``num_channels_unet == 9`` branch of diffusers 0.21.4 ``StableDiffusionInpaintPipeline``
(``prepare_mask_and_masked_image``: ``masked_image = image * (mask < 0.5)`` on the binarised mask; ``prepare_mask_latents``: the mask
interpolated to the latent size, the masked image encoded, sampled and scaled; ``latent_model_input = cat([latents, mask,
masked_image_latents], dim=1)``; no paste-back of the known region) placed in the ElasticDiffusion loop: every model row -- a randomly
picked reduced latent, a context crop -- carries the extra five channels sampled at the very latent pixels its first four were.
``diffusers`` is not installed here, so the rules are written out from its published source, as tests/img2img_cpu.py does.

It shares no code with elasticdiffusion_official_amd/.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.elastic_oracle import CosineScheduler, crop_with_context
from tests.fakes import FakeUNet
from tests.img2img_cpu import Img2ImgOracle, init_latent, latent_mask, to_vae_input, window

LATENT_CHANNELS = 4
PAD_MASK, PAD_MASKED_LATENT = 1.0, 0.0     # the extras in the pad strips (discarded with them): a choice, DESIGN.md section 22.7


def to_vae_input_masked(u8, mask_u8, dtype=torch.float32, threshold=128):
    """uint8 [H,W,3] and uint8 [H,W] numpy -> (1,3,H,W): ``vae_input * (mask / 255 < 0.5)``, i.e. the pixel where the mask byte is
    below 128 and zero elsewhere -- +0.0 (the product of a negative pixel and 0.0 would be -0.0; the specification selects)"""
    x = to_vae_input(u8, torch.float32)
    hole = torch.from_numpy(np.ascontiguousarray(mask_u8) >= threshold)[None, None].expand_as(x)
    return torch.where(hole, torch.zeros((), dtype=torch.float32), x).to(dtype)


def masked_latent(mean, std, eps_m, sf):
    """zm = (mean + std * eps_m) * sf: ``latent_dist.sample() * scaling_factor`` with the draw made explicit"""
    return (mean.float() + std.float() * eps_m) * sf


def assemble_rows_x(latent, idx, src_row, src_col, h, w, gpad, gframe, win_y0, win_x0, Sh, Sw, vpad, vframe, extra, pad_value, dtype):
    """The model rows of one phase, written as plain gathers -> (g_rows [(K*2*B),C+E,gPH,gPW], v_rows [(V*B),C+E,vPH,vPW],
    low [K,B,C,h,w]).  latent f32 [B,C,H,W], extra f32 [B,E,H,W], idx uint8 [K,h*w] (the pick q of every reduced pixel: source
    row ``src_row[2 i + q // 2]``, column ``src_col[2 j + q % 2]``), ``gpad`` / ``vpad`` = (PH, PW, top, left), frames f32
    [C,PH,PW] or None (zeros), windows ``latent[..., y0:y0+Sh, x0:x0+Sw]``.  The extra channels take the SAME source pixel as the
    latent channels of their row, and ``pad_value[e]`` where the latent takes the frame."""
    B, C = latent.shape[:2]
    E = extra.shape[1]
    K = idx.shape[0]
    both = torch.cat([latent, extra], dim=1)
    sr, sc = torch.as_tensor(src_row).long(), torch.as_tensor(src_col).long()

    def blank(n, PH, PW, frame):
        rows = torch.zeros(n, C + E, PH, PW)
        if frame is not None:
            rows[:, :C] = frame
        rows[:, C:] = torch.as_tensor(pad_value, dtype=torch.float32).view(1, E, 1, 1)
        return rows

    PH, PW, top, left = gpad
    g_rows = blank(K * 2 * B, PH, PW, gframe).view(K, 2, B, C + E, PH, PW)
    low = torch.empty(K, B, C, h, w)
    q = idx.view(K, h, w).long()
    for k in range(K):
        sy = sr[2 * torch.arange(h).view(-1, 1) + q[k] // 2]
        sx = sc[2 * torch.arange(w).view(1, -1) + q[k] % 2]
        picked = both[:, :, sy, sx]                                   # [B,C+E,h,w]
        low[k] = picked[:, :C]
        g_rows[k, :, :, :, top:top + h, left:left + w] = picked       # the unconditional and the conditional row alike
    PH, PW, top, left = vpad
    V = len(win_y0)
    v_rows = blank(V * B, PH, PW, vframe).view(V, B, C + E, PH, PW)
    for v in range(V):
        y0, x0 = int(win_y0[v]), int(win_x0[v])
        v_rows[v, :, :, top:top + Sh, left:left + Sw] = both[:, :, y0:y0 + Sh, x0:x0 + Sw]
    return g_rows.view(K * 2 * B, C + E, *gpad[:2]).to(dtype), v_rows.view(V * B, C + E, *vpad[:2]).to(dtype), low


class _Out(dict):
    __getattr__ = dict.__getitem__


class FakeUNet9(FakeUNet):
    """``FakeUNet`` on the first four channels plus a fixed 1x1 linear function of channels 4..8 (``extras_weight`` = 0: the
    extras are ignored and the model is ``FakeUNet``).  Records the rows it is given when ``record`` is a list."""

    def __init__(self, sample_size=64, extras_weight=0.05, **kw):
        super().__init__(sample_size, **kw)
        self.config.in_channels, self.config.out_channels = 9, LATENT_CHANNELS
        g = torch.Generator().manual_seed(91)
        self.register_buffer("mix", torch.randn(LATENT_CHANNELS, 5, generator=g) * extras_weight)
        self.record = None

    def forward(self, x, t, **kw):
        assert x.shape[1] == 9, x.shape
        if self.record is not None:
            self.record.append(x.detach().clone())
        y = super().forward(x[:, :LATENT_CHANNELS], t, **kw)["sample"]
        y = y + torch.einsum("oe,nehw->nohw", self.mix.to(x.dtype), x[:, LATENT_CHANNELS:])
        return _Out(sample=y)


class Inpaint9Oracle(Img2ImgOracle):
    """``init_image`` uint8 [height, width, 3] numpy, ``mask_image`` uint8 [height, width] numpy (255 = repaint), both required;
    ``latent_mask_image``: the (blurred) picture the LATENT mask is sampled from when it differs from ``mask_image`` -- the
    picture is always blanked through ``mask_image`` itself.  ``last_masked_image_latents`` keeps zm."""
    last_masked_image_latents = None
    _extras = None
    _low_extras = None

    def make_extras(self, m, zm, batch):
        """-> [batch, 5, Hl, Wl]: the latent mask as 0.0 / 1.0, then zm, one set broadcast over the prompts"""
        return torch.cat([m.float()[None, None], zm], dim=1).expand(batch, -1, -1, -1).contiguous()

    # ---- the model boundary: rows are cat([latent part, extras registered to it]) -------------------------------------------
    def unet_step(self, latent, t, text_embeds, add_text_embeds, condition_image=None, controlnet_conditioning_scale=1.0):
        assert condition_image is None and latent.shape[1] == LATENT_CHANNELS + 5
        xl = self.sd_version.startswith("XL")
        d = 128 if xl else 64
        lat, ext = latent[:, :LATENT_CHANNELS], latent[:, LATENT_CHANNELS:]
        lat = self.scheduler.scale_model_input(lat, t)
        h_p, w_p = max(d - lat.shape[-2], 0), max(d - lat.shape[-1], 0)
        l_p, t_p = w_p // 2, h_p // 2
        r_p, b_p = w_p - l_p, h_p - t_p
        if h_p or w_p:
            lat = self.background_pad(lat, (l_p, r_p, t_p, b_p), t)
            ext = torch.cat([F.pad(ext[:, :1], (l_p, r_p, t_p, b_p), value=PAD_MASK),
                             F.pad(ext[:, 1:], (l_p, r_p, t_p, b_p), value=PAD_MASKED_LATENT)], dim=1)
        x = torch.cat([lat, ext], dim=1)
        kw = {}
        if xl:
            ids = self._add_time_ids(text_embeds.dtype).repeat(x.shape[0], 1)
            kw["added_cond_kwargs"] = {"text_embeds": add_text_embeds, "time_ids": ids}
        y = self.unet(x, t, encoder_hidden_states=text_embeds, **kw)["sample"]
        if h_p or w_p:
            y = y[:, :, t_p: y.shape[-2] - b_p, l_p: y.shape[-1] - r_p]
        return y

    def random_nearest_downsample(self, x, downsample_size, **kw):
        """the pick applied to the latent and the extras together: the extras of a reduced pixel come from the latent pixel it
        was picked from (the draws do not depend on the channel count)"""
        low9, mask, idx = super().random_nearest_downsample(torch.cat([x, self._extras], dim=1), downsample_size, **kw)
        self._low_extras = low9[:, LATENT_CHANNELS:]
        return low9[:, :LATENT_CHANNELS].contiguous(), mask, idx

    def obtain_latent_direction(self, latent, t, text_embeds, add_text_embeds, **cn):
        row = torch.cat([latent, self._low_extras], dim=1)          # identical extras in the unconditional and conditional row
        uncond, cond = self.unet_step(torch.cat([row, row]), t, text_embeds, add_text_embeds).chunk(2)
        return cond - uncond, {"uncond_score": uncond, "cond_score": cond}

    def compute_local_uncond_signal(self, latent, t, uncond_text_embeds, negative_pooled, view_config, **cn):
        assert not cn
        Hl, Wl = latent.shape[-2:]
        s = self.vae_scale_factor
        ws, ctx = view_config["window_size"], view_config["context_size"]
        h_ws = Hl if ws + ctx >= Hl else ws
        w_ws = Wl if ws + ctx >= Wl else ws
        views = self.get_views(Hl * s, Wl * s, h_ws=h_ws, w_ws=w_ws, stride=view_config["stride"])
        out = torch.zeros_like(latent)
        both = torch.cat([latent, self._extras], dim=1)
        for b0 in range(0, len(views), self.view_batch_size):
            batch = views[b0:b0 + self.view_batch_size]
            crops, ctxs = [], []
            for (h0, h1, w0, w1) in batch:
                crop, n4 = crop_with_context(both, h0, h1, w0, w1, 1, ctx // 2)     # the same window for all nine channels
                crops.append(crop)
                ctxs.append(n4)
            pred = self.unet_step(torch.cat(crops), t, torch.cat([uncond_text_embeds] * len(batch)),
                                  torch.cat([negative_pooled] * len(batch)))
            for (h0, h1, w0, w1), (n_t, n_b, n_l, n_r), p in zip(batch, ctxs, pred.chunk(len(batch))):
                centre = p[:, :, n_t: p.shape[-2] - n_b, n_l: p.shape[-1] - n_r]
                dst = out[:, :, h0:h1, w0:w1]
                free = dst == 0
                dst[free] = centre[free].to(out.dtype)
        return out

    # ---- the loop ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_latent(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                        guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                        rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                        progress=lambda it: it, trace=None, logs=None, guidance_rescale=0.0, init_image=None, strength=1.0,
                        mask_image=None, latent_mask_image=None):
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
        t_start = window(num_inference_steps, strength)
        if init_image is None or mask_image is None:
            raise ValueError("a 9-channel UNet needs init_image and mask_image")
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
        B = len(prompts)
        shape = (B, LATENT_CHANNELS, height // s, width // s)      # the latent has the model's OUTPUT channels
        self.scheduler.set_timesteps(num_inference_steps)
        ts = self.scheduler.timesteps
        assert tuple(init_image.shape) == (height, width, 3) and init_image.dtype == np.uint8
        assert tuple(mask_image.shape) == (height, width) and mask_image.dtype == np.uint8
        sf = self.vae.config.scaling_factor
        dist = self.vae.encode(to_vae_input(init_image)).latent_dist
        eps_p = torch.randn(shape, dtype=self.torch_dtype)      # the posterior's noise first ...
        noise = torch.randn(shape, dtype=self.torch_dtype)      # ... then the initial noise
        a, b = self.add_noise_coefficients(ts[t_start])
        z0, x = init_latent(dist.mean.expand(shape), dist.std.expand(shape), eps_p, noise, sf, a, b)
        m = latent_mask(mask_image if latent_mask_image is None else latent_mask_image, s)
        # the picture with the hole blanked, through the binarised ORIGINAL mask; one more draw, after the two above
        dist_m = self.vae.encode(to_vae_input_masked(init_image, mask_image)).latent_dist
        eps_m = torch.randn((1,) + shape[1:], dtype=self.torch_dtype)
        zm = masked_latent(dist_m.mean, dist_m.std, eps_m, sf)
        self.last_init_latents, self.last_mask, self.last_masked_image_latents = z0, m, zm
        self._extras = self.make_extras(m, zm, B)
        for i in progress(range(t_start, len(ts))):
            t = ts[i]
            direction, info = self.approximate_latent_direction_w_resampling(
                x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=resampling_steps, drop_p=1 - new_p)
            if logs is not None and logs.get("init_downsampled_latent") is None:
                logs["init_downsampled_latent"] = info["init_downsampled_latent"]
            local = self.compute_local_uncond_signal(x, t, un, pun, vc)
            out = self.scheduler.step(self.guided(local, direction, guidance_scale), t, x)
            x0, nxt, cfg = out["pred_original_sample"], out["prev_sample"], guidance_scale
            if repaint_sampling and resampling_steps > 0 and i < len(ts) - 1:
                x = self.undo_step(nxt, ts[i + 1])                 # no blend: the model sees the known region in its input
                cfg = guidance_scale / 3
                direction, info = self.approximate_latent_direction_w_resampling(
                    x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=0, drop_p=1 - new_p)
                local = self.compute_local_uncond_signal(x, t, un, pun, vc)
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
            if trace is not None:
                trace.append(x.clone())
        return x
