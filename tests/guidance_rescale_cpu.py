"""Test-side restatement of guidance rescale (test infrastructure, never shipped; torch on the CPU).

``rescale_guided`` is the std rescale of arXiv 2305.08891 section 3.4 as diffusers pipelines apply it under the keyword
``guidance_rescale`` (the real reference carries the same function as ``rescale_noise_cfg``; the fixture
tests/golden/g15_guidance_rescale.npz holds ITS outputs and this restatement is compared with them bit for bit).

``RescaleOracle`` places it in the ElasticDiffusion loop with the semantics of DESIGN.md section 17, on top of the
unmodified ``oracle.elastic_oracle.ElasticOracle``:

  * both estimation phases: m_cfg = local + g * direction, m_text = local + direction (the g = 1 prediction), the rescaled
    m is what ``scheduler.step`` consumes;
  * the reduced-resolution prediction inside RRG: the same with (uncond_score, downsampled direction) and its own statistics;
  * ``guidance_rescale == 0`` evaluates exactly the expressions of the parent class.

It shares no code with elasticdiffusion_official_amd/.
"""
import torch
import torch.nn.functional as F

from oracle.elastic_oracle import CosineScheduler, ElasticOracle

# ---- the g15 fixture's cases (shared by tests/golden/make_guidance_rescale.py and the tests) -----------------------------
G15_SHAPES = [(1, 4, 8, 8), (2, 4, 33, 47), (3, 4, 13, 19), (1, 4, 128, 256)]
G15_MEANS = [0.0, 50.0]
G15_RESCALES = [0.7, 1.0]
G15_GUIDANCE = 10.0
G15_SEED0 = 1500
G15_PROBE_ABOVE, G15_PROBE_STRIDE = 16384, 16   # outputs larger than this are stored as a strided sample


def g15_key(shape, mean):
    return "x".join(str(s) for s in shape) + f"_m{int(mean)}"


def g15_cases():
    """-> [(key, shape, mean, seed)]; the seed is also stored in the fixture."""
    return [(g15_key(s, m), s, m, G15_SEED0 + 10 * i + j) for i, s in enumerate(G15_SHAPES) for j, m in enumerate(G15_MEANS)]


def g15_inputs(seed, shape, mean):
    """-> (local, direction, m_cfg, m_text) fp32: local = randn + mean, direction = 0.1 * randn, g = 10."""
    g = torch.Generator().manual_seed(int(seed))
    local = torch.randn(shape, generator=g) + mean
    direction = 0.1 * torch.randn(shape, generator=g)
    return local, direction, local + G15_GUIDANCE * direction, local + direction


def g15_probe(out):
    flat = out.flatten()
    return flat if flat.numel() <= G15_PROBE_ABOVE else flat[3::G15_PROBE_STRIDE].contiguous()


def sample_std(x):
    return x.std(dim=tuple(range(1, x.ndim)), keepdim=True)


def ratio_fp64(m_cfg, m_text):
    """std(m_text[b]) / std(m_cfg[b]) evaluated in fp64 on the fp32 inputs -> float64 [B]"""
    return (sample_std(m_text.double()) / sample_std(m_cfg.double())).flatten()


def rescale_with_ratio(m_cfg, ratio, guidance_rescale):
    """The elementwise part for a given fp32 ratio [B]: gr * (m * r) + (1 - gr) * m, each op rounded on its own."""
    r = ratio.to(m_cfg.dtype).view(-1, *([1] * (m_cfg.ndim - 1)))
    return guidance_rescale * (m_cfg * r) + (1 - guidance_rescale) * m_cfg


def rescale_guided(m_cfg, m_text, guidance_rescale):
    return rescale_with_ratio(m_cfg, (sample_std(m_text) / sample_std(m_cfg)).flatten(), guidance_rescale)


class RescaleOracle(ElasticOracle):
    guidance_rescale = 0.0

    def guided(self, base, direction, g):
        m = base + g * direction
        if not self.guidance_rescale:
            return m
        return rescale_guided(m, base + direction, self.guidance_rescale)

    def reduced_resolution_guidance(self, t, latent_x0_original, guidance_scale, rrg_scale, donwsampled_scores):
        low_latent = donwsampled_scores["latent"]
        eps = self.guided(donwsampled_scores["uncond_score"], donwsampled_scores["direction"], guidance_scale)
        ddim = self.scheduler.step(eps, t, low_latent)
        x0_up = F.interpolate(ddim["pred_original_sample"], size=latent_x0_original.shape[-2:], mode="nearest")
        grads = []
        for j in range(latent_x0_original.shape[0]):
            with torch.enable_grad():
                probe = latent_x0_original[j:j + 1].clone().detach().requires_grad_(True)
                loss = rrg_scale * F.mse_loss(x0_up[j:j + 1], probe)
                loss.backward()
            grads.append(probe.grad.clone() * -1.0)
        return torch.cat(grads), {"x0": [ddim["pred_original_sample"]], "rrg_latent_out": [ddim["prev_sample"]]}

    @torch.no_grad()
    def generate_latent(self, prompts, negative_prompts="", height=768, width=768, num_inference_steps=50,
                        guidance_scale=10.0, resampling_steps=20, new_p=0.3, rrg_stop_t=0.2, rrg_init_weight=1000,
                        rrg_scherduler_cls=CosineScheduler, cosine_scale=3.0, repaint_sampling=True,
                        progress=lambda it: it, condition_image=None, controlnet_conditioning_scale=1.0,
                        trace=None, logs=None, guidance_rescale=0.0):
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
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
        x = torch.randn((len(prompts), self.unet.config.in_channels, height // s, width // s), dtype=self.torch_dtype)
        self.scheduler.set_timesteps(num_inference_steps)
        cn = {}
        if condition_image is not None:
            cn = dict(condition_image=self.prepare_condition(condition_image),
                      controlnet_conditioning_scale=controlnet_conditioning_scale)
        ts = self.scheduler.timesteps
        for i, t in enumerate(progress(ts)):
            direction, info = self.approximate_latent_direction_w_resampling(
                x, t, text_embeds, add_text_embeds, downsample_size, resampling_steps=resampling_steps,
                drop_p=1 - new_p, **cn)
            if logs is not None and logs.get("init_downsampled_latent") is None:
                logs["init_downsampled_latent"] = info["init_downsampled_latent"]
            local = self.compute_local_uncond_signal(x, t, un, pun, vc, **cn)
            out = self.scheduler.step(self.guided(local, direction, guidance_scale), t, x)
            x0, nxt, cfg = out["pred_original_sample"], out["prev_sample"], guidance_scale
            if repaint_sampling and resampling_steps > 0 and i < len(ts) - 1:
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
            if trace is not None:
                trace.append(x.clone())
        return x

    def plain_cfg_generate(self, latent, text, pooled, guidance_scale, guidance_rescale=0.0):
        """The plain CFG + DDIM loop of ``generate()`` over ``unet_step`` with the rescale (noise_pred_text = cond)
        -> (final latent, [pred_original_sample per step])"""
        inter = []
        for t in self.scheduler.timesteps:
            uncond, cond = self.unet_step(torch.cat([latent] * 2), t, text, pooled).chunk(2)
            m = uncond + guidance_scale * (cond - uncond)
            if guidance_rescale:
                m = rescale_guided(m, cond, guidance_rescale)
            out = self.scheduler.step(m, t, latent)
            latent = out["prev_sample"]
            inter.append(out["pred_original_sample"])
        return latent, inter
