"""-m gpu: v-prediction, trailing / linspace spacing and zero-SNR betas through the HIP path.

Bars (the project's existing ones, tests/test_hip_parity.py / test_real_arch_parity.py):
  * kernels fed identical fp32 inputs: BIT-EXACT against the restatement's torch-CPU op sequence
    (``DDIMOracle.step`` with ``prediction_type="v_prediction"``, ``ElasticOracle.reduced_resolution_guidance``);
  * the fused epilogue in v mode: bit-identical to the chain of separate kernels in v mode;
  * end-to-end latents against the reference-held g13 fixtures and against the live oracle: rel-L2 < 1e-4, host RNG
    stream ends in exactly the reference's state; interleaved vs alone 1e-5;
  * the reduced-width real SD 1.5 architecture in fp32: rel-L2 < 1e-3 after every denoising step.
"""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from oracle import elastic_oracle as eo
from oracle.ddim import DDIMOracle
from tests import ddim_variants as V
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE, synthetic_text_embeds
from tests.golden import cases
from tests.test_hip_parity import DEV, FUSED_CASES, dev_i32, rel_l2

pytestmark = pytest.mark.gpu

V_TRAILING = dict(prediction_type="v_prediction", timestep_spacing="trailing")
V_TRAILING_ZSNR = dict(V_TRAILING, rescale_betas_zero_snr=True)


def _mods():
    from elasticdiffusion_official_amd import geometry, ops, schedule
    return geometry, ops, schedule


def _schedules(kw, steps):
    """(product schedule, restatement) with timesteps set; the restatement is plain DDIMOracle where it can be"""
    _, _, schedule = _mods()
    sch = schedule.DDIMSchedule(**kw)
    orc = DDIMOracle(**kw) if set(kw) == {"prediction_type"} else V.DDIMVariants(**kw)
    ts = sch.set_timesteps(steps)
    orc.set_timesteps(steps)
    assert torch.equal(ts, orc.timesteps)
    return sch, orc, ts


# ---------------------------------------------------------------------------------------------------
# kernels, bit-exact
# ---------------------------------------------------------------------------------------------------
# the shapes / timesteps of test_cfg_ddim_and_undo_bit_exact with DDIMOracle(prediction_type="v_prediction"), plus the
# alpha_bar = 0 timestep (999) of a zero-SNR trailing schedule and the last step of one (prev_t < 0)
KERNEL_SCHEDULES = [(dict(prediction_type="v_prediction"), 50, 0), (dict(prediction_type="v_prediction"), 50, 49),
                    (dict(prediction_type="v_prediction"), 10, 3), (dict(prediction_type="v_prediction"), 4, 1),
                    (V_TRAILING_ZSNR, 5, 0), (V_TRAILING_ZSNR, 5, 4), (V_TRAILING, 7, 2)]


@pytest.mark.parametrize("shape", [(1, 4, 64, 128), (2, 4, 67, 97), (1, 4, 128, 256)])
@pytest.mark.parametrize("kw,steps,ti", KERNEL_SCHEDULES)
def test_cfg_ddim_v_prediction_bit_exact(shape, kw, steps, ti):
    _, ops, _ = _mods()
    sch, orc_s, ts = _schedules(kw, steps)
    if kw.get("rescale_betas_zero_snr") and ti == 0:
        assert int(ts[ti]) == 999 and float(sch.alphas_cumprod[999]) == 0.0
    g = torch.Generator().manual_seed(steps * 100 + ti)
    local, direction, x = (torch.randn(shape, generator=g) for _ in range(3))
    guidance = 10.0 / 3
    out = orc_s.step(local + guidance * direction, ts[ti], x)
    prev, x0 = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    ops.cfg_ddim_step(local.to(DEV), direction.to(DEV), x.to(DEV), prev, x0, np.float32(guidance),
                      *sch.step_coefficients(ts[ti]), prediction_type="v_prediction")
    assert bool(torch.isfinite(prev).all())
    assert torch.equal(x0.cpu(), out["pred_original_sample"])
    assert torch.equal(prev.cpu(), out["prev_sample"])
    # the scalar (non-16-byte) kernel: an odd element count on a misaligned view gives the same values
    n = local.numel() - 3
    flat = [t.flatten()[1:1 + n].to(DEV).clone() for t in (local, direction, x)]
    buf_p, buf_z = torch.empty(n + 1, device=DEV), torch.empty(n + 1, device=DEV)
    ops.cfg_ddim_step(*flat, buf_p[1:], buf_z[1:], np.float32(guidance), *sch.step_coefficients(ts[ti]),
                      prediction_type="v_prediction")
    assert torch.equal(buf_p[1:].cpu(), out["prev_sample"].flatten()[1:1 + n])
    assert torch.equal(buf_z[1:].cpu(), out["pred_original_sample"].flatten()[1:1 + n])
    # the keyword's default and its explicit epsilon value are the epsilon kernels
    if not kw.get("rescale_betas_zero_snr"):
        e1, e2 = (torch.empty(shape, device=DEV) for _ in range(2))
        e3, e4 = (torch.empty(shape, device=DEV) for _ in range(2))
        ops.cfg_ddim_step(local.to(DEV), direction.to(DEV), x.to(DEV), e1, e2, np.float32(guidance),
                          *sch.step_coefficients(ts[ti]))
        ops.cfg_ddim_step(local.to(DEV), direction.to(DEV), x.to(DEV), e3, e4, np.float32(guidance),
                          *sch.step_coefficients(ts[ti]), prediction_type="epsilon")
        assert torch.equal(e1, e3) and torch.equal(e2, e4) and not torch.equal(e1, prev)


@pytest.mark.parametrize("Hl,Wl,h,w", [(64, 128, 32, 64), (128, 256, 64, 128), (67, 97, 44, 64), (96, 96, 64, 64)])
@pytest.mark.parametrize("weight", [1000.0, 437.53, 11.0])
@pytest.mark.parametrize("kw,steps,ti", [(dict(prediction_type="v_prediction"), 50, 7), (V_TRAILING_ZSNR, 5, 0)])
def test_rrg_update_v_prediction_bit_exact(Hl, Wl, h, w, weight, kw, steps, ti):
    geometry, ops, _ = _mods()
    sch, orc_s, ts = _schedules(kw, steps)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), orc_s)
    g = torch.Generator().manual_seed(int(weight))
    B = 2
    prev, x0 = torch.randn(B, 4, Hl, Wl, generator=g), torch.randn(B, 4, Hl, Wl, generator=g)
    low, unc, ldir = (torch.randn(B, 4, h, w, generator=g) for _ in range(3))
    t = ts[ti]
    grad, _ = orc.reduced_resolution_guidance(t, x0, guidance_scale=10.0 / 3, rrg_scale=np.float64(weight),
                                              donwsampled_scores={"latent": low, "uncond_score": unc, "direction": ldir})
    want = prev + grad
    pp = geometry.PickPlan(Hl, Wl, h, w)
    out = torch.empty(B, 4, Hl, Wl, device=DEV)
    sb, sa = sch.step_coefficients(t)[:2]
    ops.rrg_update(prev.to(DEV), x0.to(DEV), low.to(DEV), unc.to(DEV), ldir.to(DEV), dev_i32(pp.up_row),
                   dev_i32(pp.up_col), out, np.float32(10.0 / 3), sb, sa, np.float32(2.0 / (4 * Hl * Wl)),
                   np.float32(weight), prediction_type="v_prediction")
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------
# fused epilogue in v mode == the chain of separate kernels in v mode, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_CASES)
@pytest.mark.parametrize("B,K,dtype", [(1, 4, torch.float32), (2, 1, torch.bfloat16), (1, 8, torch.float16)])
@pytest.mark.parametrize("kw,steps,ti", [(dict(prediction_type="v_prediction"), 50, 7), (V_TRAILING_ZSNR, 5, 0)])
def test_fused_epilogue_v_prediction_equals_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype, kw, steps, ti):
    geometry, ops, _ = _mods()
    from elasticdiffusion_official_amd import host_rng
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    g = torch.Generator().manual_seed(Hl * 131 + Wl + K)
    x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    torch.manual_seed(17)
    stamp = torch.empty(h * w, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(h * w).draw(K, 0.7, lambda: None, stamp=stamp).to(DEV)
    stamp = stamp.to(DEV)
    T = {k: dev_i32(getattr(pp, k)) for k in ("src_row", "src_col", "inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")}
    cover = tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left))
    pick = tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col"))
    n_g, n_v = 2 * K * B, vp.V * B
    g_rows = torch.empty(n_g, 4, gpad.PH, gpad.PW, device=DEV, dtype=dtype)
    low = torch.empty(K, B, 4, h, w, device=DEV)
    ops.pick_assemble(x, idx, T["src_row"], T["src_col"], g_rows, h, w, gpad.top, gpad.left, None, low)
    g_out = torch.randn(n_g, 4, gpad.PH, gpad.PW, generator=g).to(dtype).to(DEV)
    v_cpu = torch.randn(n_v, 4, vpad.PH, vpad.PW, generator=g)
    v_cpu[torch.rand(v_cpu.shape, generator=g) < 0.2] = 0.0
    v_out = v_cpu.to(dtype).to(DEV)
    sch, _, ts = _schedules(kw, steps)
    coef = sch.step_coefficients(ts[ti])
    guidance, w_rrg, norm = np.float32(10.0 / 3), np.float32(437.53), np.float32(2.0 / (4 * Hl * Wl))
    vp_kw = dict(prediction_type="v_prediction")
    dirs = torch.empty(K, B, 4, h, w, device=DEV)
    unc1, ldir1 = torch.empty(B, 4, h, w, device=DEV), torch.empty(B, 4, h, w, device=DEV)
    direction1, local1 = torch.empty_like(x), torch.empty_like(x)
    prev1, x01, nxt1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ops.unpad_direction(g_out, dirs, unc1, gpad.top, gpad.left)
    ops.fill_directions(dirs, stamp, T["inv_row"], T["inv_col"], T["up_row"], T["up_col"], T["down_row"], T["down_col"],
                        direction1, ldir1)
    ops.scatter_centres(v_out, local1, vp.n_col_blocks, *cover)
    ops.cfg_ddim_step(local1, direction1, x, prev1, x01, guidance, *coef, **vp_kw)
    ops.rrg_update(prev1, x01, low[K - 1], unc1, ldir1, T["up_row"], T["up_col"], nxt1, guidance, coef[0], coef[1], norm,
                   w_rrg, **vp_kw)
    assert bool(torch.isfinite(nxt1).all())
    # with x_next (fused RRG) and every by-product
    out = {k: torch.full_like(x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    unc2, ldir2 = torch.full_like(unc1, 5.0), torch.full_like(ldir1, 5.0)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, out["prev"], out["x0"], low_dir=ldir2, uncond_last=unc2, direction=out["direction"],
                       local=out["local"], x_next=out["x_next"], low_latent=low[K - 1], rrg_norm=norm, rrg_weight=w_rrg,
                       **vp_kw)
    for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1)):
        assert torch.equal(out[name], want), name
    assert torch.equal(unc2, unc1) and torch.equal(ldir2, ldir1)
    # without x_next and without the optional outputs
    p3, z3 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, p3, z3, **vp_kw)
    assert torch.equal(p3, prev1) and torch.equal(z3, x01)
    if not kw.get("rescale_betas_zero_snr"):  # and v mode is not the epsilon launch
        p4, z4 = torch.empty_like(x), torch.empty_like(x)
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                           coef, p4, z4)
        assert not torch.equal(p4, p3)


# ---------------------------------------------------------------------------------------------------
# end to end against the reference-held fixtures
# ---------------------------------------------------------------------------------------------------
def _pipe_for(name, text_encoder=None):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    c = V.VARIANT_CASES[name]
    xl = c["sd"].startswith("XL")
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=V.VBS, unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            text_encoder=text_encoder or V.embed_fn(xl), scheduler=DDIMSchedule(**c["sched"]))


def _loop_kw(name):
    c = V.VARIANT_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)


@pytest.mark.parametrize("name", list(V.VARIANT_CASES))
def test_end_to_end_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "g13_scheduler_variants.npz"))
    pipe = _pipe_for(name)
    assert [int(t) for t in pipe.scheduler.set_timesteps(V.VARIANT_CASES[name]["steps"])] == V.VARIANT_CASES[name]["timesteps"]
    pipe.seed_everything(V.SEED)
    imgs, log = pipe.generate_image("p", "", output_type="pt", **_loop_kw(name))
    tail = torch.rand(4)
    z = pipe.last_latents.cpu()
    want = torch.from_numpy(g[f"{name}/latent"])
    assert z.shape == want.shape and bool(torch.isfinite(imgs).all())
    print(f"{name}: rel-L2 vs reference latent {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/rng_tail"])
    assert log == {}


def test_end_to_end_with_separate_glue_kernels(golden_dir):
    """FUSED_GLUE off: ed_cfg_ddim_step_pt / ed_rrg_update_pt carry the loop; same bar, and bit-identical to the fused path."""
    from elasticdiffusion_official_amd import pipeline
    name = "v_trailing_zsnr"
    g = np.load(os.path.join(golden_dir, "g13_scheduler_variants.npz"))
    lat, tails = {}, {}
    for fused in (False, True):
        pipeline.FUSED_GLUE = fused
        try:
            pipe = _pipe_for(name)
            pipe.seed_everything(V.SEED)
            lat[fused] = pipe.generate_latents("p", "", **_loop_kw(name)).cpu()
            tails[fused] = torch.rand(4)
        finally:
            pipeline.FUSED_GLUE = True
    assert rel_l2(lat[False], torch.from_numpy(g[f"{name}/latent"])) < 1e-4
    np.testing.assert_array_equal(tails[False].numpy(), g[f"{name}/rng_tail"])
    assert torch.equal(lat[False], lat[True])


def test_interleaved_two_in_flight(golden_dir):
    """generate_latents_interleaved with a v / trailing schedule: every image as if it had run alone (1e-5), and the one
    with the fixture's seed at the fixture's bar."""
    name = "v_trailing"
    g = np.load(os.path.join(golden_dir, "g13_scheduler_variants.npz"))
    kw = _loop_kw(name)
    seeds = [V.SEED, 11, 12]

    def embed(prompts):  # stateless (the programs' calls interleave); the values V.embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe_for(name, text_encoder=embed)
    alone = []
    for s in seeds:
        pipe.seed_everything(s)
        alone.append(pipe.generate_latents("p", "", **kw).clone())
    got = pipe.generate_latents_interleaved([dict(prompts="p", negative_prompts="", seed=s) for s in seeds], in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], torch.from_numpy(g[f"{name}/latent"])) < 1e-4
    assert pipe.ticks < 3 * (2 * V.VARIANT_CASES[name]["steps"] - 1)  # calls were actually fused


# ---------------------------------------------------------------------------------------------------
# against the live oracle: ControlNet, two prompts, generate()
# ---------------------------------------------------------------------------------------------------
def test_controlnet_v_trailing_vs_oracle():
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    kw = dict(height=512, width=1024, num_inference_steps=3, resampling_steps=2, **cases.E2E_KW)
    ds = eo.get_downsample_size(512, 1024, "1.5")
    ckw = dict(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=V.embed_fn(False),
                            controlnet=FakeControlNet(), scheduler=DDIMSchedule(**V_TRAILING))
    pipe.seed_everything(7)
    z = pipe.generate_latents("p", "", **kw, **ckw).cpu()
    tail = torch.rand(4)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), V.DDIMVariants(**V_TRAILING), V.embed_fn(False), sd_version="1.5",
                           view_batch_size=4, controlnet=FakeControlNet())
    orc.seed_everything(7)
    want = orc.generate_latent("p", "", **kw, **ckw)
    print(f"controlnet v/trailing: rel-L2 {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert torch.equal(tail, torch.rand(4))


def test_two_prompts_v_trailing_zero_snr_vs_oracle():
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    kw = dict(height=512, width=768, num_inference_steps=3, resampling_steps=1, **cases.E2E_KW)
    prompts = ["p0", "p1"]
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=3, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=V.embed_fn(False, 2),
                            scheduler=DDIMSchedule(**V_TRAILING_ZSNR))
    pipe.seed_everything(5)
    z = pipe.generate_latents(prompts, "", **kw).cpu()
    tail = torch.rand(3)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), V.DDIMVariants(**V_TRAILING_ZSNR), V.embed_fn(False, 2), sd_version="1.5",
                           view_batch_size=3)
    orc.seed_everything(5)
    want = orc.generate_latent(prompts, "", **kw)
    assert z.shape == want.shape == (2, 4, 64, 96)
    print(f"two prompts v/trailing/zero-SNR: rel-L2 {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert torch.equal(tail, torch.rand(3))


@pytest.mark.parametrize("name", ["gen_sd_pad_32x64", "gen_xl_64x128"])
def test_generate_v_prediction_vs_oracle(name):
    """``generate()`` (ED:761-796, the verbose "global_img") with a v / trailing schedule against the same loop over the
    oracle's ``unet_step`` and the restatement's ``step``."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    c = cases.G11_CASES[name]
    xl = c["sd"].startswith("XL")
    (un, pun), (co, pco) = synthetic_text_embeds(1, xl=xl)
    text, pooled = torch.cat([un, co]), torch.cat([pun, pco])
    size = (4 * 8 * c["h"], 4 * 8 * c["w"])
    pipe = ElasticDiffusion(DEV, c["sd"], log_freq=1, unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            scheduler=DDIMSchedule(**V_TRAILING))
    pipe.default_size = size
    pipe.scheduler.set_timesteps(c["steps"])
    pipe.seed_everything(c["seed"])
    z = torch.randn(1, 4, c["h"], c["w"])
    seen = {}
    dec = pipe.decode_latents
    pipe.decode_latents = lambda lat: (seen.__setitem__("z", lat.clone()), dec(lat))[1]
    _, info = pipe.generate(z, text, pooled, guidance_scale=c["guidance"])
    tail = torch.rand(4)
    orc = eo.ElasticOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), V.DDIMVariants(**V_TRAILING), sd_version=c["sd"],
                           pooled_dim=16 if xl else None)
    orc.default_size = size
    orc.scheduler.set_timesteps(c["steps"])
    orc.seed_everything(c["seed"])
    latent = torch.randn(1, 4, c["h"], c["w"])
    inter = []
    for t in orc.scheduler.timesteps:
        uncond, cond = orc.unet_step(torch.cat([latent] * 2), t, text, pooled).chunk(2)
        out = orc.scheduler.step(uncond + c["guidance"] * (cond - uncond), t, latent)
        latent = out["prev_sample"]
        inter.append(out["pred_original_sample"])
    assert rel_l2(seen["z"], latent) < 1e-4, rel_l2(seen["z"], latent)
    assert rel_l2(torch.cat(info["inter_x0"]), torch.cat(inter)) < 1e-4
    assert torch.equal(tail, torch.rand(4))


# ---------------------------------------------------------------------------------------------------
# the real (reduced-width) SD 1.5 architecture in fp32, v / trailing
# ---------------------------------------------------------------------------------------------------
def test_real_architecture_fp32_v_trailing():
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    from tests import realarch as R
    c = R.REAL_CASES["cfg2_sd_512x1024"]
    unet, vae, _ = R.build_small(c["sd"])
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **R.LOOP_KW)
    orc = eo.ElasticOracle(unet, vae, V.DDIMVariants(**V_TRAILING), R.embed_fn(False), sd_version=c["sd"],
                           view_batch_size=c["vbs"])
    orc.seed_everything(c["seed"])
    want = []
    orc.generate_latent("p", "", trace=want, **kw)
    otail = torch.rand(4)
    pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=copy.deepcopy(unet), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(False), scheduler=DDIMSchedule(**V_TRAILING))
    pipe.seed_everything(c["seed"])
    got = []
    pipe.generate_latents("p", "", trace=got, **kw)
    tail = torch.rand(4)
    rels = [rel_l2(a, b) for a, b in zip(got, want)]
    print("real architecture fp32 v/trailing per-step rel-L2:", ["%.3e" % r for r in rels])
    assert len(rels) == c["steps"] and max(rels) < 1e-3, rels
    assert torch.equal(tail, otail)


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_scheduler_flags(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    base = ["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1", "--outdir",
            str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4"]
    d0 = main(base + ["--exp", "default"])
    d1 = main(base + ["--exp", "vpred", "--prediction_type", "v_prediction", "--timestep_spacing", "trailing"])
    a0 = np.asarray(Image.open(os.path.join(d0, "0.png")), dtype=np.float32)
    a1 = np.asarray(Image.open(os.path.join(d1, "0.png")), dtype=np.float32)
    assert a0.shape == a1.shape == (512, 512, 3) and np.isfinite(a1).all()
    assert a1.std() > 0  # a NaN latent decodes to a constant image
    assert not np.array_equal(a0, a1)
    args = open(os.path.join(d1, "args.txt")).read()
    assert "prediction_type: v_prediction" in args and "timestep_spacing: trailing" in args
    assert glob.glob(os.path.join(d1, "*.png"))
