"""-m gpu: guidance rescale through the HIP path.

Bars:
  * the per-sample std ratio (a reduction) against the same expression in fp64 on the same fp32 inputs: 2 ulp = 2.4e-7
    relative (torch's own fp32 evaluation sits 1.8e-8 .. 8e-8 from fp64 on the eight g15 inputs); two launches give the same bits;
  * the elementwise part, fed the kernel's own ratio: BIT-EXACT against the torch-CPU op sequence
    ``DDIMOracle.step(gr * (m * r) + (1 - gr) * m, t, x)`` / ``reduced_resolution_guidance``;
  * the fused epilogue fed the same ratio buffers: bit-identical to the chain of separate kernels;
  * end-to-end latents against the CPU restatement (tests/guidance_rescale_cpu.py): the project's rel-L2 < 1e-4, identical
    host RNG end state; interleaved vs alone 1e-5; ``guidance_rescale=0`` launches and computes what the loop always did.
"""
import os

import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle
from tests import ddim_variants as V
from tests import guidance_rescale_cpu as G
from tests.fakes import FakeUNet, FakeVAE, synthetic_text_embeds
from tests.golden import cases
from tests.test_hip_parity import DEV, FUSED_CASES, dev_i32, rel_l2
from tests.test_scheduler_variants_gpu import V_TRAILING_ZSNR, _schedules

pytestmark = pytest.mark.gpu

ULP2 = 2.4e-7   # 2 ulp of fp32, relative
GR = 0.7
EPS = dict()
V_PRED = dict(prediction_type="v_prediction")


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _moments(local, direction, g, text=None):
    """ops.guidance_moments on device tensors [B, ...] -> ratio f32 [B] (device)"""
    ops = _ops()
    B = local.shape[0]
    ratio = torch.full((B,), -1.0, device=DEV)
    ws = ops.guidance_moments_workspace(B, local.numel() // B, 0, DEV)
    ops.guidance_moments(local, direction, np.float32(g), ratio, ws, text=text)
    return ratio


def _close(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return bool(((got - want).abs() <= ULP2 * want.abs()).all())


# ---------------------------------------------------------------------------------------------------
# the reduction
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,shape,mean,seed", G.g15_cases())
def test_guidance_moments_within_2_ulp_of_fp64_and_deterministic(golden_dir, key, shape, mean, seed):
    """(1,4,8,8) is less than one block, (1,4,128,256) spans 128 blocks (the merge), B = 2 / 3 the per-sample indexing,
    33x47 / 13x19 the tails; the mean-50 cases are the ones a plain fp32 sum of squares fails (1e-4)."""
    g15 = np.load(os.path.join(golden_dir, "g15_guidance_rescale.npz"))
    local, direction, m_cfg, m_text = G.g15_inputs(seed, shape, mean)
    want = torch.from_numpy(g15[f"{key}/ratio_fp64"])
    l_d, d_d = local.to(DEV), direction.to(DEV)
    r1 = _moments(l_d, d_d, G.G15_GUIDANCE)
    r2 = _moments(l_d, d_d, G.G15_GUIDANCE)
    err = float(((r1.cpu().double() - want).abs() / want).max())
    print(f"{key}: ratio {r1.cpu().tolist()} rel. error vs fp64 {err:.2e} (bar {ULP2:.1e})")
    assert err <= ULP2, err
    assert torch.equal(r1, r2)
    # m_text given as a tensor (plain CFG): the same values, the same bits
    assert torch.equal(_moments(l_d, d_d, G.G15_GUIDANCE, text=m_text.to(DEV)), r1)
    # and the whole function, with the kernel's ratio, is the reference's output to the ratio's accuracy
    for gr in G.G15_RESCALES:
        got = G.g15_probe(G.rescale_with_ratio(m_cfg, r1.cpu(), gr)).double()
        ref = torch.from_numpy(g15[f"{key}/gr{gr}/out"]).double()
        assert float((got - ref).abs().max() / ref.abs().max()) < 4 * ULP2


def test_guidance_moments_rejects_bad_arguments():
    ops = _ops()
    a = torch.zeros(2, 4, 8, 8, device=DEV)
    ratio, ws = torch.empty(2, device=DEV), ops.guidance_moments_workspace(2, 256, 0, DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.guidance_moments(a.cpu(), a, 1.0, ratio, ws)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.guidance_moments(a, a, 1.0, ratio, ws[:1])
    with pytest.raises(RuntimeError, match="equal-shaped"):
        ops.guidance_moments(a, a[:1], 1.0, ratio, ws)
    with pytest.raises(RuntimeError, match="needs ratio"):
        ops.cfg_ddim_step(a, a, a, a.clone(), a.clone(), 1.0, 1.0, 1.0, 1.0, 1.0, guidance_rescale=0.5)
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(a, a, a, a.clone(), a.clone(), 1.0, 1.0, 1.0, 1.0, 1.0, ratio=ratio, guidance_rescale=1.5)
    ops.guidance_moments(a + 1, a, 1.0, ratio, ws)   # the launch state is clean again; a constant sample gives 0 / 0
    assert bool(torch.isnan(ratio).all())


# ---------------------------------------------------------------------------------------------------
# the consumers, bit-exact given the ratio
# ---------------------------------------------------------------------------------------------------
KERNEL_SCHEDULES = [(EPS, 50, 7), (EPS, 4, 3), (V_PRED, 50, 0), (V_PRED, 10, 3), (V_TRAILING_ZSNR, 5, 0), (V_TRAILING_ZSNR, 5, 4)]


@pytest.mark.parametrize("shape", [(1, 4, 64, 128), (2, 4, 67, 97), (3, 4, 13, 19)])
@pytest.mark.parametrize("kw,steps,ti", KERNEL_SCHEDULES)
def test_cfg_ddim_rescaled_bit_exact(shape, kw, steps, ti):
    ops = _ops()
    sch, orc_s, ts = _schedules(kw, steps)
    pt = dict(prediction_type=kw.get("prediction_type", "epsilon"))
    if kw.get("rescale_betas_zero_snr") and ti == 0:
        assert int(ts[ti]) == 999 and float(sch.alphas_cumprod[999]) == 0.0
    g = torch.Generator().manual_seed(steps * 100 + ti)
    local, direction, x = (torch.randn(shape, generator=g) for _ in range(3))
    local = local + 3.0
    guidance = 10.0 / 3
    coef = sch.step_coefficients(ts[ti])
    l_d, d_d, x_d = local.to(DEV), direction.to(DEV), x.to(DEV)
    ratio = _moments(l_d, d_d, guidance)
    m_cfg, m_text = local + guidance * direction, local + direction
    assert _close(ratio, G.ratio_fp64(m_cfg, m_text))
    out = orc_s.step(G.rescale_with_ratio(m_cfg, ratio.cpu(), GR), ts[ti], x)
    prev, x0 = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    ops.cfg_ddim_step(l_d, d_d, x_d, prev, x0, np.float32(guidance), *coef, **pt, ratio=ratio, guidance_rescale=GR)
    assert bool(torch.isfinite(prev).all())
    assert torch.equal(x0.cpu(), out["pred_original_sample"])
    assert torch.equal(prev.cpu(), out["prev_sample"])
    # the scalar kernel: two samples of an odd length on misaligned outputs
    per = local.numel() // 2 - 3 - (local.numel() // 2) % 2
    assert per % 2 == 1
    fl, fd, fx = (t.flatten()[1:1 + 2 * per].reshape(2, per) for t in (local, direction, x))
    r2 = _moments(fl.to(DEV), fd.to(DEV), guidance)
    want = orc_s.step(G.rescale_with_ratio(fl + guidance * fd, r2.cpu(), GR), ts[ti], fx)
    buf_p, buf_z = torch.empty(2 * per + 1, device=DEV), torch.empty(2 * per + 1, device=DEV)
    ops.cfg_ddim_step(fl.to(DEV), fd.to(DEV), fx.to(DEV), buf_p[1:], buf_z[1:], np.float32(guidance), *coef, **pt, ratio=r2,
                      guidance_rescale=GR)
    assert torch.equal(buf_p[1:].cpu(), want["prev_sample"].flatten())
    assert torch.equal(buf_z[1:].cpu(), want["pred_original_sample"].flatten())
    # ratio=None is the existing call, and a factor of 0 with a ratio computes the same values
    e1, e2, e3, e4, e5, e6 = (torch.empty(shape, device=DEV) for _ in range(6))
    ops.cfg_ddim_step(l_d, d_d, x_d, e1, e2, np.float32(guidance), *coef, **pt)
    ops.cfg_ddim_step(l_d, d_d, x_d, e3, e4, np.float32(guidance), *coef, **pt, ratio=None, guidance_rescale=0.0)
    ops.cfg_ddim_step(l_d, d_d, x_d, e5, e6, np.float32(guidance), *coef, **pt, ratio=ratio, guidance_rescale=0.0)
    assert torch.equal(e1, e3) and torch.equal(e2, e4) and torch.equal(e1, e5) and torch.equal(e2, e6)
    assert not torch.equal(e1, prev)


def test_plain_aligned_calls_still_take_the_16_byte_kernels():
    """The float4 path of the DDIM step is chosen as it always was when no ratio is given (element count % 4 and 16-byte
    alignment); under a ratio the ONLY additional diversion to the scalar kernels is a sample that is not a whole number of
    float4s.  ``cfg_ddim_step_width`` evaluates the predicate the launch itself uses."""
    ops = _ops()

    def bufs(n, offset=0):
        return [torch.zeros(n + offset, device=DEV)[offset:] for _ in range(5)]

    r1, r2, r3 = (torch.ones(b, device=DEV) for b in (1, 2, 3))
    assert ops.cfg_ddim_step_width(*bufs(4 * 64 * 128)) == 4                  # the plain call of every existing test / generate()
    assert ops.cfg_ddim_step_width(*bufs(2 * 4 * 67 * 97)) == 4
    assert ops.cfg_ddim_step_width(*bufs(8)) == 4
    assert ops.cfg_ddim_step_width(*bufs(4 * 67 * 97 - 3)) == 1               # n % 4 != 0
    assert ops.cfg_ddim_step_width(*bufs(1024, offset=1)) == 1                # misaligned
    b = bufs(1024)
    b[3] = torch.zeros(1025, device=DEV)[1:]
    assert ops.cfg_ddim_step_width(*b) == 1                                   # one misaligned output is enough
    assert ops.cfg_ddim_step_width(*bufs(4 * 64 * 128), ratio=r1) == 4        # with a ratio: the same ...
    assert ops.cfg_ddim_step_width(*bufs(2 * 4 * 67 * 97), ratio=r2) == 4
    assert ops.cfg_ddim_step_width(*bufs(3 * 4 * 13 * 19), ratio=r3) == 4
    assert ops.cfg_ddim_step_width(*bufs(2 * 1002), ratio=r2) == 1            # ... except per-sample length % 4 != 0 (n % 4 == 0)
    assert ops.cfg_ddim_step_width(*bufs(2 * 1002)) == 4                      # which the plain call does not care about
    assert ops.cfg_ddim_step_width(*bufs(1024, offset=1), ratio=r1) == 1
    # both widths compute the same bits, plain and rescaled (1002 per sample: scalar under a ratio, float4 without)
    g = torch.Generator().manual_seed(4)
    l, d, x = (torch.randn(2, 1002, generator=g).to(DEV) for _ in range(3))
    ratio = _moments(l, d, 3.0)
    coef = (0.6, 0.8, 0.9, 0.43)
    outs = []
    for view in (lambda t: t, lambda t: torch.cat([t.flatten()[:1], t.flatten()])[1:].reshape(2, 1002)):  # aligned / misaligned copy
        li, di, xi = view(l), view(d), view(x)
        p, z, pr, zr = (torch.empty_like(l) for _ in range(4))
        ops.cfg_ddim_step(li, di, xi, p, z, 3.0, *coef)
        ops.cfg_ddim_step(li, di, xi, pr, zr, 3.0, *coef, ratio=ratio, guidance_rescale=GR)
        outs.append((p, z, pr, zr))
    assert ops.cfg_ddim_step_width(l, d, x, outs[0][0], outs[0][1]) == 4
    assert ops.cfg_ddim_step_width(view(l), view(d), view(x), outs[1][0], outs[1][1]) == 1
    assert all(torch.equal(a, b) for a, b in zip(*outs))


class _FixedRatioOracle(G.RescaleOracle):
    """The restatement with the std ratio given (the kernel's own, read back) instead of recomputed by torch."""
    fixed_ratio = None

    def guided(self, base, direction, g):
        return G.rescale_with_ratio(base + g * direction, self.fixed_ratio, self.guidance_rescale)


@pytest.mark.parametrize("Hl,Wl,h,w", [(64, 128, 32, 64), (67, 97, 44, 64), (96, 96, 64, 64)])
@pytest.mark.parametrize("kw,steps,ti", [(EPS, 50, 7), (V_PRED, 50, 7), (V_TRAILING_ZSNR, 5, 0)])
def test_rrg_update_rescaled_bit_exact(Hl, Wl, h, w, kw, steps, ti):
    from elasticdiffusion_official_amd import geometry
    ops = _ops()
    sch, orc_s, ts = _schedules(kw, steps)
    pt = dict(prediction_type=kw.get("prediction_type", "epsilon"))
    weight, guidance, B = 437.53, 10.0 / 3, 2
    g = torch.Generator().manual_seed(Hl + w)
    prev, x0 = torch.randn(B, 4, Hl, Wl, generator=g), torch.randn(B, 4, Hl, Wl, generator=g)
    low, unc, ldir = (torch.randn(B, 4, h, w, generator=g) for _ in range(3))
    unc = unc - 2.0
    unc_d, ldir_d = unc.to(DEV), ldir.to(DEV)
    ratio_low = _moments(unc_d, ldir_d, guidance)
    assert _close(ratio_low, G.ratio_fp64(unc + guidance * ldir, unc + ldir))
    orc = _FixedRatioOracle(FakeUNet(64), FakeVAE(), orc_s)
    orc.guidance_rescale, orc.fixed_ratio = GR, ratio_low.cpu()
    t = ts[ti]
    grad, _ = orc.reduced_resolution_guidance(t, x0, guidance_scale=guidance, rrg_scale=np.float64(weight),
                                              donwsampled_scores={"latent": low, "uncond_score": unc, "direction": ldir})
    want = prev + grad
    pp = geometry.PickPlan(Hl, Wl, h, w)
    sb, sa = sch.step_coefficients(t)[:2]
    args = (prev.to(DEV), x0.to(DEV), low.to(DEV), unc_d, ldir_d, dev_i32(pp.up_row), dev_i32(pp.up_col))
    tail = (np.float32(guidance), sb, sa, np.float32(2.0 / (4 * Hl * Wl)), np.float32(weight))
    out, plain, none = (torch.empty(B, 4, Hl, Wl, device=DEV) for _ in range(3))
    ops.rrg_update(*args, out, *tail, **pt, ratio_low=ratio_low, guidance_rescale=GR)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out.cpu(), want)
    ops.rrg_update(*args, plain, *tail, **pt)
    ops.rrg_update(*args, none, *tail, **pt, ratio_low=None, guidance_rescale=0.0)
    assert torch.equal(plain, none) and not torch.equal(plain, out)


# ---------------------------------------------------------------------------------------------------
# fused == separate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_CASES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kw,steps,ti", [(EPS, 50, 7), (V_TRAILING_ZSNR, 5, 0)])
def test_fused_moments_and_epilogue_equal_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype, kw, steps, ti):
    from elasticdiffusion_official_amd import geometry, host_rng
    ops = _ops()
    pt = dict(prediction_type=kw.get("prediction_type", "epsilon"))
    ws_ = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws_, ws_, d - ws_)
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
    g_out = (torch.randn(n_g, 4, gpad.PH, gpad.PW, generator=g) + 0.5).to(dtype).to(DEV)
    v_cpu = torch.randn(n_v, 4, vpad.PH, vpad.PW, generator=g) - 1.5
    v_cpu[torch.rand(v_cpu.shape, generator=g) < 0.2] = 0.0
    v_out = v_cpu.to(dtype).to(DEV)
    sch, _, ts = _schedules(kw, steps)
    coef = sch.step_coefficients(ts[ti])
    guidance, w_rrg, norm = np.float32(10.0 / 3), np.float32(437.53), np.float32(2.0 / (4 * Hl * Wl))
    # ---- the un-fused chain's by-products and their ratios ----
    dirs = torch.empty(K, B, 4, h, w, device=DEV)
    unc1, ldir1 = torch.empty(B, 4, h, w, device=DEV), torch.empty(B, 4, h, w, device=DEV)
    direction1, local1 = torch.empty_like(x), torch.empty_like(x)
    ops.unpad_direction(g_out, dirs, unc1, gpad.top, gpad.left)
    ops.fill_directions(dirs, stamp, T["inv_row"], T["inv_col"], T["up_row"], T["up_col"], T["down_row"], T["down_col"],
                        direction1, ldir1)
    ops.scatter_centres(v_out, local1, vp.n_col_blocks, *cover)
    r1, rl1 = _moments(local1, direction1, guidance), _moments(unc1, ldir1, guidance)
    lc, dc = local1.cpu(), direction1.cpu()
    assert _close(r1, G.ratio_fp64(lc + float(guidance) * dc, lc + dc))
    # ---- the fused reduction over the model output rows ----
    geo = (vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance)
    wsp = ops.guidance_moments_workspace(B, 4 * Hl * Wl, 4 * h * w, DEV)
    r2, rl2 = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    ops.phase_moments(g_out, v_out, x.shape, stamp, pick, cover, *geo, r2, wsp, ratio_low=rl2)
    assert _close(r2, r1) and _close(rl2, rl1), (r2, r1, rl2, rl1)
    r3, rl3 = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    ops.phase_moments(g_out, v_out, x.shape, stamp, pick, cover, *geo, r3, wsp, ratio_low=rl3)
    assert torch.equal(r3, r2) and torch.equal(rl3, rl2)           # deterministic
    r4 = torch.full((B,), -1.0, device=DEV)
    ops.phase_moments(g_out, v_out, x.shape, stamp, pick, cover, *geo, r4, wsp)   # without the reduced-resolution pair
    assert torch.equal(r4, r2)
    # ---- both paths fed the same ratio buffers ----
    prev1, x01, nxt1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ops.cfg_ddim_step(local1, direction1, x, prev1, x01, guidance, *coef, **pt, ratio=r2, guidance_rescale=GR)
    ops.rrg_update(prev1, x01, low[K - 1], unc1, ldir1, T["up_row"], T["up_col"], nxt1, guidance, coef[0], coef[1], norm,
                   w_rrg, **pt, ratio_low=rl2, guidance_rescale=GR)
    assert bool(torch.isfinite(nxt1).all())
    out = {k: torch.full_like(x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    unc2, ldir2 = torch.full_like(unc1, 5.0), torch.full_like(ldir1, 5.0)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, *geo, coef, out["prev"], out["x0"], low_dir=ldir2,
                       uncond_last=unc2, direction=out["direction"], local=out["local"], x_next=out["x_next"],
                       low_latent=low[K - 1], rrg_norm=norm, rrg_weight=w_rrg, **pt, ratio=r2, ratio_low=rl2,
                       guidance_rescale=GR)
    for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1)):
        assert torch.equal(out[name], want), name
    assert torch.equal(unc2, unc1) and torch.equal(ldir2, ldir1)
    # without RRG (no x_next, no ratio_low) and without the optional outputs
    p3, z3 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, *geo, coef, p3, z3, **pt, ratio=r2, guidance_rescale=GR)
    assert torch.equal(p3, prev1) and torch.equal(z3, x01)
    # and the rescale is not a no-op
    p4, z4 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, *geo, coef, p4, z4, **pt)
    assert not torch.equal(p4, p3)
    with pytest.raises(RuntimeError, match="ratio_low"):
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, *geo, coef, p4, z4, x_next=out["x_next"],
                           low_latent=low[K - 1], **pt, ratio=r2, guidance_rescale=GR)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _pipe(name, sched_kw, text_encoder=None, **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    c = cases.E2E_CASES[name]
    xl = c["sd"].startswith("XL")
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            text_encoder=text_encoder or V.embed_fn(xl), scheduler=DDIMSchedule(**sched_kw), **extra)


def _loop_kw(name):
    c = cases.E2E_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)


_ORACLE = {}


def _oracle_latent(name, sched_kw):
    """The CPU restatement's latent and RNG tail for one case, computed once and shared."""
    key = (name, tuple(sorted(sched_kw.items())))
    if key not in _ORACLE:
        c = cases.E2E_CASES[name]
        xl = c["sd"].startswith("XL")
        orc = G.RescaleOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), V.DDIMVariants(**sched_kw), V.embed_fn(xl),
                              sd_version=c["sd"], view_batch_size=c["vbs"], pooled_dim=16 if xl else None)
        orc.seed_everything(c["seed"])
        z = orc.generate_latent("p", "", **_loop_kw(name), guidance_rescale=GR)
        _ORACLE[key] = (z, torch.rand(4))
    return _ORACLE[key]


E2E = [("cfg2_sd_512x1024", EPS), ("cfg2_sd_512x1024", V_TRAILING_ZSNR), ("xl_single_view_512x1024", EPS),
       ("xl_single_view_512x1024", V_TRAILING_ZSNR)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,sched_kw", E2E)
def test_end_to_end_vs_cpu_restatement(name, sched_kw, fused):
    """cfg2: padded global rows, RePaint and RRG active; xl_single_view: SDXL geometry.  Fused glue and the separate kernels."""
    from elasticdiffusion_official_amd import pipeline
    want, otail = _oracle_latent(name, sched_kw)
    pipeline.FUSED_GLUE = fused
    try:
        pipe = _pipe(name, sched_kw)
        pipe.seed_everything(cases.E2E_CASES[name]["seed"])
        z = pipe.generate_latents("p", "", **_loop_kw(name), guidance_rescale=GR).cpu()
        tail = torch.rand(4)
    finally:
        pipeline.FUSED_GLUE = True
    print(f"{name} {sorted(sched_kw)} fused={fused}: rel-L2 vs restatement {rel_l2(z, want):.3e}")
    assert bool(torch.isfinite(z).all())
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert torch.equal(tail, otail)


@pytest.mark.parametrize("name,sched_kw", E2E)
def test_zero_is_the_loop_as_it_was_and_the_keyword_is_not_ignored(name, sched_kw):
    from elasticdiffusion_official_amd import ops
    seed = cases.E2E_CASES[name]["seed"]
    lat, counts = {}, {}
    for label, extra in (("omitted", {}), ("zero", dict(guidance_rescale=0.0)), ("on", dict(guidance_rescale=GR))):
        pipe = _pipe(name, sched_kw)
        pipe.seed_everything(seed)
        ops.TIMER.start()
        try:
            lat[label] = pipe.generate_latents("p", "", **_loop_kw(name), **extra).cpu()
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert torch.equal(lat["omitted"], lat["zero"])
    assert rel_l2(lat["on"], lat["omitted"]) > 1e-3
    # launches: with 0 exactly what the loop launches without the keyword -- no moments, no *_gr entry point
    steps = cases.E2E_CASES[name]["steps"]
    phases = 2 * steps - 1
    epi = "ed_phase_epilogue_pt" if sched_kw.get("prediction_type") == "v_prediction" else "ed_phase_epilogue"
    assert counts["omitted"] == counts["zero"]
    glue = {k: v for k, v in counts["zero"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k
            or "moments" in k or k.endswith("_gr")}
    assert glue == {"ed_assemble_rows": phases, epi: phases, "ed_undo_step": steps - 1}, counts["zero"]
    glue_on = {k: v for k, v in counts["on"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k
               or "moments" in k or k.endswith("_gr")}
    assert glue_on == {"ed_assemble_rows": phases, "ed_phase_moments": phases, "ed_phase_epilogue_gr": phases,
                       "ed_undo_step": steps - 1}, counts["on"]


@pytest.mark.parametrize("name,sched_kw", E2E)
def test_interleaved_two_jobs_match_each_alone(name, sched_kw):
    kw = dict(_loop_kw(name), guidance_rescale=GR)
    xl = cases.E2E_CASES[name]["sd"].startswith("XL")

    def embed(prompts):  # stateless (the programs' calls interleave); the values V.embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1, xl=xl)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe(name, sched_kw, text_encoder=embed)
    seeds = [cases.E2E_CASES[name]["seed"], 11]
    alone = []
    for s in seeds:
        pipe.seed_everything(s)
        alone.append(pipe.generate_latents("p", "", **kw).clone())
    got = pipe.generate_latents_interleaved([dict(prompts="p", negative_prompts="", seed=s) for s in seeds], in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], _oracle_latent(name, sched_kw)[0]) < 1e-4
    assert not torch.equal(got[0], got[1])


def test_pipeline_rejects_values_outside_the_unit_interval():
    pipe = _pipe("cfg2_sd_512x1024", EPS)
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.generate_latents("p", "", **_loop_kw("cfg2_sd_512x1024"), guidance_rescale=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.generate_image("p", "", **_loop_kw("cfg2_sd_512x1024"), guidance_rescale=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.generate_latents_interleaved([dict(prompts="p", seed=1)], **_loop_kw("cfg2_sd_512x1024"), guidance_rescale=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.generate(torch.zeros(1, 4, 32, 64), None, None, guidance_rescale=bad)


def test_verbose_logs_with_rescale():
    """verbose=True keeps the by-products (direction / local) and logs the rescaled reduced-resolution x0: latents unchanged,
    the reference's image_log keys present (``global_img`` comes from ``generate(..., guidance_rescale=)``)."""
    name = "cfg2_sd_512x1024"
    lat = {}
    for verbose in (False, True):
        pipe = _pipe(name, EPS, verbose=verbose, log_freq=2)
        pipe.seed_everything(3)
        imgs, log = pipe.generate_image("p", "", **_loop_kw(name), guidance_rescale=GR, progress=lambda it: it)
        lat[verbose] = pipe.last_latents.clone()
    assert torch.equal(lat[False], lat[True])
    assert set(log) == {"global_img", "global_img_inter_x0_imgs", "intermediate_x0_imgs", "intermediate_cascade_x0_imgs"}
    assert set(log["intermediate_cascade_x0_imgs"]) == {"rrg"}
    assert all(bool(torch.isfinite(z).all()) for z in pipe._logs["rrg_x0"])


def test_generate_with_rescale_vs_cpu_restatement():
    """``generate()`` (ED:761-796): the reference's function with noise_pred_text = cond, on a latent that needs padding."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.G11_CASES["gen_sd_pad_32x64"]
    (un, pun), (co, pco) = synthetic_text_embeds(1)
    text, pooled = torch.cat([un, co]), torch.cat([pun, pco])
    size = (4 * 8 * c["h"], 4 * 8 * c["w"])
    lat = {}
    for gr in (GR, 0.0):
        pipe = ElasticDiffusion(DEV, c["sd"], log_freq=1, unet=FakeUNet(c["sample"]), vae=FakeVAE())
        pipe.default_size = size
        pipe.scheduler.set_timesteps(c["steps"])
        pipe.seed_everything(c["seed"])
        z = torch.randn(1, 4, c["h"], c["w"])
        seen = {}
        dec = pipe.decode_latents
        pipe.decode_latents = lambda lat_, dec=dec, seen=seen: (seen.__setitem__("z", lat_.clone()), dec(lat_))[1]
        _, info = pipe.generate(z, text, pooled, guidance_scale=c["guidance"], guidance_rescale=gr)
        tail = torch.rand(4)
        orc = G.RescaleOracle(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), sd_version=c["sd"])
        orc.default_size = size
        orc.scheduler.set_timesteps(c["steps"])
        orc.seed_everything(c["seed"])
        latent, inter = orc.plain_cfg_generate(torch.randn(1, 4, c["h"], c["w"]), text, pooled, c["guidance"], gr)
        assert rel_l2(seen["z"], latent) < 1e-4, rel_l2(seen["z"], latent)
        assert rel_l2(torch.cat(info["inter_x0"]), torch.cat(inter)) < 1e-4
        assert torch.equal(tail, torch.rand(4))
        lat[gr] = seen["z"]
    assert rel_l2(lat[GR], lat[0.0]) > 1e-3


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_guidance_rescale_flag(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    d = main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1", "--outdir",
              str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4", "--exp", "gr",
              "--guidance_rescale", "0.7"])
    a = np.asarray(Image.open(os.path.join(d, "0.png")), dtype=np.float32)
    assert a.shape == (512, 512, 3) and np.isfinite(a).all()
    assert a.std() > 0  # a NaN latent decodes to a constant image
    assert "guidance_rescale: 0.7" in open(os.path.join(d, "args.txt")).read()
    with pytest.raises(SystemExit):
        main(["--guidance_rescale", "1.5", "--outdir", str(tmp_path)])
