"""-m gpu: the HIP product path (through the C ABI) against the oracle on the same seeded inputs, and against the
golden fixtures produced by the real reference.

Bars (stated per test):
  * kernels fed identical fp32 inputs must be BIT-EXACT against the oracle's torch-CPU op sequence (gathers, selects
    and the fp32 arithmetic kernels, which are compiled without contraction and use the reference's op order);
  * end-to-end latents (the injected fake UNet/VAE run on the GPU: conv/sin differ from the CPU in the last ulp):
    relative L2 < 1e-4 -- ten times tighter than BASELINE.json's 1e-3 target;
  * the host RNG stream must end in exactly the state the reference leaves (torch.rand tail equality).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import elastic_oracle as eo
from oracle.ddim import DDIMOracle
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE, synthetic_text_embeds
from tests.glue_geometries import FUSED_ROWS, PICK_ROWS, SCALAR_IMAGES, VIEW_ROWS, misaligned
from tests.golden import cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gpu_mods():
    from elasticdiffusion_official_amd import geometry, ops, schedule
    return geometry, ops, schedule


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------
# kernels, one by one, bit-exact
# ---------------------------------------------------------------------------------------------------
VIEW_CASES = [(64, 128, 64, None), (128, 256, 128, None), (256, 256, 128, None), (135, 240, 64, None),
              (96, 96, 64, 48), (67, 97, 64, None), (32, 64, 64, None), (128, 192, 128, 32)]
VIEW_CASES += VIEW_ROWS  # crop widths / pad offsets that are no multiple of 4: the scalar gather (tests/glue_geometries.py)


@pytest.mark.parametrize("Hl,Wl,sample,patch", VIEW_CASES)
@pytest.mark.parametrize("B", [1, 2])
def test_gather_views_and_scatter_centres_bit_exact(Hl, Wl, sample, patch, B):
    geometry, ops, _ = _gpu_mods()
    ws = patch if patch is not None else sample // 2
    ctx = sample - ws
    vp = geometry.ViewPlan(Hl, Wl, ws, ws, ctx)
    g = torch.Generator().manual_seed(Hl * 1000 + Wl)
    x = torch.randn(B, 4, Hl, Wl, generator=g)
    # oracle crops
    h_ws = Hl if ws + ctx >= Hl else ws
    w_ws = Wl if ws + ctx >= Wl else ws
    views = eo.get_views(Hl * 8, Wl * 8, h_ws, w_ws, ws)
    assert views == vp.views
    crops, ctxs = [], []
    for v in views:
        c, n4 = eo.crop_with_context(x, *v, 1, ctx // 2)
        crops.append(c)
        ctxs.append(n4)
    assert [tuple(c) for c in ctxs] == [tuple(c) for c in vp.ctx]
    want = torch.cat(crops)  # rows v*B + b
    out = torch.empty(vp.V * B, 4, vp.Sh, vp.Sw, device=DEV)
    ops.gather_views(x.to(DEV), out, dev_i32(vp.win_y0), dev_i32(vp.win_x0), vp.Sh, vp.Sw)
    assert torch.equal(out.cpu(), want)
    # the padded-view call of the pipeline (views smaller than the model): the crop at its offset inside the noise frame, every
    # model dtype; expected by plain slicing, 16-bit values by torch's own round-to-nearest-even
    vpad = geometry.PadPlan(vp.Sh, vp.Sw, sample)
    if vpad.padded:
        frame = torch.randn(4, vpad.PH, vpad.PW, generator=g)
        want_p = frame.unsqueeze(0).repeat(vp.V * B, 1, 1, 1)
        want_p[:, :, vpad.top:vpad.top + vp.Sh, vpad.left:vpad.left + vp.Sw] = want
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            out_p = torch.full((vp.V * B, 4, vpad.PH, vpad.PW), 9.0, device=DEV, dtype=dtype)
            ops.gather_views(x.to(DEV), out_p, dev_i32(vp.win_y0), dev_i32(vp.win_x0), vp.Sh, vp.Sw, vpad.top, vpad.left,
                             frame.to(DEV))
            assert torch.equal(out_p.cpu(), want_p.to(dtype)), dtype
        out_z = torch.full((vp.V * B, 4, vpad.PH, vpad.PW), 9.0, device=DEV)   # without a frame the pad region is zero
        ops.gather_views(x.to(DEV), out_z, dev_i32(vp.win_y0), dev_i32(vp.win_x0), vp.Sh, vp.Sw, vpad.top, vpad.left)
        want_z = torch.zeros_like(want_p)
        want_z[:, :, vpad.top:vpad.top + vp.Sh, vpad.left:vpad.left + vp.Sw] = want
        assert torch.equal(out_z.cpu(), want_z)

    # scatter: predictions with exact zeros sprinkled in, so the value-based first-writer rule is exercised
    pred = torch.randn(vp.V * B, 4, vp.Sh, vp.Sw, generator=g)
    pred[torch.rand(pred.shape, generator=g) < 0.2] = 0.0
    ref = torch.zeros(B, 4, Hl, Wl)
    for k, ((h0, h1, w0, w1), (n_t, n_b, n_l, n_r)) in enumerate(zip(views, ctxs)):
        p = pred[k * B:(k + 1) * B]
        centre = p[:, :, n_t: p.shape[-2] - n_b, n_l: p.shape[-1] - n_r]
        dst = ref[:, :, h0:h1, w0:w1]
        free = dst == 0
        dst[free] = centre[free]
    rb, rs, cb, cs = vp.cover_tables()
    local = torch.full((B, 4, Hl, Wl), 7.0, device=DEV)  # need not be zeroed
    ops.scatter_centres(pred.to(DEV), local, vp.n_col_blocks, dev_i32(rb), dev_i32(rs), dev_i32(cb), dev_i32(cs))
    assert torch.equal(local.cpu(), ref)


PICK_CASES = [(64, 128, 32, 64), (128, 256, 64, 128), (64, 64, 64, 64), (135, 240, 36, 64), (96, 96, 64, 64),
              (67, 97, 44, 64), (256, 256, 128, 128)]
PICK_CASES += PICK_ROWS  # w / pad offsets that are no multiple of 4: the scalar pick and unpad kernels (tests/glue_geometries.py)


@pytest.mark.parametrize("Hl,Wl,h,w", PICK_CASES)
@pytest.mark.parametrize("B", [1, 2])
def test_pick_assemble_and_fill_bit_exact(Hl, Wl, h, w, B):
    """ed_pick_assemble / ed_unpad_direction / ed_fill_directions against the oracle's tensor-level
    random_nearest_downsample + fill chain, with the host sampler producing the picks."""
    geometry, ops, _ = _gpu_mods()
    from elasticdiffusion_official_amd import host_rng
    K = 4
    pp = geometry.PickPlan(Hl, Wl, h, w)
    d = 128 if max(h, w) > 64 else 64
    pad = geometry.PadPlan(h, w, d)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), DDIMOracle())
    torch.manual_seed(5)
    x = torch.randn(B, 4, Hl, Wl)
    frame = torch.randn(4, pad.PH, pad.PW)
    # oracle chain (draws from the global generator)
    torch.manual_seed(99)
    prev, exclude, lows, masks, idxs = None, None, [], [], []
    for k in range(K):
        low, mask, prev = orc.random_nearest_downsample(x, (h, w), prev_random_indices=prev, exclude_mask=exclude,
                                                        drop_p=0.7, nearest=(k == 0))
        if exclude is None:
            exclude = torch.zeros(len(prev), 4, dtype=torch.bool)
        exclude[torch.arange(len(prev)), prev] = True
        lows.append(low), masks.append(mask), idxs.append(prev.clone())
    tail_ref = torch.rand(3)
    # host sampler: same stream
    torch.manual_seed(99)
    stamp = torch.empty(h * w, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(h * w).draw(K, 0.7, lambda: None, stamp=stamp)
    assert torch.equal(torch.rand(3), tail_ref)
    assert torch.equal(idx.long(), torch.stack(idxs))
    # assemble
    rows = torch.empty(K * 2 * B, 4, pad.PH, pad.PW, device=DEV)
    low_dev = torch.empty(K, B, 4, h, w, device=DEV)
    ops.pick_assemble(x.to(DEV), idx.to(DEV), dev_i32(pp.src_row), dev_i32(pp.src_col), rows, h, w, pad.top, pad.left,
                      frame.to(DEV), low_dev)
    assert torch.equal(low_dev.cpu(), torch.stack(lows))
    rows_c = rows.cpu().view(K, 2, B, 4, pad.PH, pad.PW)
    for k in range(K):
        want = frame.unsqueeze(0).repeat(B, 1, 1, 1).clone()
        want[:, :, pad.top:pad.top + h, pad.left:pad.left + w] = lows[k]
        assert torch.equal(rows_c[k, 0], want) and torch.equal(rows_c[k, 1], want)
    # fake model output -> directions
    g = torch.Generator().manual_seed(3)
    out = torch.randn(K * 2 * B, 4, pad.PH, pad.PW, generator=g)
    o = out.view(K, 2, B, 4, pad.PH, pad.PW)[..., pad.top:pad.top + h, pad.left:pad.left + w]
    dirs_ref = o[:, 1] - o[:, 0]
    dirs = torch.empty(K, B, 4, h, w, device=DEV)
    unc = torch.empty(B, 4, h, w, device=DEV)
    ops.unpad_direction(out.to(DEV), dirs, unc, pad.top, pad.left)
    assert torch.equal(dirs.cpu(), dirs_ref) and torch.equal(unc.cpu(), o[K - 1, 0])
    # fill
    target = torch.full((B, 4, Hl, Wl), float("nan")).half()
    for k in range(K):
        target = orc.fill_in_from_downsampled_direction(target, dirs_ref[k], masks[k], fill_all=(k == K - 1))
    low_dir_ref = F.interpolate(target, size=(h, w), mode="nearest")
    tgt = torch.empty(B, 4, Hl, Wl, device=DEV)
    low_dir = torch.empty(B, 4, h, w, device=DEV)
    ops.fill_directions(dirs, stamp.to(DEV), dev_i32(pp.inv_row), dev_i32(pp.inv_col), dev_i32(pp.up_row),
                        dev_i32(pp.up_col), dev_i32(pp.down_row), dev_i32(pp.down_col), tgt, low_dir)
    assert torch.equal(tgt.cpu(), target) and torch.equal(low_dir.cpu(), low_dir_ref)


@pytest.mark.parametrize("shape", [(1, 4, 64, 128), (2, 4, 67, 97), (1, 4, 128, 256)])
@pytest.mark.parametrize("steps,ti", [(50, 0), (50, 49), (10, 3), (4, 1)])
def test_cfg_ddim_and_undo_bit_exact(shape, steps, ti):
    _, ops, schedule = _gpu_mods()
    sch, orc_s = schedule.DDIMSchedule(), DDIMOracle()
    ts = sch.set_timesteps(steps)
    orc_s.set_timesteps(steps)
    assert torch.equal(ts, orc_s.timesteps)
    g = torch.Generator().manual_seed(steps * 100 + ti)
    local, direction, x = (torch.randn(shape, generator=g) for _ in range(3))
    guidance = 10.0 / 3
    out = orc_s.step(local + guidance * direction, ts[ti], x)
    prev, x0 = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    ops.cfg_ddim_step(local.to(DEV), direction.to(DEV), x.to(DEV), prev, x0, np.float32(guidance),
                      *sch.step_coefficients(ts[ti]))
    assert torch.equal(x0.cpu(), out["pred_original_sample"])
    assert torch.equal(prev.cpu(), out["prev_sample"])
    if ti + 1 < steps:
        orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), orc_s)
        torch.manual_seed(1234)
        want = orc.undo_step(out["prev_sample"], ts[ti + 1])
        tail = torch.rand(2)
        from elasticdiffusion_official_amd import host_rng
        torch.manual_seed(1234)
        n_sub = 1000 // steps
        noise = host_rng.draw_noise_into(torch.empty((n_sub,) + shape).pin_memory())
        assert torch.equal(torch.rand(2), tail)
        got = torch.empty(shape, device=DEV)
        ops.undo_step(prev, noise.to(DEV), sch.undo_coefficients(ts[ti + 1]).to(DEV), got)
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("Hl,Wl,h,w", [(64, 128, 32, 64), (128, 256, 64, 128), (67, 97, 44, 64), (96, 96, 64, 64)])
@pytest.mark.parametrize("weight", [1000.0, 437.53, 11.0])
def test_rrg_update_bit_exact(Hl, Wl, h, w, weight):
    geometry, ops, schedule = _gpu_mods()
    sch, orc_s = schedule.DDIMSchedule(), DDIMOracle()
    ts = sch.set_timesteps(50)
    orc_s.set_timesteps(50)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), orc_s)
    g = torch.Generator().manual_seed(int(weight))
    B = 2
    prev, x0 = torch.randn(B, 4, Hl, Wl, generator=g), torch.randn(B, 4, Hl, Wl, generator=g)
    low, unc, ldir = (torch.randn(B, 4, h, w, generator=g) for _ in range(3))
    t = ts[7]
    grad, _ = orc.reduced_resolution_guidance(t, x0, guidance_scale=10.0 / 3, rrg_scale=np.float64(weight),
                                              donwsampled_scores={"latent": low, "uncond_score": unc, "direction": ldir})
    want = prev + grad
    pp = geometry.PickPlan(Hl, Wl, h, w)
    out = torch.empty(B, 4, Hl, Wl, device=DEV)
    sb, sa = sch.step_coefficients(t)[:2]
    ops.rrg_update(prev.to(DEV), x0.to(DEV), low.to(DEV), unc.to(DEV), ldir.to(DEV), dev_i32(pp.up_row),
                   dev_i32(pp.up_col), out, np.float32(10.0 / 3), sb, sa, np.float32(2.0 / (4 * Hl * Wl)),
                   np.float32(weight))
    assert torch.equal(out.cpu(), want)


# The flat kernels hold n = B*4*H*W elements, always a multiple of 4: their scalar forms (k_cfg_ddim_s, k_undo_s, k_rrg_update at
# W % 4 == 0) run only when an operand accessed 16 bytes at a time is not 16-byte aligned.  Same arithmetic per element, so the
# same bits as the all-aligned launch -- which the tests above hold to the oracle.
FLAT_SHAPE = (2, 4, 16, 24)


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_cfg_ddim_misaligned_operand_bit_equal(prediction_type, rescale):
    _, ops, schedule = _gpu_mods()
    sch = schedule.DDIMSchedule()
    coef = sch.step_coefficients(sch.set_timesteps(50)[7])
    g = torch.Generator().manual_seed(41)
    ins = [torch.randn(FLAT_SHAPE, generator=g).to(DEV) for _ in range(3)]   # local, direction, x
    kw = dict(prediction_type=prediction_type)
    if rescale:
        kw.update(ratio=torch.tensor([0.8, 1.1], device=DEV), guidance_rescale=0.7)
    prev, x0 = torch.empty(FLAT_SHAPE, device=DEV), torch.empty(FLAT_SHAPE, device=DEV)
    assert ops.cfg_ddim_step_width(*ins, prev, x0, kw.get("ratio")) == 4
    ops.cfg_ddim_step(*ins, prev, x0, np.float32(10.0 / 3), *coef, **kw)
    assert bool(torch.isfinite(prev).all()) and bool(torch.isfinite(x0).all())
    for k in range(5):                                                       # one operand off a 16-byte boundary at a time
        args = list(ins) + [torch.full(FLAT_SHAPE, 9.0, device=DEV), torch.full(FLAT_SHAPE, 9.0, device=DEV)]
        args[k] = misaligned(args[k])
        assert ops.cfg_ddim_step_width(*args, kw.get("ratio")) == 1
        ops.cfg_ddim_step(*args, np.float32(10.0 / 3), *coef, **kw)
        assert torch.equal(args[3], prev) and torch.equal(args[4], x0), k


def test_undo_step_misaligned_operand_bit_equal():
    _, ops, schedule = _gpu_mods()
    sch = schedule.DDIMSchedule()
    ts = sch.set_timesteps(200)                                              # 5 sub-steps: the 4-unrolled loop and its tail
    coef = sch.undo_coefficients(ts[3]).to(DEV)
    n_sub = coef.numel() // 2
    g = torch.Generator().manual_seed(43)
    x = torch.randn(FLAT_SHAPE, generator=g).to(DEV)
    noise = torch.randn((n_sub,) + FLAT_SHAPE, generator=g).to(DEV)
    want = ops.undo_step(x, noise, coef, torch.empty(FLAT_SHAPE, device=DEV))
    assert n_sub == 5 and bool(torch.isfinite(want).all()) and not torch.equal(want, x)
    for k in range(3):
        args = [x, noise, torch.full(FLAT_SHAPE, 9.0, device=DEV)]
        args[k] = misaligned(args[k])
        got = ops.undo_step(args[0], args[1], coef, args[2])
        assert torch.equal(got, want), k


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_rrg_update_misaligned_operand_bit_equal(prediction_type, rescale):
    geometry, ops, schedule = _gpu_mods()
    sch = schedule.DDIMSchedule()
    sb, sa = sch.step_coefficients(sch.set_timesteps(50)[7])[:2]
    B, C, H, W = FLAT_SHAPE
    h, w = 8, 13
    g = torch.Generator().manual_seed(47)
    prev, x0 = (torch.randn(FLAT_SHAPE, generator=g).to(DEV) for _ in range(2))
    low, unc, ldir = (torch.randn(B, C, h, w, generator=g).to(DEV) for _ in range(3))
    up = dev_i32(geometry.nearest_index_map(h, H)), dev_i32(geometry.nearest_index_map(w, W))
    tail = (np.float32(10.0 / 3), sb, sa, np.float32(2.0 / (4 * H * W)), np.float32(437.53))
    kw = dict(prediction_type=prediction_type)
    if rescale:
        kw.update(ratio_low=torch.tensor([0.8, 1.1], device=DEV), guidance_rescale=0.7)
    want = ops.rrg_update(prev, x0, low, unc, ldir, *up, torch.empty(FLAT_SHAPE, device=DEV), *tail, **kw)
    assert bool(torch.isfinite(want).all()) and not torch.equal(want, prev)
    for k in range(3):
        args = [prev, x0, torch.full(FLAT_SHAPE, 9.0, device=DEV)]
        args[k] = misaligned(args[k])
        got = ops.rrg_update(args[0], args[1], low, unc, ldir, *up, args[2], *tail, **kw)
        assert torch.equal(got, want), k
    # the reduced-resolution operands are read one element at a time in both forms: no alignment condition
    got = ops.rrg_update(prev, x0, misaligned(low), misaligned(unc), misaligned(ldir), *up,
                         torch.full(FLAT_SHAPE, 9.0, device=DEV), *tail, **kw)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", list(cases.G7_CASES))
def test_tiled_decode_vs_golden_and_oracle(golden_dir, name):
    """ed_tile_gather_pad + VAE + ed_tile_accumulate_normalise against the reference's tiled_decode output."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    g = np.load(os.path.join(golden_dir, "g7_tiled_decode.npz"))
    Hl, Wl, sample, low_vram, seed = cases.G7_CASES[name]
    pipe = ElasticDiffusion(DEV, "1.5", unet=FakeUNet(sample), vae=FakeVAE(), low_vram=low_vram)
    z = torch.randn(1, 4, Hl, Wl, generator=torch.Generator().manual_seed(seed))
    img = pipe.tiled_decode(z.to(DEV), tile_batch=3).cpu()
    cases.assert_image_matches(g, name, img, 2e-5)


def test_gather2d_nearest_and_zero_pad():
    geometry, ops, _ = _gpu_mods()
    x = torch.randn(2, 3, 20, 28)
    rows = geometry.nearest_index_map(20, 33)
    cols = geometry.nearest_index_map(28, 50)
    want = F.interpolate(x, size=(33, 50), mode="nearest")
    R = np.stack([rows, rows])
    Cc = np.stack([cols, cols])
    R[1, :3] = -1  # zero rows
    want[1, :, :3] = 0
    out = torch.empty(2, 3, 33, 50, device=DEV)
    ops.gather2d(x.to(DEV), out, dev_i32([0, 1]), dev_i32(R), dev_i32(Cc))
    assert torch.equal(out.cpu(), want)
    out16 = torch.empty(2, 3, 33, 50, device=DEV, dtype=torch.bfloat16)
    ops.gather2d(x.to(DEV), out16, dev_i32([0, 1]), dev_i32(R), dev_i32(Cc))
    assert torch.equal(out16.cpu(), want.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_model_boundary_dtypes(dtype):
    """16-bit model tensors: stores round to nearest even like torch, loads widen exactly."""
    geometry, ops, _ = _gpu_mods()
    vp = geometry.ViewPlan(64, 128, 32, 32, 32)
    x = torch.randn(1, 4, 64, 128)
    out = torch.empty(vp.V, 4, vp.Sh, vp.Sw, device=DEV, dtype=dtype)
    ops.gather_views(x.to(DEV), out, dev_i32(vp.win_y0), dev_i32(vp.win_x0), vp.Sh, vp.Sw)
    ref32 = torch.empty(vp.V, 4, vp.Sh, vp.Sw, device=DEV)
    ops.gather_views(x.to(DEV), ref32, dev_i32(vp.win_y0), dev_i32(vp.win_x0), vp.Sh, vp.Sw)
    assert torch.equal(out.cpu(), ref32.cpu().to(dtype))
    pred = torch.randn(vp.V, 4, vp.Sh, vp.Sw).to(dtype)
    rb, rs, cb, cs = vp.cover_tables()
    a = torch.empty(1, 4, 64, 128, device=DEV)
    b = torch.empty(1, 4, 64, 128, device=DEV)
    ops.scatter_centres(pred.to(DEV), a, vp.n_col_blocks, dev_i32(rb), dev_i32(rs), dev_i32(cb), dev_i32(cs))
    ops.scatter_centres(pred.float().to(DEV), b, vp.n_col_blocks, dev_i32(rb), dev_i32(rs), dev_i32(cb), dev_i32(cs))
    assert torch.equal(a.cpu(), b.cpu())


def test_cpu_tensors_are_rejected_loudly():
    _, ops, _ = _gpu_mods()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cfg_ddim_step(*(torch.zeros(8) for _ in range(5)), 1.0, 1.0, 1.0, 1.0, 1.0)


# ---------------------------------------------------------------------------------------------------
# end to end: product (GPU) vs oracle (CPU) vs golden (real reference)
# ---------------------------------------------------------------------------------------------------
def _embed_fn(xl):
    (un, pun), (co, pco) = synthetic_text_embeds(1, xl=xl)
    state = {"n": 0}

    def fn(_):
        state["n"] += 1
        return (un, pun) if state["n"] % 2 == 1 else (co, pco)

    return fn


@pytest.mark.parametrize("name", list(cases.E2E_CASES))
def test_end_to_end_vs_oracle_and_golden(golden_dir, name):
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.E2E_CASES[name]
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    xl = c["sd"].startswith("XL")
    cn = c.get("controlnet", False)
    kw = dict(cases.E2E_KW)
    kw.update(c.get("kw", {}))
    ckw = {}
    if cn:
        ds = eo.get_downsample_size(c["H"], c["W"], c["sd"])
        ckw = dict(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)
    pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            text_encoder=_embed_fn(xl), controlnet=FakeControlNet() if cn else None)
    if c.get("patch") is not None:
        pipe.set_view_config(c["patch"])
    pipe.seed_everything(c["seed"])
    imgs, log = pipe.generate_image("p", "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                                    resampling_steps=c["R"], tiled_decoder=bool(c.get("tiled")), output_type="pt",
                                    **kw, **ckw)
    tail = torch.rand(4)
    z = pipe.last_latents.cpu()
    want = torch.from_numpy(g[f"{name}/latent"])
    assert z.shape == want.shape
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    if c.get("keep_image"):
        cases.assert_image_matches(g, name, imgs, 1e-3)
    # the host generators end in exactly the reference's state
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/rng_tail"])
    assert log == {}


def test_pil_output_and_api_surface():
    from elasticdiffusion_official_amd import ElasticDiffusion
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=_embed_fn(False))
    pipe.seed_everything(0)
    imgs, log = pipe.generate_image(prompts="a", negative_prompts="", height=512, width=768, num_inference_steps=2,
                                    resampling_steps=1)
    assert len(imgs) == 1 and imgs[0].size == (768, 512) and imgs[0].mode == "RGB" and log == {}
    assert pipe.get_downsample_size(1024, 2048) == (32, 64)
    assert pipe.get_views(512, 1024, 32, 32, 32)[1] == (0, 32, 32, 64)
    with pytest.raises(ValueError):
        pipe.generate_image("a", height=515, width=512, num_inference_steps=1)


def test_cpu_device_is_rejected():
    from elasticdiffusion_official_amd import ElasticDiffusion
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ElasticDiffusion(torch.device("cpu"), "1.5", unet=FakeUNet(64), vae=FakeVAE())


def _embed_fn_batch(B, xl=False):
    (un, pun), (co, pco) = synthetic_text_embeds(B, xl=xl)
    state = {"n": 0}

    def fn(_):
        state["n"] += 1
        return (un, pun) if state["n"] % 2 == 1 else (co, pco)

    return fn


@pytest.mark.parametrize("sd,sample,H,W,B,R,patch", [
    ("1.5", 64, 512, 768, 2, 1, None),      # batch of two prompts: rows are (view, prompt) ordered
    ("1.5", 64, 256, 512, 1, 2, None),      # latent 32x64: one dimension smaller than the model -> padded VIEWS too
    ("1.5", 64, 1080, 1920, 1, 1, None),    # windows do not tile: overlapping centres, fractional reduction 135 -> 36
    ("XL1.0", 128, 1024, 1536, 2, 1, 96),   # SDXL geometry, custom patch size, two prompts
    # sizes whose rows leave the 4-wide kernels (tests/glue_geometries.py: SCALAR_IMAGES, classes (px4, gx4))
    SCALAR_IMAGES["ff_one_view"] + (1, 1, None),    # 512x304: FF, one padded view, both pad offsets 13
    SCALAR_IMAGES["ff_views"] + (2, 2, None),       # 768x432: FF, Sw = 54 at offset 5, w = 36 at offset 14
    SCALAR_IMAGES["ft"] + (2, 2, None),             # 520x256: FT, w = 31
    SCALAR_IMAGES["tf"] + (1, 1, None),             # 528x272: TF, Sw = 34 at offset 15
    SCALAR_IMAGES["ff_xl"] + (1, 1, None),          # 1024x600 SDXL: FF, offset 26
    SCALAR_IMAGES["ft_many"] + (1, 1, None),        # 1920x1080 portrait: FT, 40 views overlapping on both axes
])
def test_edge_geometries_and_prompt_batches_vs_oracle(sd, sample, H, W, B, R, patch):
    """No golden for these: the oracle runs on the CPU in the test (seconds).  rel-L2 < 1e-4, identical RNG end state."""
    _edge_run_vs_oracle(sd, sample, H, W, B, R, patch)


def test_controlnet_condition_views_at_an_odd_pad_offset_vs_oracle():
    """768x432 with a ControlNet: the condition rows are cut by ed_gather2d for views of Sw = 54 at v_off_x = 5 and picks of
    w = 36 at g_off_x = 14 (pixel offsets 40 and 112), next to latent rows assembled by the scalar forms.  The bar of
    test_edge_geometries_and_prompt_batches_vs_oracle."""
    _edge_run_vs_oracle(*SCALAR_IMAGES["ff_views"], 1, 1, None, controlnet=True)


def _edge_run_vs_oracle(sd, sample, H, W, B, R, patch, controlnet=False):
    from elasticdiffusion_official_amd import ElasticDiffusion
    xl = sd.startswith("XL")
    kw = dict(height=H, width=W, num_inference_steps=2, guidance_scale=10.0, resampling_steps=R, new_p=0.3,
              rrg_stop_t=0.4, rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
    if controlnet:
        ds = eo.get_downsample_size(H, W, sd)
        kw.update(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)
    prompts = ["p%d" % i for i in range(B)]
    pipe = ElasticDiffusion(DEV, sd, view_batch_size=3, unet=FakeUNet(sample, xl=xl), vae=FakeVAE(),
                            text_encoder=_embed_fn_batch(B, xl), controlnet=FakeControlNet() if controlnet else None)
    orc = eo.ElasticOracle(FakeUNet(sample, xl=xl), FakeVAE(), DDIMOracle(), _embed_fn_batch(B, xl), sd_version=sd,
                           view_batch_size=3, pooled_dim=16 if xl else None, controlnet=FakeControlNet() if controlnet else None)
    if patch is not None:
        pipe.set_view_config(patch)
        orc.set_view_config(patch)
    pipe.seed_everything(5)
    z = pipe.generate_latents(prompts, "", **kw).cpu()
    tail = torch.rand(3)
    orc.seed_everything(5)
    want = orc.generate_latent(prompts, "", **kw)
    assert z.shape == want.shape == (B, 4, H // 8, W // 8)
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert torch.equal(tail, torch.rand(3))


def test_interleaved_images_equal_running_each_alone():
    """generate_latents_interleaved: three images (different prompts / seeds), two in flight -- the 20-row phase of one
    fused with the RePaint phase of the other into one forward with per-row timesteps.  Every image must come out as
    if it had run alone with seed_everything(seed) (its own host RNG stream), and the caller's RNG state is untouched."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    kw = dict(height=512, width=1024, num_inference_steps=3, guidance_scale=10.0, resampling_steps=2, new_p=0.3,
              rrg_stop_t=0.4, rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
    def embed(prompts):  # prompt-dependent deterministic embeddings of the fake model's width
        out = []
        for p in ([prompts] if isinstance(prompts, str) else prompts):
            g = torch.Generator().manual_seed(sum(p.encode()) + 1)
            out.append(torch.randn(1, 77, 32, generator=g))
        e = torch.cat(out)
        return e, e

    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=embed)
    jobs = [dict(prompts="a cat", negative_prompts="blurry", seed=11), dict(prompts="a dog", seed=12),
            dict(prompts=["two", "prompts"], seed=13)]
    alone = []
    for j in jobs:
        pipe.seed_everything(j["seed"])
        alone.append(pipe.generate_latents(j["prompts"], j.get("negative_prompts", ""), **kw).clone())
    torch.manual_seed(777)
    np.random.seed(777)
    done = []
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, on_done=lambda i, z: done.append(i), **kw)
    assert torch.equal(torch.rand(3), torch.manual_seed(777) and torch.rand(3))  # outer torch stream untouched
    assert sorted(done) == [0, 1, 2] and pipe.ticks < 3 * (2 * 3 - 1)           # calls were actually fused
    for z, want in zip(got, alone):
        assert z.shape == want.shape
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert pipe._runner.stats()["eager"] == 0


# ---------------------------------------------------------------------------------------------------
# fused glue (ed_assemble_rows / ed_phase_epilogue) == the chain of separate entry points, bit for bit
# ---------------------------------------------------------------------------------------------------
FUSED_CASES = [  # Hl, Wl, h, w, model size d, patch
    (64, 128, 32, 64, 64, None),      # cfg2: padded global rows
    (128, 256, 64, 128, 128, None),   # cfg3
    (256, 256, 128, 128, 128, None),  # cfg4: 16 views, no padding
    (67, 97, 44, 64, 64, None),       # ragged: overlapping centres, fractional reduction, odd latent width; w = gPW = Sw = 64 and
                                      # no x offsets, so every row kernel is 4-wide here (only ed_rrg_update is scalar, W = 97)
    (32, 64, 32, 64, 64, None),       # views smaller than the model: padded VIEW rows too, separate row shapes
    (96, 96, 64, 64, 64, 48),         # custom patch size
]
FUSED_CASES += FUSED_ROWS  # the scalar classes (px4, gx4) = FF, FT, TF of ed_assemble_rows and odd offsets in the epilogue


@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_CASES)
@pytest.mark.parametrize("B,K,dtype", [(1, 4, torch.float32), (2, 1, torch.bfloat16), (1, 8, torch.float16)])
def test_fused_glue_equals_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype):
    geometry, ops, schedule = _gpu_mods()
    from elasticdiffusion_official_amd import host_rng
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    g = torch.Generator().manual_seed(Hl * 131 + Wl + K)
    x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    gframe = torch.randn(4, gpad.PH, gpad.PW, generator=g).to(DEV) if gpad.padded else None
    vframe = torch.randn(4, vpad.PH, vpad.PW, generator=g).to(DEV) if vpad.padded else None
    torch.manual_seed(17)
    stamp = torch.empty(h * w, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(h * w).draw(K, 0.7, lambda: None, stamp=stamp).to(DEV)
    stamp = stamp.to(DEV)
    T = {k: dev_i32(getattr(pp, k)) for k in ("src_row", "src_col", "inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")}
    wy, wx = dev_i32(vp.win_y0), dev_i32(vp.win_x0)
    cover = tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left))
    n_g, n_v = 2 * K * B, vp.V * B
    # ---- assemble: separate vs fused ----
    def rows():
        return (torch.full((n_g, 4, gpad.PH, gpad.PW), 9.0, device=DEV, dtype=dtype),
                torch.full((n_v, 4, vpad.PH, vpad.PW), 9.0, device=DEV, dtype=dtype))
    g1, v1 = rows()
    low1 = torch.empty(K, B, 4, h, w, device=DEV)
    ops.pick_assemble(x, idx, T["src_row"], T["src_col"], g1, h, w, gpad.top, gpad.left, gframe, low1)
    ops.gather_views(x, v1, wy, wx, vp.Sh, vp.Sw, vpad.top, vpad.left, vframe)
    g2, v2 = rows()
    low2 = torch.empty(K, B, 4, h, w, device=DEV)
    ops.assemble_rows(x, idx, T["src_row"], T["src_col"], g2, h, w, gpad.top, gpad.left, gframe, low2, v2, wy, wx, vp.Sh,
                      vp.Sw, vpad.top, vpad.left, vframe)
    assert torch.equal(g1, g2) and torch.equal(v1, v2) and torch.equal(low1, low2)
    # ---- epilogue: separate chain vs fused (model outputs with exact zeros so first-writer-wins is exercised) ----
    g_out = torch.randn(n_g, 4, gpad.PH, gpad.PW, generator=g).to(dtype).to(DEV)
    v_cpu = torch.randn(n_v, 4, vpad.PH, vpad.PW, generator=g)
    v_cpu[torch.rand(v_cpu.shape, generator=g) < 0.2] = 0.0
    v_out = v_cpu.to(dtype).to(DEV)
    sch = schedule.DDIMSchedule()
    ts = sch.set_timesteps(50)
    coef = sch.step_coefficients(ts[7])
    guidance, w_rrg, norm = np.float32(10.0 / 3), np.float32(437.53), np.float32(2.0 / (4 * Hl * Wl))
    dirs = torch.empty(K, B, 4, h, w, device=DEV)
    unc1, ldir1 = torch.empty(B, 4, h, w, device=DEV), torch.empty(B, 4, h, w, device=DEV)
    direction1, local1 = torch.empty_like(x), torch.empty_like(x)
    prev1, x01, nxt1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ops.unpad_direction(g_out, dirs, unc1, gpad.top, gpad.left)
    ops.fill_directions(dirs, stamp, T["inv_row"], T["inv_col"], T["up_row"], T["up_col"], T["down_row"], T["down_col"],
                        direction1, ldir1)
    ops.scatter_centres(v_out, local1, vp.n_col_blocks, *cover)
    ops.cfg_ddim_step(local1, direction1, x, prev1, x01, guidance, *coef)
    ops.rrg_update(prev1, x01, low1[K - 1], unc1, ldir1, T["up_row"], T["up_col"], nxt1, guidance, coef[0], coef[1], norm, w_rrg)
    out = {k: torch.full_like(x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    unc2, ldir2 = torch.full_like(unc1, 5.0), torch.full_like(ldir1, 5.0)
    ops.phase_epilogue(g_out, v_out, x, stamp, tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")),
                       cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance, coef, out["prev"], out["x0"],
                       low_dir=ldir2, uncond_last=unc2, direction=out["direction"], local=out["local"],
                       x_next=out["x_next"], low_latent=low1[K - 1], rrg_norm=norm, rrg_weight=w_rrg)
    for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1)):
        assert torch.equal(out[name], want), name
    assert torch.equal(unc2, unc1) and torch.equal(ldir2, ldir1)
    # optional outputs may be omitted
    p3, z3 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")),
                       cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance, coef, p3, z3)
    assert torch.equal(p3, prev1) and torch.equal(z3, x01)


@pytest.mark.parametrize("name", ["cfg2_sd_512x1024", "cfg3_xl_1024x2048", "overlap_536x776"])
def test_end_to_end_with_separate_glue_kernels(golden_dir, name):
    """The un-fused glue path (FUSED_GLUE = False) still reproduces the reference goldens, and the fused default gives
    the SAME latents bit for bit (same fp32 operation order)."""
    from elasticdiffusion_official_amd import ElasticDiffusion, pipeline
    c = cases.E2E_CASES[name]
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    xl = c["sd"].startswith("XL")
    kw = dict(cases.E2E_KW)
    kw.update(c.get("kw", {}))
    lat = {}
    for fused in (False, True):
        pipeline.FUSED_GLUE = fused
        try:
            pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                                    text_encoder=_embed_fn(xl))
            pipe.seed_everything(c["seed"])
            lat[fused] = pipe.generate_latents("p", "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                                               resampling_steps=c["R"], **kw).cpu()
        finally:
            pipeline.FUSED_GLUE = True
    assert rel_l2(lat[False], torch.from_numpy(g[f"{name}/latent"])) < 1e-4
    assert torch.equal(lat[False], lat[True])


# ---------------------------------------------------------------------------------------------------
# generate() and the verbose image logs (ED:761-796, 1092-1118)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.G11_CASES))
def test_generate_vs_reference_golden(golden_dir, name):
    """The reference's plain CFG + DDIM ``generate`` (its verbose "global_img"), incl. the noised-background padding of
    a latent smaller than the model and the per-strip reseed side effects on the host generators."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.G11_CASES[name]
    g = np.load(os.path.join(golden_dir, "g11_generate.npz"))
    xl = c["sd"].startswith("XL")
    (un, pun), (co, pco) = synthetic_text_embeds(1, xl=xl)
    pipe = ElasticDiffusion(DEV, c["sd"], log_freq=1, unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE())
    pipe.default_size = (4 * 8 * c["h"], 4 * 8 * c["w"])
    pipe.scheduler.set_timesteps(c["steps"])
    pipe.seed_everything(c["seed"])
    z = torch.randn(1, 4, c["h"], c["w"])
    seen = {}
    dec = pipe.decode_latents
    pipe.decode_latents = lambda lat: (seen.__setitem__("z", lat.clone()), dec(lat))[1]
    img, info = pipe.generate(z, torch.cat([un, co]), torch.cat([pun, pco]), guidance_scale=c["guidance"])
    tail = torch.rand(4)
    assert img.size == (c["w"] * 8, c["h"] * 8)
    assert rel_l2(seen["z"], torch.from_numpy(g[f"{name}/final"])) < 1e-4
    assert rel_l2(torch.cat(info["inter_x0"]), torch.from_numpy(g[f"{name}/inter_x0"])) < 1e-4
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/rng_tail"])


def test_verbose_image_log():
    """verbose=True: the reference's image_log keys (ED:1092-1118), PIL grids of the right size; latents unchanged."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    kw = dict(height=512, width=1024, num_inference_steps=4, guidance_scale=10.0, resampling_steps=2, new_p=0.3,
              rrg_stop_t=0.4, rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
    lat = {}
    for verbose in (False, True):
        pipe = ElasticDiffusion(DEV, "1.5", verbose=verbose, log_freq=2, view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(),
                                text_encoder=_embed_fn(False))
        pipe.seed_everything(3)
        imgs, log = pipe.generate_image("p", "", **kw)
        lat[verbose] = pipe.last_latents.clone()
    assert torch.equal(lat[False], lat[True])
    assert set(log) == {"global_img", "global_img_inter_x0_imgs", "intermediate_x0_imgs", "intermediate_cascade_x0_imgs"}
    assert log["global_img"].size == (512, 256)                      # the reduced-resolution generation (32x64 latent)
    assert log["intermediate_x0_imgs"].size == (2 * 1026 + 2, 516)  # 2 logged steps in make_grid's padded layout
    assert set(log["intermediate_cascade_x0_imgs"]) == {"rrg"}


def test_verbose_init_low_matches_oracle():
    """ED:1023-1024 with RePaint on (the default): the latent the verbose ``global_img`` is generated from is the reduced
    latent of the FIRST phase (nearest downsample of the initial noise), not the RePaint phase's."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    kw = dict(height=512, width=1024, num_inference_steps=3, guidance_scale=10.0, resampling_steps=2, new_p=0.3,
              rrg_stop_t=0.4, rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
    pipe = ElasticDiffusion(DEV, "1.5", verbose=True, log_freq=2, view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(),
                            text_encoder=_embed_fn(False))
    pipe.seed_everything(23)
    pipe.generate_latents("p", "", **kw)
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), DDIMOracle(), _embed_fn(False), sd_version="1.5", view_batch_size=4)
    orc.seed_everything(23)
    logs = {}
    orc.generate_latent("p", "", logs=logs, **kw)
    assert torch.equal(pipe._logs["init_low"].cpu(), logs["init_downsampled_latent"])


@pytest.mark.parametrize("cls_name", ["LinearScheduler", "ConstScheduler"])
def test_other_rrg_schedulers_vs_oracle(cls_name):
    """``rrg_scherduler_cls`` other than the cosine default (ED:73-94, 972-979): the product path's own classes and the
    oracle's give the same latents (rel-L2 < 1e-4) and RNG end state."""
    import elasticdiffusion_official_amd as pkg
    from elasticdiffusion_official_amd import ElasticDiffusion
    kw = dict(height=512, width=768, num_inference_steps=4, guidance_scale=10.0, resampling_steps=2, new_p=0.3,
              rrg_stop_t=0.4, rrg_init_weight=600, cosine_scale=10.0, repaint_sampling=True)
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=3, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=_embed_fn(False))
    orc = eo.ElasticOracle(FakeUNet(64), FakeVAE(), DDIMOracle(), _embed_fn(False), sd_version="1.5", view_batch_size=3)
    pipe.seed_everything(31)
    z = pipe.generate_latents("p", "", rrg_scherduler_cls=getattr(pkg, cls_name), **kw).cpu()
    tail = torch.rand(3)
    orc.seed_everything(31)
    want = orc.generate_latent("p", "", rrg_scherduler_cls=getattr(eo, cls_name), **kw)
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert torch.equal(tail, torch.rand(3))
