"""-m gpu: regional prompts through the HIP path.

Bars (the project's existing ones):
  * ``ed_region_weights``: BIT-EXACT against the torch-CPU op sequence of tests/regional_cpu.py, 4-wide and scalar forms;
  * ``ed_assemble_rows_n``: bit-identical to ``ed_assemble_rows`` / ``ed_assemble_rows_x`` at copies = 2, and to their rows
    duplicated at copies = 4;
  * the fused regional epilogue: bit-identical to the chain of separate kernels run once per region on its (uncond, cond_p) pair
    rows plus ``ed_region_blend``; the std ratios of the fused reduction within 2 ulp of the chain's (a reduction in another order);
  * end to end against ``RegionalOracle``: latent rel-L2 < 1e-4 and the host RNG stream in exactly the same end state; fused and
    un-fused glue the same bits; interleaved against alone 1e-5;
  * a run without ``regions`` launches exactly the entry points it launched before and gives the same bits.
"""
import os

import numpy as np
import pytest
import torch

from tests import regional_cpu as RG
from tests.dpm_solver_cpu import DPMSolverCPU
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
from tests.glue_geometries import FUSED_ROWS, misaligned
from tests.golden import cases
from tests.test_hip_parity import DEV, dev_i32, rel_l2

pytestmark = pytest.mark.gpu

ULP2 = 2.4e-7   # 2 ulp of fp32, relative (tests/test_guidance_rescale_gpu.py)
GR = 0.7
V_TRAILING_ZSNR = dict(prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True)
REGIONAL_ENTRY_POINTS = ("ed_region_weights", "ed_assemble_rows_n", "ed_region_blend", "ed_phase_epilogue_rg", "ed_phase_moments_rg")


def _mods():
    from elasticdiffusion_official_amd import geometry, host_rng, ops, schedule
    return geometry, host_rng, ops, schedule


# ---------------------------------------------------------------------------------------------------
# ed_region_weights
# ---------------------------------------------------------------------------------------------------
def _masks(n, Hl, Wl, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 256, (n, Hl, Wl), generator=g, dtype=torch.uint8)
    sel = torch.rand(n, Hl, Wl, generator=g)
    m[sel < 0.3] = 0          # uncovered, one-hot and overlapping pixels all occur
    m[sel > 0.7] = 255
    return m


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("Hl,Wl", [(1, 1), (3, 5), (64, 128), (67, 97)])
def test_region_weights_bit_exact(n, Hl, Wl):
    """64 x 128 takes the 4-pixel form; 1 x 1, 3 x 5 and 67 x 97 (pixel counts that are no multiple of 4) and a mask buffer one
    byte off a 4-byte boundary the scalar one"""
    _, _, ops, _ = _mods()
    masks = _masks(n, Hl, Wl, 100 * n + Hl)
    weights = [1.0, 2.0, 0.5, 3.25, 1.0, 0.75, 1.5][:n]
    want = RG.region_weights(masks, weights)
    got = ops.region_weights(masks.to(DEV), weights)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n + 1, Hl, Wl)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    off = ops.region_weights(misaligned(masks), weights, out=misaligned(torch.empty(n + 1, Hl, Wl)))
    assert torch.equal(off.cpu().view(torch.int32), want.view(torch.int32))
    # one-hot coverage: exactly 1.0 / 0.0
    hot = torch.zeros(n, Hl, Wl, dtype=torch.uint8)
    hot[0] = 255
    w = ops.region_weights(hot.to(DEV), weights).cpu()
    assert torch.equal(w[1], torch.ones(Hl, Wl)) and float(w[0].abs().max()) == 0.0 and float(w[2:].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------
# ed_assemble_rows_n
# ---------------------------------------------------------------------------------------------------
def _geometry(Hl, Wl, h, w, d, patch):
    geometry = _mods()[0]
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    T = {k: dev_i32(getattr(pp, k)) for k in ("src_row", "src_col", "inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")}
    T["win_y0"], T["win_x0"] = dev_i32(vp.win_y0), dev_i32(vp.win_x0)
    return pp, vp, gpad, vpad, T


def _picks(h, w, K):
    host_rng = _mods()[1]
    torch.manual_seed(17)
    stamp = torch.empty(h * w, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(h * w).draw(K, 0.7, lambda: None, stamp=stamp).to(DEV)
    return idx, stamp.to(DEV)


@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_ROWS)
@pytest.mark.parametrize("B,K,dtype", [(1, 3, torch.float32), (2, 2, torch.float16)])
def test_assemble_rows_n_equals_pair_rows(Hl, Wl, h, w, d, patch, B, K, dtype):
    _, _, ops, _ = _mods()
    pp, vp, gpad, vpad, T = _geometry(Hl, Wl, h, w, d, patch)
    g = torch.Generator().manual_seed(Hl + 7 * Wl)
    x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    gframe = torch.randn(4, gpad.PH, gpad.PW, generator=g).to(DEV)
    vframe = torch.randn(4, vpad.PH, vpad.PW, generator=g).to(DEV)
    idx, _ = _picks(h, w, K)
    geo = lambda g_rows, low, v_rows: (x, idx, T["src_row"], T["src_col"], g_rows, h, w, gpad.top, gpad.left, gframe, low, v_rows,  # noqa: E731
                                       T["win_y0"], T["win_x0"], vp.Sh, vp.Sw, vpad.top, vpad.left, vframe)

    def rows(copies, C=4):
        return (torch.full((K * copies * B, C, gpad.PH, gpad.PW), 9.0, device=DEV, dtype=dtype),
                torch.full((K, B, 4, h, w), 9.0, device=DEV), torch.full((vp.V * B, C, vpad.PH, vpad.PW), 9.0, device=DEV, dtype=dtype))

    g2, low2, v2 = rows(2)
    ops.assemble_rows(*geo(g2, low2, v2))
    gn, lown, vn = rows(2)
    ops.assemble_rows_n(*geo(gn, lown, vn), 2)
    assert torch.equal(gn, g2) and torch.equal(lown, low2) and torch.equal(vn, v2)
    g4, low4, v4 = rows(4)
    ops.assemble_rows_n(*geo(g4, low4, v4), 4)
    pair = g2.view(K, 2, B, 4, gpad.PH, gpad.PW)
    assert torch.equal(g4.view(K, 4, B, 4, gpad.PH, gpad.PW), pair[:, :1].expand(-1, 4, -1, -1, -1, -1))
    assert torch.equal(pair[:, 0], pair[:, 1]) and torch.equal(low4, low2) and torch.equal(v4, v2)
    # with E = 5 extra channels: ed_assemble_rows_x's bits at copies = 2, its rows three times at copies = 3
    extra = torch.randn(B, 5, Hl, Wl, generator=g).to(DEV)
    pad_value = torch.tensor([1.0, 0.0, 0.25, -2.0, 0.0]).to(DEV)
    gx, lowx, vx = rows(2, 9)
    ops.assemble_rows_x(*geo(gx, lowx, vx), extra, pad_value)
    gy, lowy, vy = rows(2, 9)
    ops.assemble_rows_n(*geo(gy, lowy, vy), 2, extra, pad_value)
    assert torch.equal(gy, gx) and torch.equal(lowy, lowx) and torch.equal(vy, vx)
    g3, low3, v3 = rows(3, 9)
    ops.assemble_rows_n(*geo(g3, low3, v3), 3, extra, pad_value)
    assert torch.equal(g3.view(K, 3, B, 9, gpad.PH, gpad.PW), gx.view(K, 2, B, 9, gpad.PH, gpad.PW)[:, :1].expand(-1, 3, -1, -1, -1, -1))
    assert torch.equal(v3, vx) and torch.equal(low3, lowx)


# ---------------------------------------------------------------------------------------------------
# the fused regional epilogue == the chain of separate kernels per region + ed_region_blend, bit for bit
# ---------------------------------------------------------------------------------------------------
class _Case:
    """model output rows of K steps x (1 + P) rows x B samples on one geometry, and the region weights"""

    def __init__(self, Hl, Wl, h, w, d, patch, B, K, dtype, P, weights=None):
        _, _, ops, _ = _mods()
        self.pp, self.vp, self.gpad, self.vpad, self.T = _geometry(Hl, Wl, h, w, d, patch)
        self.B, self.K, self.P, self.h, self.w, self.Hl, self.Wl = B, K, P, h, w, Hl, Wl
        g = torch.Generator().manual_seed(Hl * 131 + Wl + K + 1000 * P)
        self.x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
        self.x0h = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
        self.idx, self.stamp = _picks(h, w, K)
        T, gpad, vpad, vp = self.T, self.gpad, self.vpad, self.vp
        self.cover = tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left))
        self.pick = tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col"))
        pair = torch.empty(2 * K * B, 4, gpad.PH, gpad.PW, device=DEV, dtype=dtype)
        self.low = torch.empty(K, B, 4, h, w, device=DEV)
        ops.pick_assemble(self.x, self.idx, T["src_row"], T["src_col"], pair, h, w, gpad.top, gpad.left, None, self.low)
        self.g_out = (torch.randn(K * (1 + P) * B, 4, gpad.PH, gpad.PW, generator=g) + 0.5).to(dtype).to(DEV)
        v_cpu = torch.randn(vp.V * B, 4, vpad.PH, vpad.PW, generator=g) - 1.5
        v_cpu[torch.rand(v_cpu.shape, generator=g) < 0.2] = 0.0
        self.v_out = v_cpu.to(dtype).to(DEV)
        if weights is not None:
            self.region_w = weights.to(DEV).contiguous()
        elif P == 1:
            self.region_w = torch.ones(1, Hl, Wl, device=DEV)
        else:
            self.region_w = ops.region_weights(_masks(P - 1, Hl, Wl, Hl + P).to(DEV), [1.0, 2.0, 0.5][:P - 1])
        self.guidance, self.w_rrg, self.norm = np.float32(10.0 / 3), np.float32(437.53), np.float32(2.0 / (4 * Hl * Wl))
        self.geo = (vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, self.guidance)

    def pair_rows(self, p):
        K, B, P, gpad = self.K, self.B, self.P, self.gpad
        g6 = self.g_out.view(K, 1 + P, B, 4, gpad.PH, gpad.PW)
        return g6[:, [0, 1 + p]].reshape(2 * K * B, 4, gpad.PH, gpad.PW).contiguous()

    def directions(self):
        """the un-fused chain up to the class direction: -> (direction, low_dir, uncond_last, local)"""
        _, _, ops, _ = _mods()
        T, B, K, P, h, w = self.T, self.B, self.K, self.P, self.h, self.w
        full = torch.empty(P, B, 4, self.Hl, self.Wl, device=DEV)
        lows = torch.empty(P, B, 4, h, w, device=DEV)
        dirs, unc = torch.empty(K, B, 4, h, w, device=DEV), torch.empty(B, 4, h, w, device=DEV)
        for p in range(P):
            ops.unpad_direction(self.pair_rows(p), dirs, unc, self.gpad.top, self.gpad.left)
            ops.fill_directions(dirs, self.stamp, *self.pick, full[p], lows[p])
        direction = ops.region_blend(full, self.region_w)
        w_low = self.region_w[:, T["down_row"].long()][:, :, T["down_col"].long()].contiguous()
        low_dir = ops.region_blend(lows, w_low)
        local = torch.empty_like(self.x)
        ops.scatter_centres(self.v_out, local, self.vp.n_col_blocks, *self.cover)
        return direction, low_dir, unc, local


def _close(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return bool(((got - want).abs() <= ULP2 * want.abs()).all())


def _fused(c, coef, pt, rs=None, ms=None, rrg=True, by_products=True, g_out=None, region_w=None, x_shape=None):
    """ops.phase_epilogue with region_w -> dict of every output (sentinel 5.0 where it is not written)"""
    _, _, ops, _ = _mods()
    out = {k: torch.full_like(c.x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    out["uncond_last"], out["low_dir"] = (torch.full((c.B, 4, c.h, c.w), 5.0, device=DEV) for _ in range(2))
    kw = dict(prediction_type=pt, region_w=c.region_w if region_w is None else region_w)
    if by_products:
        kw.update(low_dir=out["low_dir"], uncond_last=out["uncond_last"], direction=out["direction"], local=out["local"])
    if rrg:
        kw.update(x_next=out["x_next"], low_latent=c.low[c.K - 1], rrg_norm=c.norm, rrg_weight=c.w_rrg)
    if rs is not None:
        kw.update(ratio=rs[0], ratio_low=rs[1] if rrg else None, guidance_rescale=GR)
    if ms is not None:
        kw.update(multistep=ms)
    ops.phase_epilogue(c.g_out if g_out is None else g_out, c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, coef, out["prev"],
                       out["x0"], **kw)
    return out


@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_ROWS)
@pytest.mark.parametrize("B,K,dtype", [(1, 4, torch.float32), (2, 1, torch.bfloat16), (1, 8, torch.float16)])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_fused_regional_epilogue_equals_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype, P):
    """every combination of guidance rescale on / off, multistep history on / off (and the DDIM update) and epsilon / v-prediction;
    all by-products, and x_next with RRG"""
    _, _, ops, schedule = _mods()
    c = _Case(Hl, Wl, h, w, d, patch, B, K, dtype, P)
    direction1, ldir1, unc1, local1 = c.directions()
    assert bool(torch.isfinite(direction1).all())
    # the std ratios: the fused reduction over the rows against the chain's over its tensors
    wsp = ops.guidance_moments_workspace(B, 4 * Hl * Wl, 4 * h * w, DEV)
    r1, rl1 = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    ops.guidance_moments(local1, direction1, c.guidance, r1, wsp)
    ops.guidance_moments(unc1, ldir1, c.guidance, rl1, wsp)
    r2, rl2 = torch.full((B,), -1.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    ops.phase_moments(c.g_out, c.v_out, c.x.shape, c.stamp, c.pick, c.cover, *c.geo, r2, wsp, ratio_low=rl2, region_w=c.region_w)
    assert _close(r2, r1) and _close(rl2, rl1), (r2, r1, rl2, rl1)
    r3 = torch.full((B,), -1.0, device=DEV)
    ops.phase_moments(c.g_out, c.v_out, c.x.shape, c.stamp, c.pick, c.cover, *c.geo, r3, wsp, region_w=c.region_w)
    assert torch.equal(r3, r2)
    for vp_kw in (dict(), dict(prediction_type="v_prediction")):
        pt = vp_kw.get("prediction_type", "epsilon")
        prod = schedule.DPMSolverSchedule(solver_order=2, **vp_kw)
        ts = prod.set_timesteps(20)
        coef = prod.multistep_coefficients(ts[7], ts[6], False)
        ddim = prod.step_coefficients(ts[7])
        assert coef[5] != 0.0
        for step in ("ddim", "ms1", "ms2"):
            ms = None if step == "ddim" else coef[2:] + (c.x0h if step == "ms2" else None,)
            ms_kw = {} if ms is None else dict(multistep=ms)
            for rescale in (False, True):
                flat_rs = dict(ratio=r2, guidance_rescale=GR) if rescale else {}
                rrg_rs = dict(ratio_low=rl2, guidance_rescale=GR) if rescale else {}
                prev1, x01, nxt1 = torch.empty_like(c.x), torch.empty_like(c.x), torch.empty_like(c.x)
                ops.cfg_ddim_step(local1, direction1, c.x, prev1, x01, c.guidance, *ddim, prediction_type=pt, **flat_rs, **ms_kw)
                ops.rrg_update(prev1, x01, c.low[K - 1], unc1, ldir1, c.T["up_row"], c.T["up_col"], nxt1, c.guidance, ddim[0],
                               ddim[1], c.norm, c.w_rrg, prediction_type=pt, **rrg_rs)
                out = _fused(c, ddim, pt, rs=(r2, rl2) if rescale else None, ms=ms)
                what = (pt, step, rescale)
                for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1),
                                   ("uncond_last", unc1), ("low_dir", ldir1)):
                    assert torch.equal(out[name].view(torch.int32), want.view(torch.int32)), (name, what)
                # without RRG and without the optional outputs: the same prev / x0, nothing else written
                bare = _fused(c, ddim, pt, rs=(r2, rl2) if rescale else None, ms=ms, rrg=False, by_products=False)
                assert torch.equal(bare["prev"], prev1) and torch.equal(bare["x0"], x01), what
                assert all(float(bare[k].min()) == 5.0 for k in ("x_next", "direction", "local", "uncond_last", "low_dir"))
                if P == 1:  # w == 1 everywhere: the plain entry points on the same rows, bit for bit
                    plain = {k: torch.full_like(c.x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
                    unc2, ldir2 = torch.empty_like(unc1), torch.empty_like(ldir1)
                    ops.phase_epilogue(c.g_out, c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, ddim, plain["prev"], plain["x0"],
                                       low_dir=ldir2, uncond_last=unc2, direction=plain["direction"], local=plain["local"],
                                       x_next=plain["x_next"], low_latent=c.low[K - 1], rrg_norm=c.norm, rrg_weight=c.w_rrg,
                                       prediction_type=pt, **ms_kw,
                                       **(dict(ratio=r2, ratio_low=rl2, guidance_rescale=GR) if rescale else {}))
                    for name in plain:
                        assert torch.equal(out[name].view(torch.int32), plain[name].view(torch.int32)), (name, what)
                    assert torch.equal(out["uncond_last"], unc2) and torch.equal(out["low_dir"], ldir2)


def test_null_region_w_launches_the_plain_kernels():
    """the library's own rule: region_w NULL with P = 1 is ed_phase_epilogue_ms / _gr and ed_phase_moments"""
    from elasticdiffusion_official_amd import _hip
    _, _, ops, schedule = _mods()
    c = _Case(*FUSED_ROWS[1], 1, 2, torch.float32, 1)
    prod = schedule.DPMSolverSchedule()
    ts = prod.set_timesteps(20)
    coef, ddim = prod.multistep_coefficients(ts[7], ts[6], False), prod.step_coefficients(ts[7])
    L, st = _hip.lib(), torch.cuda.current_stream(DEV).cuda_stream
    gpad, vpad = c.gpad, c.vpad
    for multistep in (0, 1):
        want_p, want_z = torch.empty_like(c.x), torch.empty_like(c.x)
        ops.phase_epilogue(c.g_out, c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, ddim, want_p, want_z,
                           **(dict(multistep=coef[2:] + (c.x0h,)) if multistep else {}))
        p, z = torch.empty_like(c.x), torch.empty_like(c.x)
        sc = tuple(float(v) for v in (coef[2:] if multistep else (ddim[2], ddim[3], 0.0, 0.0)))
        err = L.ed_phase_epilogue_rg(c.g_out.data_ptr(), c.v_out.data_ptr(), 0, c.x.data_ptr(), c.stamp.data_ptr(),
                                     *(t.data_ptr() for t in c.pick), *(t.data_ptr() for t in c.cover), None, p.data_ptr(),
                                     z.data_ptr(), None, None, None, None, None, c.K, c.B, 4, c.Hl, c.Wl, c.h, c.w, gpad.PH, gpad.PW,
                                     gpad.top, gpad.left, vpad.PH, vpad.PW, c.vp.n_col_blocks, float(c.guidance), float(ddim[0]), float(ddim[1]),
                                     *sc, 0.0, 0.0, 0, None, None, 0.0, 0.0, c.x0h.data_ptr() if multistep else None, multistep,
                                     None, 1, st)
        assert err == 0
        assert torch.equal(p, want_p) and torch.equal(z, want_z)


# ---------------------------------------------------------------------------------------------------
# one-hot halves, zero-weight rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", [FUSED_ROWS[1], FUSED_ROWS[3]])
def test_one_hot_halves_are_the_plain_epilogue_of_each_region(Hl, Wl, h, w, d, patch):
    """left half region 0 (the base prompt), right half region 1: on each half every output equals the plain epilogue run on the
    (uncond, cond_p) pair rows of that half's region; low_dir takes the half its (down_row, down_col) sample lies in"""
    _, _, ops, schedule = _mods()
    B, K = 2, 3
    ww = torch.zeros(2, Hl, Wl)
    ww[0, :, :Wl // 2], ww[1, :, Wl // 2:] = 1.0, 1.0
    c = _Case(Hl, Wl, h, w, d, patch, B, K, torch.float16, 2, weights=ww)
    sch = schedule.DDIMSchedule()
    ts = sch.set_timesteps(50)
    coef = sch.step_coefficients(ts[7])
    out = _fused(c, coef, "epsilon")
    plain = []
    for p in range(2):
        o = {k: torch.empty_like(c.x) for k in ("prev", "x0", "x_next", "direction", "local")}
        o["uncond_last"], o["low_dir"] = (torch.empty(B, 4, h, w, device=DEV) for _ in range(2))
        ops.phase_epilogue(c.pair_rows(p), c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, coef, o["prev"], o["x0"],
                           low_dir=o["low_dir"], uncond_last=o["uncond_last"], direction=o["direction"], local=o["local"],
                           x_next=o["x_next"], low_latent=c.low[K - 1], rrg_norm=c.norm, rrg_weight=c.w_rrg)
        plain.append(o)
    assert not torch.equal(plain[0]["direction"], plain[1]["direction"])
    half = Wl // 2
    for name in ("prev", "x0", "direction", "local"):
        assert torch.equal(out[name][..., :half], plain[0][name][..., :half]), name
        assert torch.equal(out[name][..., half:], plain[1][name][..., half:]), name
    assert torch.equal(out["uncond_last"], plain[0]["uncond_last"]) and torch.equal(out["uncond_last"], plain[1]["uncond_last"])
    right = (c.T["down_col"].long() >= half).view(1, 1, 1, w)          # the half a reduced pixel's sample point lies in
    assert bool(right.any()) and not bool(right.all())
    assert torch.equal(out["low_dir"], torch.where(right, plain[1]["low_dir"], plain[0]["low_dir"]))
    # x_next: the RRG term reads low_dir at up_col[X], whose sample point may lie in the other half -- rebuild it from the parts
    nxt = torch.empty_like(c.x)
    ops.rrg_update(out["prev"], out["x0"], c.low[K - 1], out["uncond_last"], out["low_dir"], c.T["up_row"], c.T["up_col"], nxt,
                   c.guidance, coef[0], coef[1], c.norm, c.w_rrg)
    assert torch.equal(out["x_next"], nxt)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_zero_weight_rows_are_not_read(dtype):
    """the rows of a region whose weight is 0 everywhere hold NaN: every output is what it is without them"""
    _, _, ops, schedule = _mods()
    Hl, Wl, h, w, d, patch = FUSED_ROWS[2]
    B, K, P = 2, 3, 3
    g = torch.Generator().manual_seed(5)
    ww = torch.zeros(P, Hl, Wl)
    a = torch.rand(Hl, Wl, generator=g)
    ww[0], ww[2] = a, 1.0 - a
    ww[0, :4], ww[2, :4] = 0.0, 0.0                                    # and a band where every weight is 0: d = 0
    c = _Case(Hl, Wl, h, w, d, patch, B, K, dtype, P, weights=ww)
    sch = schedule.DDIMSchedule()
    ts = sch.set_timesteps(50)
    coef = sch.step_coefficients(ts[7])
    wsp = ops.guidance_moments_workspace(B, 4 * Hl * Wl, 4 * h * w, DEV)

    def run(g_out):
        r, rl = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
        ops.phase_moments(g_out, c.v_out, c.x.shape, c.stamp, c.pick, c.cover, *c.geo, r, wsp, ratio_low=rl, region_w=c.region_w)
        out = _fused(c, coef, "epsilon", rs=(r, rl), g_out=g_out)
        out["ratio"], out["ratio_low"] = r, rl
        return out

    clean = run(c.g_out)
    poisoned = c.g_out.clone()
    poisoned.view(K, 1 + P, B, 4, c.gpad.PH, c.gpad.PW)[:, 2] = float("nan")
    got = run(poisoned)
    for name, want in clean.items():
        assert bool(torch.isfinite(got[name]).all()), name
        assert torch.equal(got[name], want), name
    assert float(clean["direction"][:, :, :4].abs().max()) == 0.0
    # the un-fused blend skips them too
    full = torch.randn(P, B, 4, Hl, Wl, generator=g).to(DEV)
    want = ops.region_blend(full, c.region_w)
    full[1] = float("nan")
    assert torch.equal(ops.region_blend(full, c.region_w), want)
    assert torch.equal(want.cpu(), RG.blend(full.cpu(), ww))


@pytest.mark.parametrize("shape", [(1, 4, 3, 5), (2, 4, 64, 128), (2, 3, 67, 97)])
def test_region_blend_bit_exact(shape):
    _, _, ops, _ = _mods()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H)
    for P in (1, 2, 5, 8):
        dirs = torch.randn(P, B, C, H, W, generator=g)
        ww = torch.rand(P, H, W, generator=g)
        ww[torch.rand(P, H, W, generator=g) < 0.4] = 0.0
        want = RG.blend(dirs, ww)
        got = ops.region_blend(dirs.to(DEV), ww.to(DEV))
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
        off = ops.region_blend(misaligned(dirs), misaligned(ww), out=misaligned(torch.empty(shape)))
        assert torch.equal(off.cpu().view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------------
# rejections: nothing is launched
# ---------------------------------------------------------------------------------------------------
def test_rejections_leave_nothing_launched():
    from elasticdiffusion_official_amd import _hip
    _, _, ops, schedule = _mods()
    c = _Case(*FUSED_ROWS[1], 1, 2, torch.float32, 2)
    Hl, Wl, h, w = c.Hl, c.Wl, c.h, c.w
    sch = schedule.DDIMSchedule()
    coef = sch.step_coefficients(sch.set_timesteps(50)[7])
    prev, x0 = torch.full_like(c.x, 3.0), torch.full_like(c.x, 3.0)

    def epi(region_w, g_out=None, **kw):
        ops.phase_epilogue(c.g_out if g_out is None else g_out, c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, coef, prev, x0,
                           region_w=region_w, **kw)

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        epi(c.region_w.cpu())
    with pytest.raises(RuntimeError, match="region_w must be"):
        epi(c.region_w[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="region_w must be"):
        epi(torch.ones(9, Hl, Wl, device=DEV), g_out=torch.zeros(c.K * 10, 4, c.gpad.PH, c.gpad.PW, device=DEV))
    buf = torch.full((2 * 4 * Hl * Wl,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps an output"):     # the weights alias x0
        ops.phase_epilogue(c.g_out, c.v_out, c.x, c.stamp, c.pick, c.cover, *c.geo, coef, prev, buf[:4 * Hl * Wl].view(1, 4, Hl, Wl),
                           region_w=buf[2 * Hl * Wl:4 * Hl * Wl].view(2, Hl, Wl))
    with pytest.raises(AssertionError):                                # rows of a pair batch with P = 2 weights
        epi(c.region_w, g_out=c.pair_rows(0))
    ws = ops.guidance_moments_workspace(1, 4 * Hl * Wl, 0, DEV)
    ratio = torch.full((1,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.phase_moments(c.g_out, c.v_out, c.x.shape, c.stamp, c.pick, c.cover, *c.geo, ratio, ws, region_w=c.region_w.cpu())
    masks = torch.zeros(2, Hl, Wl, dtype=torch.uint8, device=DEV)
    for bad_masks, bad_weights, match in ((masks.cpu(), [1, 1], "no CPU fallback"), (masks, [1.0], "weights"), (masks, [1.0, 0.0], "weights"),
                                          (masks, [1.0, float("nan")], "weights"), (masks[:0], [], "masks must be"),
                                          (torch.zeros(8, Hl, Wl, dtype=torch.uint8, device=DEV), [1.0] * 8, "masks must be")):
        with pytest.raises(RuntimeError, match=match):
            ops.region_weights(bad_masks, bad_weights)
    dirs = torch.zeros(2, 1, 4, Hl, Wl, device=DEV)
    out = torch.full((1, 4, Hl, Wl), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_blend(dirs.cpu(), c.region_w, out)
    with pytest.raises(RuntimeError, match="planes"):
        ops.region_blend(dirs, torch.ones(3, Hl, Wl, device=DEV), out)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.region_blend(dirs, c.region_w, dirs[0])
    g_rows = torch.full((c.K * 3, 4, c.gpad.PH, c.gpad.PW), 3.0, device=DEV)
    v_rows = torch.full((c.vp.V, 4, c.vpad.PH, c.vpad.PW), 3.0, device=DEV)
    asm = (c.x, c.idx, c.T["src_row"], c.T["src_col"], g_rows, h, w, c.gpad.top, c.gpad.left, None, None, v_rows, c.T["win_y0"],
           c.T["win_x0"], c.vp.Sh, c.vp.Sw, c.vpad.top, c.vpad.left, None)
    for copies in (1, 10, 2):                                          # 2: the rows hold 3 per step
        with pytest.raises(RuntimeError, match="assemble_rows_n"):
            ops.assemble_rows_n(*asm, copies)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.assemble_rows_n(c.x.cpu(), *asm[1:], 3)
    torch.cuda.synchronize()
    for t in (prev, x0, buf, ratio, out, g_rows, v_rows):
        assert float(t.min()) == 3.0 and float(t.max()) == 3.0         # nothing was launched
    assert ops._LAUNCH["device"] is None
    # the library refuses the same on its own (hipErrorInvalidValue = 1, before any launch)
    import ctypes
    L, st = _hip.lib(), torch.cuda.current_stream(DEV).cuda_stream
    wout = torch.full((3, Hl, Wl), 3.0, device=DEV)
    two = (ctypes.c_float * 2)(1.0, 1.0)
    assert L.ed_region_weights(masks.data_ptr(), (ctypes.c_float * 8)(*[1.0] * 8), 8, Hl * Wl, wout.data_ptr(), st) == 1
    assert L.ed_region_weights(masks.data_ptr(), two, 0, Hl * Wl, wout.data_ptr(), st) == 1
    assert L.ed_region_weights(masks.data_ptr(), (ctypes.c_float * 2)(1.0, -1.0), 2, Hl * Wl, wout.data_ptr(), st) == 1
    assert L.ed_region_weights(masks.data_ptr(), two, 2, Hl * Wl, None, st) == 1
    assert L.ed_region_weights(wout.data_ptr() + 8, two, 2, Hl * Wl, wout.data_ptr(), st) == 1           # masks inside the output
    n = 4 * Hl * Wl
    assert L.ed_region_blend(dirs.data_ptr(), c.region_w.data_ptr(), out.data_ptr(), 0, 4, Hl * Wl, st) == 1
    assert L.ed_region_blend(dirs.data_ptr(), c.region_w.data_ptr(), out.data_ptr(), 9, 4, Hl * Wl, st) == 1
    assert L.ed_region_blend(dirs.data_ptr(), None, out.data_ptr(), 2, 4, Hl * Wl, st) == 1
    assert L.ed_region_blend(dirs.data_ptr(), buf.data_ptr() + 4 * (n - 8), buf.data_ptr(), 2, 4, Hl * Wl, st) == 1  # w overlaps out
    gpad, vpad = c.gpad, c.vpad

    def lib_epi(region_w, P, x0_ptr=None):
        return L.ed_phase_epilogue_rg(c.g_out.data_ptr(), c.v_out.data_ptr(), 0, c.x.data_ptr(), c.stamp.data_ptr(),
                                      *(t.data_ptr() for t in c.pick), *(t.data_ptr() for t in c.cover), None, prev.data_ptr(),
                                      x0.data_ptr() if x0_ptr is None else x0_ptr, None, None, None, None, None, c.K, c.B, 4, Hl, Wl,
                                      h, w, gpad.PH, gpad.PW, gpad.top, gpad.left, vpad.PH, vpad.PW, c.vp.n_col_blocks, 1.0,
                                      *(float(v) for v in coef), 0.0, 0.0, 0.0, 0.0, 0, None, None, 0.0, 0.0, None, 0, region_w, P, st)

    assert lib_epi(c.region_w.data_ptr(), 0) == 1 and lib_epi(c.region_w.data_ptr(), 9) == 1
    assert lib_epi(None, 2) == 1
    assert lib_epi(buf.data_ptr() + 4 * (n - 8), 2, x0_ptr=buf.data_ptr()) == 1                          # region_w overlaps x0

    def lib_mom(region_w, P, ratio_ptr=None):
        return L.ed_phase_moments_rg(c.g_out.data_ptr(), c.v_out.data_ptr(), 0, c.stamp.data_ptr(), *(t.data_ptr() for t in c.pick),
                                     *(t.data_ptr() for t in c.cover), ratio.data_ptr() if ratio_ptr is None else ratio_ptr, None,
                                     ws.data_ptr(), c.K, c.B, 4, Hl, Wl, h, w, gpad.PH, gpad.PW, gpad.top, gpad.left, vpad.PH,
                                     vpad.PW, c.vp.n_col_blocks, 1.0, region_w, P, st)

    assert lib_mom(c.region_w.data_ptr(), 0) == 1 and lib_mom(c.region_w.data_ptr(), 9) == 1 and lib_mom(None, 2) == 1
    assert lib_mom(buf.data_ptr(), 2, ratio_ptr=buf.data_ptr() + 16) == 1                                 # region_w overlaps ratio

    def lib_asm(copies, E=0, extra=None):
        return L.ed_assemble_rows_n(c.x.data_ptr(), c.B, 4, Hl, Wl, c.idx.data_ptr(), c.T["src_row"].data_ptr(),
                                    c.T["src_col"].data_ptr(), None, g_rows.data_ptr(), None, c.K, h, w, gpad.PH, gpad.PW, gpad.top,
                                    gpad.left, c.T["win_y0"].data_ptr(), c.T["win_x0"].data_ptr(), None, v_rows.data_ptr(), c.vp.V,
                                    c.vp.Sh, c.vp.Sw, vpad.PH, vpad.PW, vpad.top, vpad.left, 0, extra, E, None, copies, st)

    assert lib_asm(1) == 1 and lib_asm(10) == 1 and lib_asm(3, E=2) == 1 and lib_asm(3, E=-1) == 1
    torch.cuda.synchronize()
    for t in (prev, x0, buf, ratio, out, g_rows, v_rows, wout):
        assert float(t.min()) == 3.0 and float(t.max()) == 3.0


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _regions(H, W):
    """two regions: the right half as a picture mask, and an overlapping box with weight 2"""
    half = np.zeros((H, W), np.uint8)
    half[:, W // 2:] = 255
    return [("a harbour at dusk", half), ("a lighthouse", (W // 4, H // 4, 3 * W // 4, 3 * H // 4), 2.0)]


def _loop_kw(name):
    c = cases.E2E_CASES[name]
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)
    kw.update(c.get("kw", {}))
    return kw


def _cond_kw(name):
    from oracle.elastic_oracle import get_downsample_size
    c = cases.E2E_CASES[name]
    if not c.get("controlnet"):
        return {}
    ds = get_downsample_size(c["H"], c["W"], c["sd"])
    return dict(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)


def _sched_pair(variant):
    """variant -> (the product's scheduler, the restatement's)"""
    _, _, _, schedule = _mods()
    if variant == "ddim":
        return schedule.DDIMSchedule(), DPMSolverCPU(sampler="ddim")
    if variant == "v_rescale":
        return schedule.DDIMSchedule(**V_TRAILING_ZSNR), DPMSolverCPU(sampler="ddim", **V_TRAILING_ZSNR)
    assert variant == "dpm"
    return schedule.DPMSolverSchedule(solver_order=2), DPMSolverCPU(solver_order=2)


def _pipe(name, variant="ddim", **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.E2E_CASES[name]
    xl = c["sd"].startswith("XL")
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            text_encoder=RG.prompt_embeds(xl), scheduler=_sched_pair(variant)[0],
                            controlnet=FakeControlNet() if c.get("controlnet") else None, **extra)


_ORACLE = {}


def _oracle(name, variant="ddim", regional=True):
    """RegionalOracle's (latent, RNG tail, weights) for one case, computed once and shared"""
    key = (name, variant, regional)
    if key not in _ORACLE:
        c = cases.E2E_CASES[name]
        xl = c["sd"].startswith("XL")
        orc = RG.RegionalOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), _sched_pair(variant)[1], RG.prompt_embeds(xl),
                                sd_version=c["sd"], view_batch_size=c["vbs"], pooled_dim=16 if xl else None,
                                controlnet=FakeControlNet() if c.get("controlnet") else None)
        orc.seed_everything(c["seed"])
        kw = dict(_loop_kw(name), **_cond_kw(name))
        if variant == "v_rescale":
            kw["guidance_rescale"] = GR
        if regional:
            kw["regions"] = _regions(c["H"], c["W"])
        z = orc.generate_latent(["p"], "", **kw)
        _ORACLE[key] = (z, torch.rand(4), orc.last_region_weights)
    return _ORACLE[key]


def _run(name, variant="ddim", fused=True, regional=True, count=False):
    from elasticdiffusion_official_amd import ops, pipeline
    c = cases.E2E_CASES[name]
    kw = dict(_loop_kw(name), **_cond_kw(name))
    if variant == "v_rescale":
        kw["guidance_rescale"] = GR
    if regional:
        kw["regions"] = _regions(c["H"], c["W"])
    pipeline.FUSED_GLUE = fused
    counts = None
    try:
        pipe = _pipe(name, variant)
        pipe.seed_everything(c["seed"])
        if count:
            ops.TIMER.start()
        try:
            z = pipe.generate_latents("p", "", **kw).cpu()
            tail = torch.rand(4)
        finally:
            if count:
                counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    finally:
        pipeline.FUSED_GLUE = True
    return z, tail, pipe, counts


E2E = [("cfg2_sd_512x1024", "ddim"), ("xl_single_view_512x1024", "ddim"), ("cn_sd_512x1024", "ddim"),
       ("cfg2_sd_512x1024", "v_rescale"), ("cfg2_sd_512x1024", "dpm")]


@pytest.mark.parametrize("name,variant", E2E)
def test_end_to_end_vs_regional_oracle(name, variant):
    """cfg2: padded global rows, RePaint and RRG active; xl_single_view: SDXL's pooled rows; cn: ControlNet condition rows; then
    guidance rescale on a v-prediction / zero-SNR schedule and DPM-Solver++(2M).  Fused and un-fused glue give the same bits."""
    want, otail, ow = _oracle(name, variant)
    z, tail, pipe, counts = _run(name, variant, fused=True, count=True)
    err = rel_l2(z, want)
    print(f"{name} {variant}: rel-L2 vs RegionalOracle {err:.3e}")
    assert bool(torch.isfinite(z).all())
    assert err < 1e-4, err
    assert torch.equal(tail, otail)
    # the weights: [P, Hl, Wl] on the device, the restatement's bits (Pillow's resize bytes, then the fp32 sequence)
    w = pipe.last_region_weights
    assert w.is_cuda and tuple(w.shape) == (3, cases.E2E_CASES[name]["H"] // 8, cases.E2E_CASES[name]["W"] // 8)
    assert torch.equal(w.cpu().view(torch.int32), ow.view(torch.int32))
    # launches: one weights launch per image, the regional assemble and epilogue once per phase in the places of the plain ones
    c = cases.E2E_CASES[name]
    phases = 2 * c["steps"] - 1 if _loop_kw(name).get("repaint_sampling", True) and c["R"] > 0 else c["steps"]
    glue = {k: v for k, v in counts.items() if k.startswith("ed_assemble") or "epilogue" in k or "moments" in k or "region" in k}
    expect = {"ed_region_weights": 1, "ed_assemble_rows_n": phases, "ed_phase_epilogue_rg": phases}
    if variant == "v_rescale":
        expect["ed_phase_moments_rg"] = phases
    assert glue == expect, counts
    # the un-fused path: the same bits
    z2, tail2, _, counts2 = _run(name, variant, fused=False, count=True)
    assert torch.equal(z2, z) and torch.equal(tail2, tail)
    assert counts2["ed_region_blend"] == 2 * phases and "ed_phase_epilogue_rg" not in counts2, counts2
    # and the regions matter
    assert rel_l2(z, _oracle(name, variant, regional=False)[0]) > 1e-3


def test_run_without_regions_is_the_loop_as_it_was(golden_dir):
    name = "cfg2_sd_512x1024"
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    z1, tail1, pipe, counts1 = _run(name, regional=False, count=True)
    z2, tail2, _, counts2 = _run(name, regional=False, count=True)
    assert torch.equal(z1, z2) and torch.equal(tail1, tail2) and counts1 == counts2
    assert pipe.last_region_weights is None
    assert not any(k in counts1 for k in REGIONAL_ENTRY_POINTS), counts1
    c = cases.E2E_CASES[name]
    phases = 2 * c["steps"] - 1
    glue = {k: v for k, v in counts1.items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k or "moments" in k}
    assert glue == {"ed_assemble_rows": phases, "ed_phase_epilogue": phases, "ed_undo_step": c["steps"] - 1}, counts1
    assert rel_l2(z1, torch.from_numpy(g[f"{name}/latent"])) < 1e-4          # the golden of the real reference
    np.testing.assert_array_equal(tail1.numpy(), g[f"{name}/rng_tail"])
    # the host RNG stream does not depend on the regions
    _, tail3, pipe3, _ = _run(name, regional=True)
    assert torch.equal(tail3, tail1) and pipe3.last_region_weights is not None


def test_one_full_region_is_the_plain_run_with_that_prompt():
    """weight 1 for the region everywhere, 0 for the base prompt: its rows are computed and never read"""
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    q = "a harbour at dusk"
    pipe = _pipe(name)
    pipe.seed_everything(c["seed"])
    want = pipe.generate_latents(q, "", **_loop_kw(name)).cpu()
    pipe.seed_everything(c["seed"])
    got = pipe.generate_latents("p", "", **_loop_kw(name), regions=[(q, np.full((c["H"], c["W"]), 255, np.uint8))]).cpu()
    assert rel_l2(got, want) < 1e-5, rel_l2(got, want)     # the model's own batch-shape dependent rounding, as between interleaved jobs
    pipe.seed_everything(c["seed"])
    assert rel_l2(pipe.generate_latents("p", "", **_loop_kw(name)).cpu(), want) > 1e-3


def test_mask_forms_blur_and_refusals():
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    H, W = c["H"], c["W"]
    kw = dict(_loop_kw(name), num_inference_steps=1, resampling_steps=1)
    pipe = _pipe(name)
    from PIL import Image
    half = np.zeros((H, W), np.uint8)
    half[:, W // 2:] = 255
    ws = []
    for mask in (half, torch.from_numpy(half), Image.fromarray(half), (W // 2, 0, W, H)):
        pipe.seed_everything(1)
        pipe.generate_latents("p", "", **kw, regions=[("q", mask)])
        ws.append(pipe.last_region_weights.cpu())
    assert all(torch.equal(w, ws[0]) for w in ws[1:])
    want = RG.region_weights(torch.from_numpy(RG.latent_mask(half, H, W))[None], [1.0])
    assert torch.equal(ws[0], want)
    low = torch.from_numpy(RG.latent_mask(half, H, W))
    pipe.generate_latents("p", "", **kw, regions=[("q", low)])
    assert torch.equal(pipe.last_region_weights.cpu(), want)          # a latent-size mask is used as is
    pipe.generate_latents("p", "", **kw, regions=[("q", half, 2.0)], region_blur=12.0)
    soft = RG.region_weights(torch.from_numpy(RG.latent_mask(half, H, W, region_blur=12.0))[None], [2.0])
    got = pipe.last_region_weights.cpu()
    assert float((got - soft).abs().max()) <= 2.0 * (1.0 / 255) + 1e-6  # the blur's bytes are Pillow's to within one level
    assert not torch.equal(got, ws[0])
    for bad in (dict(regions=[("q", half[:, :-8])]), dict(regions=[]), dict(regions=[("q", half, 0.0)]), dict(region_blur=2.0),
                dict(regions=[("q", half)], region_blur=-1.0)):
        with pytest.raises(ValueError):
            pipe.generate_latents("p", "", **kw, **bad)
        with pytest.raises(ValueError):
            pipe.generate_image("p", "", **kw, **bad)
    with pytest.raises(ValueError):
        pipe.generate_latents_interleaved([dict(prompts="p", seed=1, regions=[("q", half[:, :-8])])], **kw)
    with pytest.raises(ValueError, match="generate_image"):
        pipe.generate(torch.zeros(1, 4, 64, 64), None, None, regions=[("q", half)])


class _ChunkingEncoder:
    """a stand-in for a chunking text encoder: 77 tokens per started 20 characters of the longest prompt, the prompt's own
    embedding (``RG.prompt_embeds``) tiled over the chunks"""

    def __init__(self):
        self.fn = RG.prompt_embeds(False)
        self.calls = []

    def chunks(self, prompts):
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        return max(1 + len(p) // 20 for p in prompts)

    def __call__(self, prompts, min_chunks=None):
        n = max(self.chunks(prompts), int(min_chunks or 1))
        e, p = self.fn(prompts)
        self.calls.append((list(prompts) if not isinstance(prompts, str) else [prompts], n))
        return e.repeat(1, n, 1), p.repeat(1, n, 1)


def test_region_prompts_share_the_chunk_count_of_the_longest():
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    kw = dict(_loop_kw(name), num_inference_steps=1, resampling_steps=1)
    long_q = "a harbour at dusk with fishing boats and gulls over the quay"      # 60 characters: 4 chunks of this stand-in
    enc = _ChunkingEncoder()
    assert enc.chunks(long_q) == 4 and enc.chunks(["p", ""]) == 1
    pipe = _pipe(name)
    pipe.text_encoder = enc
    pipe.seed_everything(1)
    z = pipe.generate_latents("p", "", **kw, regions=[(long_q, (c["W"] // 2, 0, c["W"], c["H"]))]).cpu()
    assert bool(torch.isfinite(z).all())
    assert [n for _, n in enc.calls] == [4, 4, 4] and enc.calls[2][0] == [long_q]  # negative, base and region prompt alike
    # the tiled embedding has the mean of the single chunk: the latent of the run with the plain stand-in, to the mean's rounding
    pipe2 = _pipe(name)
    pipe2.seed_everything(1)
    z2 = pipe2.generate_latents("p", "", **kw, regions=[(long_q, (c["W"] // 2, 0, c["W"], c["H"]))]).cpu()
    assert rel_l2(z, z2) < 1e-5
    enc.calls.clear()
    pipe.generate_latents_interleaved([dict(prompts="p", seed=1), dict(prompts="p", seed=2, regions=[(long_q, (0, 0, 64, 64))])], **kw)
    assert enc.calls and all(n == 4 for _, n in enc.calls)                        # one chunk count for all jobs of the call


def test_image_prompt_tokens_ride_on_every_conditional_row():
    """an IP-Adapter's image tokens (stand-ins here: the loop only concatenates them) go behind the text tokens of the base AND the
    region rows, the zero-embedding tokens behind every unconditional row; the restatement with the same contexts agrees"""
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    g = torch.Generator().manual_seed(4)
    iun, ico = torch.randn(1, 4, 32, generator=g), torch.randn(1, 4, 32, generator=g)
    base = RG.prompt_embeds(False)

    def with_tokens(prompts):
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        e, _ = base(prompts)
        e = torch.cat([e, torch.cat([iun if p == "" else ico for p in prompts])], dim=1)
        return e, e

    kw = dict(_loop_kw(name), regions=_regions(c["H"], c["W"]))
    orc = RG.RegionalOracle(FakeUNet(c["sample"]), FakeVAE(), DPMSolverCPU(sampler="ddim"), with_tokens, sd_version=c["sd"],
                            view_batch_size=c["vbs"])
    orc.seed_everything(c["seed"])
    want = orc.generate_latent(["p"], "", **kw)
    pipe = _pipe(name)
    pipe._check_ip_adapter = lambda *a, **k: None
    pipe._ip_tokens = lambda B, image, embeds: (iun.to(DEV).expand(B, -1, -1), ico.to(DEV).expand(B, -1, -1))
    seen, embed_rows = [], pipe._embed_rows

    def spy(K, V, un, co, pun, pco):
        seen.append((K, V, un, co))
        return embed_rows(K, V, un, co, pun, pco)
    pipe._embed_rows = spy
    pipe.seed_everything(c["seed"])
    z = pipe.generate_latents("p", "", **kw, ip_adapter_image_embeds=torch.zeros(1, 8)).cpu()
    assert rel_l2(z, want) < 1e-4, rel_l2(z, want)
    assert seen and all(isinstance(co, list) and len(co) == 3 for _, _, _, co in seen)
    for _, _, un, cos in seen:
        assert un.shape[1] == 81 and torch.equal(un[:, 77:].cpu(), iun)
        assert all(co.shape[1] == 81 and torch.equal(co[:, 77:].cpu(), ico) for co in cos)
    assert len({tuple(co[0, 0, :4].tolist()) for co in seen[0][3]}) == 3           # three different prompts


def test_interleaved_two_jobs_with_different_regions_match_each_alone():
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    kw = _loop_kw(name)
    H, W = c["H"], c["W"]
    jobs = [dict(prompts="p", negative_prompts="", seed=c["seed"], regions=_regions(H, W)),
            dict(prompts="p", negative_prompts="", seed=11, regions=[("a meadow", (0, 0, W // 2, H))], region_blur=8.0)]
    pipe = _pipe(name)
    alone = []
    for job in jobs:
        pipe.seed_everything(job["seed"])
        alone.append(pipe.generate_latents(job["prompts"], "", **kw, regions=job["regions"],
                                           region_blur=job.get("region_blur", 0.0)).clone())
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], _oracle(name)[0]) < 1e-4
    assert rel_l2(got[0], got[1]) > 1e-2


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_region_flags(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    base = ["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "3", "--resampling_steps", "1", "--outdir",
            str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4"]
    mask = np.zeros((512, 512), np.uint8)
    mask[256:] = 255
    path = str(tmp_path / "mask.png")
    Image.fromarray(mask).save(path)
    d0 = main(base + ["--exp", "default"])
    d1 = main(base + ["--exp", "regions", "--region_prompt", "mountains", "--region_mask", "0,0,256,512", "--region_prompt",
                      "a harbour", "--region_mask", path + ":2", "--region_blur", "8"])
    a0, a1 = (np.asarray(Image.open(os.path.join(d, "0.png")), dtype=np.float32) for d in (d0, d1))
    assert a0.shape == a1.shape == (512, 512, 3) and np.isfinite(a1).all() and a1.std() > 0
    assert not np.array_equal(a0, a1)
    args = open(os.path.join(d1, "args.txt")).read()
    assert "region_prompt: ['mountains', 'a harbour']" in args and "region_blur: 8.0" in args
    with pytest.raises(SystemExit):
        main(base + ["--region_prompt", "mountains"])
    with pytest.raises(SystemExit):
        main(base + ["--region_prompt", "mountains", "--region_mask", "0,0,256,600"])
