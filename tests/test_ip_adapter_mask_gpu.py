"""-m gpu: IP-Adapter attention masks on the device -- ``ed_ip_mask_rows`` against ``ed_assemble_rows_n``'s
extra channels and the torch-CPU restatement, bit for bit; ``ed_flash_attention_ipm`` against its fp32 / fp64 statement, its limits
(m == 1, m == 0, one-hot masks), its addressing (m_sb = 0, a level offset, poison around every valid word), its rejections and the
adversarial families; the dispatch of models.Attention; the reduced-width XL forward; the pipeline (all-255 / all-0 / box masks,
graph replay across a change of masks, the rows a phase is handed, jobs in flight, the command line)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import attention_cases as A
from tests import ip_adapter_mask_spec as KS
from tests import ip_adapter_multi_spec as MS
from tests import ip_mask_cpu as C
from tests.glue_geometries import SCALAR_GEOMETRIES, launch_class, plans

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
SEGMENTATIONS = [(4,), (32,), (16, 16), (4, 16), (1, 1, 1, 1)]
WEIGHTS = (0.6, 1.0, -0.5, 0.3)
ABS = {torch.bfloat16: 3e-2, torch.float16: 6e-3}     # test_ip_adapter_multi_gpu's absolute bar for |v| ~ 1


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _w(values):
    return torch.tensor(list(values), dtype=torch.float32, device=DEV)


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# ed_ip_mask_rows
# ---------------------------------------------------------------------------------------------------------------------
# the smallest geometries of tests/glue_geometries.py, all with 64 x 64 rows: "ff_views" (three views, strips left and right of both
# parts), "ft" / "tf" (each leaves one of ed_assemble_rows_n's 4-wide paths) -- their rows are 64 high, so none has strips above and
# below; "both_axes" (a 384 x 320 px picture: 48 x 40 latent, 40 x 34 reduced) adds them: the picked frame sits at (12, 15), the
# one window at (8, 12)
GEOMETRIES = dict({k: SCALAR_GEOMETRIES[k] for k in ("ff_views", "ft", "tf")}, both_axes=(48, 40, 40, 34, 64))
MASK_GEOMETRIES = list(GEOMETRIES)


def _mask_case(name, B, A_, K, copies, nan_outside=False):
    """-> (device args of ops.ip_mask_rows / ops.assemble_rows_n, the CPU restatement's rows)"""
    Hl, Wl, h, w, d = GEOMETRIES[name]
    pp, vp, gpad, vpad = plans(Hl, Wl, h, w, d)
    assert (gpad.PH, gpad.PW, vpad.PH, vpad.PW) == (d, d, d, d)
    if name == "both_axes":
        assert min(gpad.top, gpad.left, vpad.top, vpad.left) > 0
    g = torch.Generator().manual_seed(Hl * 7 + Wl + A_)
    idx = torch.randint(0, 4, (K, h * w), generator=g, dtype=torch.uint8)
    masks = C.u8_masks(B, A_, Hl, Wl, seed=Hl + 3 * A_)
    cpu = (idx, _i32(pp.src_row), _i32(pp.src_col), h, w, gpad.top, gpad.left, _i32(vp.win_y0), _i32(vp.win_x0), vp.Sh, vp.Sw,
           vpad.top, vpad.left, d, d, copies)
    dev = tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in cpu)
    return masks, cpu, dev, (Hl, Wl, h, w, d, vp, gpad, vpad)


@pytest.mark.parametrize("name", MASK_GEOMETRIES)
@pytest.mark.parametrize("B,A_,copies", [(1, 1, 2), (2, 4, 3), (1, 4, 2), (2, 1, 3)])
def test_ip_mask_rows_bit_exact(name, B, A_, copies):
    """level 0 == channels C.. of ed_assemble_rows_n with extra = masks, pad_value = 0 and fp32 rows; levels 1..3 == the torch-CPU
    restatement; masks hold exact 0, exact 1 and k / 255; NaN planted outside every gathered pixel changes no bit"""
    ops = _ops()
    K = 2
    masks, cpu, dev, (Hl, Wl, h, w, d, vp, gpad, vpad) = _mask_case(name, B, A_, K, copies)
    assert bool((masks == 0).any()) and bool((masks == 1).any()) and bool(((masks > 0) & (masks < 1)).any())
    want = C.mask_rows(masks, *cpu)
    md = masks.to(DEV)
    got = ops.ip_mask_rows(md, *dev)
    rows = (K * copies + vp.V) * B
    lay, S_ = ops.ip_mask_layout(d, d)
    assert tuple(got.shape) == (rows, A_, S_) and got.dtype == torch.float32
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    # level 0 against the assemble launch
    x = torch.randn(B, 4, Hl, Wl, generator=torch.Generator().manual_seed(1)).to(DEV)
    g_rows = torch.full((K * copies * B, 4 + A_, d, d), 9.0, device=DEV)
    v_rows = torch.full((vp.V * B, 4 + A_, d, d), 9.0, device=DEV)
    idx, sr, sc = dev[0], dev[1], dev[2]
    ops.assemble_rows_n(x, idx, sr, sc, g_rows, h, w, gpad.top, gpad.left, None, None, v_rows, dev[7], dev[8], vp.Sh, vp.Sw, vpad.top,
                        vpad.left, None, copies, md, torch.zeros(A_, device=DEV))
    l0 = got[:, :, :d * d].view(rows, A_, d, d)
    assert torch.equal(l0[:K * copies * B], g_rows[:, 4:]) and torch.equal(l0[K * copies * B:], v_rows[:, 4:])
    # an explicit output buffer gives the same bits
    out = torch.full((rows, A_, S_), 7.0, device=DEV)
    assert ops.ip_mask_rows(md, *dev, out=out) is out and torch.equal(out, got)
    # poison: every mask pixel that no row gathers becomes NaN.  The views tile the whole latent, so the launch with both parts
    # reads every pixel; the global rows alone (the picks of K = 2 steps) leave pixels unread -- which ones, an index image tells
    pick_cpu = cpu[:7] + (None, None, 0, 0, 0, 0) + cpu[13:]
    pick_dev = dev[:7] + (None, None, 0, 0, 0, 0) + dev[13:]
    index_img = torch.arange(1, Hl * Wl + 1, dtype=torch.float32).view(1, 1, Hl, Wl)
    hit = C.level0(index_img, *pick_cpu).long().unique()
    used = torch.zeros(Hl * Wl, dtype=torch.bool)
    used[hit[hit > 0] - 1] = True
    used = used.view(Hl, Wl)
    assert bool((~used).any()) and bool(used.any())
    poisoned = masks.clone()
    poisoned[:, :, ~used] = float("nan")
    assert torch.equal(ops.ip_mask_rows(poisoned.to(DEV), *pick_dev).view(torch.int32), got[:K * copies * B].view(torch.int32))


def test_ip_mask_rows_reaches_both_launch_classes_and_one_part_alone():
    ops = _ops()
    assert launch_class(*SCALAR_GEOMETRIES["ft"]) == (False, True) and launch_class(*SCALAR_GEOMETRIES["tf"]) == (True, False)
    masks, cpu, dev, (Hl, Wl, h, w, d, vp, gpad, vpad) = _mask_case("ff_views", 2, 2, 2, 2)
    md = masks.to(DEV)
    both = ops.ip_mask_rows(md, *dev)
    picks = ops.ip_mask_rows(md, *dev[:7], None, None, 0, 0, 0, 0, d, d, 2)
    views = ops.ip_mask_rows(md, None, None, None, 0, 0, 0, 0, *dev[7:13], d, d, 2)
    n_g = 2 * 2 * 2
    assert torch.equal(picks, both[:n_g]) and torch.equal(views, both[n_g:])


def test_ip_mask_rows_rejections_and_a_clean_next_launch():
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    masks, cpu, dev, (Hl, Wl, h, w, d, vp, gpad, vpad) = _mask_case("ff_views", 1, 2, 1, 2)
    md = masks.to(DEV)
    out = torch.empty((1 * 2 + vp.V) * 1, 2, ops.ip_mask_layout(d, d)[1], device=DEV)
    idx, sr, sc, wy, wx = dev[0], dev[1], dev[2], dev[7], dev[8]
    st = torch.cuda.current_stream().cuda_stream

    def raw(masks_p=md.data_ptr(), A_=2, PH=d, PW=d, Sw=vp.Sw, w_=w, out_p=out.data_ptr(), copies=2, idx_p=idx.data_ptr()):
        return _hip.lib().ed_ip_mask_rows(masks_p, 1, A_, Hl, Wl, idx_p, sr.data_ptr(), sc.data_ptr(), 1, h, w_, gpad.top, gpad.left,
                                          wy.data_ptr(), wx.data_ptr(), vp.V, vp.Sh, Sw, vpad.top, vpad.left, PH, PW, copies, out_p, st)
    assert raw(masks_p=None) == 1 and raw(out_p=None) == 1 and raw(idx_p=None) == 1            # NULL pointers
    assert raw(A_=0) == 1 and raw(A_=5) == 1                                                    # A outside 1..4
    assert raw(PH=d + 4) == 1 and raw(PW=d - 4) == 1                                            # not multiples of 8
    assert raw(Sw=d + 1) == 1 and raw(w_=d + 1) == 1                                            # a window / frame that does not fit
    assert raw(copies=1) == 1 and raw(copies=10) == 1
    with pytest.raises(RuntimeError, match="ip_mask_rows"):
        ops.ip_mask_rows(md, *dev[:13], d + 4, d, 2)
    with pytest.raises(RuntimeError, match="ip_mask_rows"):
        ops.ip_mask_rows(masks.to(DEV)[:, :1].expand(-1, 5, -1, -1).contiguous(), *dev)
    with pytest.raises(RuntimeError, match="ip_mask_rows"):
        ops.ip_mask_rows(masks, *dev)                                                           # host masks
    torch.cuda.synchronize()
    assert raw() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), C.mask_rows(masks, *cpu).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# ed_flash_attention_ipm
# ---------------------------------------------------------------------------------------------------------------------
def _qkv(B, H, Nq, N, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, device=DEV, generator=g).mul(1.5).to(dtype)
    kv = torch.randn(B, N, 2 * H * 64, device=DEV, generator=g)
    kv[..., :H * 64] *= 1.5
    kv = kv.to(dtype)
    return q, kv[..., :H * 64], kv[..., H * 64:]


def _mask(B, A_, Nq, seed):
    """random masks in [0, 1] with planted rows of exact 0 and exact 1"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    m = torch.rand(B, A_, Nq, device=DEV, generator=g)
    m[:, :, 0] = 0.0
    m[:, :, Nq // 2] = 1.0
    if Nq > 2:
        m[:, 0, Nq - 1], m[:, A_ - 1, 1] = 1.0, 0.0
    return m


def _sdpa(q, k, v, H):
    import torch.nn.functional as F
    hd = lambda t: t.reshape(t.shape[0], -1, H, 64).transpose(1, 2)     # noqa: E731
    return F.scaled_dot_product_attention(hd(q), hd(k), hd(v), scale=0.125).transpose(1, 2).reshape(q.shape)


def _plain(q, k, v, H, nt, segs, w, m):
    """the plain route: A + 1 SDPA calls and the masked axpys in the same dtype"""
    out = _sdpa(q, k[:, :nt], v[:, :nt], H)
    for a, (lo, hi) in enumerate(MS.segments(nt, segs)[1:]):
        out = out + (w[a] * m[:, a]).to(q.dtype)[..., None] * _sdpa(q, k[:, lo:hi], v[:, lo:hi], H)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H", [(2, 3), (1, 10)])
@pytest.mark.parametrize("Nq", [1, 100, 513])
@pytest.mark.parametrize("Nt", [1, 77, 97, 160])
def test_masked_attention_grid(dtype, B, H, Nq, Nt):
    """per segmentation: against A + 1 fp32 softmaxes with the mask under section 32.5's bar relative to the plain route measured
    here; m == 1 is ops.flash_attention_ipn bit for bit; m == 0 the text-only launch; one-hot masks pick ipn's rows with one weight;
    m_sb = 0 and a level inside a larger buffer give the bits of the expanded / compact mask"""
    ops = _ops()
    for segs in SEGMENTATIONS:
        A_ = len(segs)
        w = WEIGHTS[:A_]
        wd = _w(w)
        q, k, v = _qkv(B, H, Nq, Nt + sum(segs), dtype, Nq * 7 + Nt * 3 + sum(segs) + 100 * A_)
        m = _mask(B, A_, Nq, Nq + Nt + A_)
        got = ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m)
        ref = KS.masked_ref(q, k, v, H, Nt, segs, w, m, torch.float32)
        plain = _plain(q, k, v, H, Nt, segs, w, m)
        assert got.shape == (B, Nq, H * 64) and got.dtype == dtype and got.is_contiguous() and bool(torch.isfinite(got).all())
        err, err_p = float((got.float() - ref).abs().max()), float((plain.float() - ref).abs().max())
        rel, rel_p = float((got.float() - ref).norm() / ref.norm()), float((plain.float() - ref).norm() / ref.norm())
        print(f"ipm {dtype} B{B} H{H} Nq{Nq} Nt{Nt} segs{segs}: max|err| {err:.2e} (plain {err_p:.2e})  rel {rel:.2e} (plain {rel_p:.2e})")
        assert rel < 1.5 * rel_p + 1e-4, (segs, rel, rel_p)
        assert err < 3.0 * err_p + 4e-3, (segs, err, err_p)
        # m == 1 and m == 0
        ipn = ops.flash_attention_ipn(q, k, v, H, Nt, segs, wd)
        assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, torch.ones_like(m)), ipn)
        text = ops.flash_attention(q, k[:, :Nt], v[:, :Nt], H, v_path=8)
        assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, torch.zeros_like(m)), text)
        assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, torch.zeros_like(wd), m), text)
        # one-hot masks: row i is ipn's row i with every weight but w[i mod A] zeroed
        i = torch.arange(Nq, device=DEV)
        hot = (i[None, :] % A_ == torch.arange(A_, device=DEV)[:, None]).float()[None].expand(B, -1, -1).contiguous()
        got_hot = ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, hot)
        for a in range(A_):
            only = torch.zeros_like(wd)
            only[a] = wd[a]
            assert torch.equal(got_hot[:, a::A_], ops.flash_attention_ipn(q, k, v, H, Nt, segs, only)[:, a::A_]), (segs, a)
        # m_sb = 0: one mask for the batch
        shared = ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m[:1])
        assert torch.equal(shared, ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m[:1].expand(B, -1, -1).contiguous()))
        assert torch.equal(shared, ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m[0]))
        # a level at a non-zero offset inside a larger per-row buffer (as ops.ip_mask_rows lays it out)
        big = torch.full((B, A_, 37 + Nq + 11), float("nan"), device=DEV)
        big[:, :, 37:37 + Nq] = m
        assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, big[:, :, 37:37 + Nq]), got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_around_the_mask_changes_no_bit(dtype):
    """NaN / Inf behind row Nq - 1 of every adapter, behind the buffer's last element (the buffer ends where the last valid word
    ends: the allocator's slack is all there is behind it, so a read past it cannot be made visible, only a read inside the pad)
    and in another batch entry's rows"""
    ops = _ops()
    B, H, Nt = 3, 3, 77
    for Nq, segs in ((100, (4, 16)), (513, (1, 1, 1, 1)), (1, (32,)), (257, (16, 16))):
        A_ = len(segs)
        q, k, v = _qkv(B, H, Nq, Nt + sum(segs), dtype, Nq + A_)
        m = _mask(B, A_, Nq, Nq)
        wd = _w(WEIGHTS[:A_])
        clean = ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m)
        pad = 5
        flat = torch.full((B * A_ * (Nq + pad) - pad,), float("nan"), device=DEV)       # ends right behind the last valid word
        flat[1::2] = float("inf")
        view = torch.as_strided(flat, (B, A_, Nq), (A_ * (Nq + pad), Nq + pad, 1))
        view.copy_(m)
        assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, view), clean)
        m2 = m.clone()
        m2[1] = float("nan")                                                           # another batch entry's rows
        got = ops.flash_attention_ipm(q, k, v, H, Nt, segs, wd, m2)
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]) and not bool(torch.isfinite(got[1]).all())


def test_masked_kernel_rejections_and_a_clean_next_launch():
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    q = torch.randn(1, 64, 128, device=DEV).half()
    kv = torch.randn(1, 200, 128, device=DEV).half()
    w4 = _w(WEIGHTS)
    m = torch.rand(1, 4, 64, device=DEV)
    cases = [(77, ()), (77, (4, 4, 4, 4, 4)), (77, (4, 0)), (77, (16, 17)), (161, (4, 4))]
    for nt, segs in cases:                    # A = 0; A = 5; a zero-length segment; 33 image keys; Nt = 161
        n = nt + sum(segs)
        with pytest.raises(RuntimeError):
            ops.flash_attention_ipm(q, kv[:, :n], kv[:, :n], 2, nt, segs, torch.zeros(len(segs), device=DEV),
                                    torch.ones(1, max(1, len(segs)), 64, device=DEV))
    k = kv[:, :85].contiguous()
    q40, kv40 = torch.randn(1, 64, 80, device=DEV).half(), torch.randn(1, 85, 80, device=DEV).half()
    with pytest.raises(RuntimeError):
        ops.flash_attention_ipm(q40, kv40, kv40, 2, 77, (4, 4), w4[:2], m[:, :2])          # head dimension 40
    with pytest.raises(RuntimeError):
        ops.flash_attention_ipm(q.float(), k.float(), k.float(), 2, 77, (4, 4), w4[:2], m[:, :2])   # a 32-bit dtype
    for bad in (m[:, :2].cpu(), m[:, :2].double(), m[:, :3], m[:, :2, :63], None, m[:, :2, ::2][..., :32]):
        with pytest.raises(RuntimeError):     # host masks; fp64; a wrong adapter count; too few rows; None; a non-unit last stride
            ops.flash_attention_ipm(q, k, k, 2, 77, (4, 4), w4[:2], bad)
    # the C entry point refuses by itself, before any launch
    out = torch.empty_like(q)
    st = torch.cuda.current_stream().cuda_stream

    def raw(nt=77, segs=(4, 4), hd=64, code=1, m_p=m.data_ptr(), m_sb=0, m_sa=64):
        ni = (ctypes.c_int32 * max(1, len(segs)))(*segs)
        return _hip.lib().ed_flash_attention_ipm(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), out.data_ptr(), code, 1, 2, 64, nt, len(segs),
                                                 ctypes.addressof(ni), hd, q.stride(0), q.stride(1), kv.stride(0), kv.stride(1),
                                                 kv.stride(0), kv.stride(1), out.stride(0), out.stride(1), 0.125, w4.data_ptr(),
                                                 m_p, m_sb, m_sa, st)
    for nt, segs in cases:
        assert raw(nt, segs) == 1, (nt, segs)
    assert raw(hd=40) == 1 and raw(code=0) == 1                                            # head dim 40; fp32
    assert raw(m_p=None) == 1 and raw(m_p=m.data_ptr() + 2) == 1                            # NULL; misaligned
    assert raw(m_sa=63) == 1 and raw(m_sb=-1) == 1                                          # m_sa < Nq
    torch.cuda.synchronize()
    got = ops.flash_attention_ipm(q, k, k, 2, 77, (4, 4), w4[:2], m[:, :2])
    torch.cuda.synchronize()
    assert float((got.double() - KS.masked_ref(q, k, k, 2, 77, (4, 4), WEIGHTS, m[:, :2])).abs().max()) < 2.6 * ABS[torch.float16]


def _with_segments(dtype, q, kt, vt, H, segs, seed, builder=A.gaussian, outlier_in=None):
    """test_ip_adapter_multi_gpu._with_segments: image rows of ``builder`` behind the text rows; ``outlier_in`` = a: late_outlier's
    query row scores 180 against the LAST key of segment a"""
    _, ki, vi = builder(dtype, 64, kt.shape[0], H, A.MIN_NQ, sum(segs), seed, DEV)
    ki, vi = ki.clone(), vi.clone()
    if outlier_in is not None:
        b, h, row = A._at("late_outlier", q.shape[0], H)
        qr = q[b, row, h * 64:(h + 1) * 64].float()
        key = sum(segs[:outlier_in + 1]) - 1
        ki[b, key, h * 64:(h + 1) * 64] = (qr * (180.0 * 8.0 / float(qr.pow(2).sum()))).to(dtype)
    return torch.cat([kt, ki], 1), torch.cat([vt, vi], 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nt", [1, 77, 97, 160])
def test_masked_kernel_on_planted_rows(Nt, dtype):
    """the one-pass families of tests/attention_cases.py (uniform row, all-negative row, outlier key in the text part and inside one
    image segment) with a non-trivial mask, against float64; four launches give the same bits"""
    ops = _ops()
    B, H, Nq = 1, 3, 100
    q, kt, vt = A.combined(dtype, 64, B, H, Nq, Nt, 11 + Nt, DEV, creeping=False)
    for segs, hot in (((4, 16), 1), ((1, 1, 1, 1), 3), ((32,), 0)):
        A_ = len(segs)
        w = WEIGHTS[:A_]
        m = _mask(B, A_, Nq, 77 + A_).mul(0.75).add(0.125)      # in [0.125, 0.875]: no planted row loses its image term
        k, v = _with_segments(dtype, q, kt, vt, H, segs, 500 + sum(segs), outlier_in=hot)
        got = ops.flash_attention_ipm(q, k, v, H, Nt, segs, _w(w), m)
        for _ in range(3):
            assert torch.equal(ops.flash_attention_ipm(q, k, v, H, Nt, segs, _w(w), m), got)
        ref = KS.masked_ref(q, k, v, H, Nt, segs, w, m)
        bar = ABS[dtype] * (1.0 + sum(abs(x) for x in w))
        err = float((got.double() - ref).abs().max())
        print(f"planted {dtype} Nt{Nt} segs{segs}: max|err| {err:.2e} (bar {bar:.2e})")
        assert bool(torch.isfinite(got).all()) and err < bar
        # q = 0: the mean of V per segment, the image means weighted by w m
        b2, _, row2 = A._at("uniform_row", B, H)
        mean = v[b2, :Nt].double().mean(0)
        for a, (lo, hi) in enumerate(MS.segments(Nt, segs)[1:]):
            mean = mean + float(_w(w)[a] * m[b2, a, row2]) * v[b2, lo:hi].double().mean(0)
        assert float((got[b2, row2].double() - mean).abs().max()) < min(2e-2, ABS[dtype]) * (1.0 + sum(abs(x) for x in w))
        # the outlier row: one text V row plus w m times one V row of the hot segment, plus the other segments' softmaxes
        b, h, row = A._at("late_outlier", B, H)
        hs = slice(h * 64, (h + 1) * 64)
        want = vt[b, A.outlier_key(Nt), hs].double()
        for a, (lo, hi) in enumerate(MS.segments(Nt, segs)[1:]):
            c = float(_w(w)[a] * m[b, a, row])
            if a == hot:
                want = want + c * v[b, hi - 1, hs].double()
            else:
                want = want + c * MS.softmax_v(q[b:b + 1, row:row + 1, hs], k[b:b + 1, lo:hi, hs], v[b:b + 1, lo:hi, hs], 1)[0, 0]
        assert float((got[b, row, hs].double() - want).abs().max()) < bar


def test_masked_kernel_large_values_stay_finite():
    """fp16, |v| up to 3e4 in the text rows and in every segment; 1 + sum |w m| <= 1.9, so every exact output stays below 65504"""
    ops = _ops()
    dtype, B, H, Nq, Nt = torch.float16, 1, 3, 100, 77
    q, kt, vt = A.large_v(dtype, 64, B, H, Nq, Nt, 5, DEV)
    for segs, w in (((16, 16), (0.6, -0.3)), ((4, 16), (0.3, -0.6))):
        m = _mask(B, len(segs), Nq, 3)
        k, v = _with_segments(dtype, q, kt, vt, H, segs, 900 + len(segs), builder=A.large_v)
        got = ops.flash_attention_ipm(q, k, v, H, Nt, segs, _w(w), m)
        assert bool(torch.isfinite(got).all())
        err = float((got.double() - KS.masked_ref(q, k, v, H, Nt, segs, w, m)).abs().max())
        print(f"large v segs{segs}: max|err| {err:.3e}")
        assert err < ABS[dtype] * A.V_LARGE * 1.9
        assert float(got.float().abs().max()) <= A.V_LARGE * 1.9


# ---------------------------------------------------------------------------------------------------------------------
# models.Attention: launch counts from ops.TIMER
# ---------------------------------------------------------------------------------------------------------------------
def _attention(dim, heads, head_dim, cross, segs, seed):
    from elasticdiffusion_official_amd import models as M
    torch.manual_seed(seed)
    a = M.Attention(dim, heads, head_dim, cross_dim=cross)
    lin = lambda: torch.nn.Linear(cross, heads * head_dim, bias=False)   # noqa: E731
    a.set_ip_adapter(lin(), lin(), segs[0])
    for n in segs[1:]:
        a.add_ip_adapter(lin(), lin(), n, torch.zeros(len(segs)))
    return a.eval().requires_grad_(False)


@pytest.mark.parametrize("segs", [(4, 16), (4,)])
@pytest.mark.parametrize("head_dim,fused", [(64, True), (40, False)])
def test_attention_module_with_masks_takes_one_launch_where_the_kernel_applies(head_dim, fused, segs):
    ops = _ops()
    heads, PH, PW = (10 if head_dim == 64 else 8), 64, 32
    w = (0.75, 0.5)[:len(segs)]
    a32 = _attention(heads * head_dim, heads, head_dim, 64, segs, 3)
    a16 = copy.deepcopy(a32).to(DEV, torch.float16)
    g = torch.Generator(device=DEV).manual_seed(9)
    lay, S_ = ops.ip_mask_layout(PH, PW)
    N = lay[1][1]                                                       # the layer reads level 1: 32 x 16 = 512 query rows
    x = torch.randn(2, N, heads * head_dim, device=DEV, generator=g).half()
    ctx = torch.randn(2, 77 + sum(segs), 64, device=DEV, generator=g).half()
    m = torch.rand(2, len(segs), S_, device=DEV, generator=g)
    m[:, :, lay[1][0]:lay[1][0] + 7] = 0.0
    wd = _w(w)
    a16.ip_mask = (m, PH, PW, wd)
    ops.TIMER.start()
    try:
        with torch.no_grad():
            got = a16(x, ctx)
    finally:
        timed = ops.TIMER.stop()
    seen = {k: v[0] for k, v in timed.items() if k.startswith("ed_flash_attention")}
    assert seen == ({"ed_flash_attention_ipm": 1} if fused else {"ed_flash_attention": 1 + len(segs)}), seen
    with torch.no_grad():
        assert torch.equal(got, a16(x, ctx, kv=a16.project_kv(ctx)))
        a32.ip_mask = (m.cpu(), PH, PW, wd.cpu())
        ref = a32(x.float().cpu(), ctx.float().cpu())                   # the fp32 CPU module with the same masks
        a32.ip_mask = None
        a16.ip_mask = (torch.zeros_like(m), PH, PW, wd)
        zero = a16(x, ctx)
        a16.ip_mask = None
        a16.set_ip_adapter()
        text_only = a16(x, ctx[:, :77].contiguous())
    scale = float(ref.abs().max())
    assert float((got.float().cpu() - ref).abs().max()) <= 1e-2 * scale
    assert float((zero.float() - text_only.float()).abs().max()) <= 1e-3 * scale
    assert float((got.float() - text_only.float()).abs().max()) > 1e-2 * scale          # the adapters show
    with pytest.raises(ValueError, match="matches no level"):
        a16b = copy.deepcopy(a32).to(DEV, torch.float16)
        a16b.ip_mask = (m, PH, PW, wd)
        a16b(x[:, :100].contiguous(), ctx)


# ---------------------------------------------------------------------------------------------------------------------
# the reduced-width XL forward
# ---------------------------------------------------------------------------------------------------------------------
NI_BASE, NI_PLUS, CLIP_DIM, EMBED_DIM, SEQ = 4, 16, 48, 80, 10


def _adapters_for(sd, dtype=torch.float32, gain=4.0):
    from elasticdiffusion_official_amd import models as M
    from tests import ip_adapter_spec as IS
    cfg = M.SMALL_UNET_CONFIGS["sdxl" if sd.startswith("XL") else "sd15"]
    return [IS.random_adapter(cfg, NI_BASE, CLIP_DIM, seed=5, dtype=dtype, gain=gain),
            MS.random_plus_adapter(cfg, NI_PLUS, EMBED_DIM, seed=6, dtype=dtype, gain=gain)]


def _embeds(B=1, seed=8):
    g = torch.Generator().manual_seed(seed)
    e = [torch.randn(B, CLIP_DIM, generator=g), 2.0 * torch.randn(B, SEQ, EMBED_DIM, generator=g)]
    return e, [None, 2.0 * torch.randn(1, SEQ, EMBED_DIM, generator=g)]


def test_real_architecture_forward_with_masks(monkeypatch):
    """the fp16 6-row forward of the reduced-width XL UNet (64 x 64 latent, a base and a Plus adapter) with masks against its own
    fp32 CPU forward with the same masks: rel-L2 at most twice the text-only figure measured here"""
    from elasticdiffusion_official_amd import ElasticDiffusion
    from tests import realarch as R
    ops = _ops()
    sd = "XL1.0"
    unet, vae, _ = R.build_small(sd)
    adapters = _adapters_for(sd)
    S = unet.config.sample_size // 2
    g = torch.Generator().manual_seed(21)
    x = torch.randn(6, 4, S, S, generator=g)
    text = torch.randn(6, 77, 64, generator=g)
    pooled = torch.randn(6, 32, generator=g)
    (eb, ep), _ = _embeds(6)
    t = torch.tensor(500)
    kw = {"added_cond_kwargs": {"text_embeds": pooled, "time_ids": torch.zeros(6, 6)}}
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    pipe = ElasticDiffusion(DEV, sd, view_batch_size=4, unet=copy.deepcopy(unet).to(torch.float16), vae=copy.deepcopy(vae),
                            text_encoder=lambda s: None, use_graphs=False)

    def forward(txt, ipm=None):
        txt16 = txt.to(DEV, torch.float16)
        return pipe._forward_rows(x.to(DEV, torch.float16), t.to(DEV), txt16, pooled.to(DEV, torch.float16), None, pipe._text_kv(txt16),
                                  None, ipm).float().cpu()
    with torch.no_grad():
        rel0 = R.rel_l2(forward(text), unet(x, t, encoder_hidden_states=text, **kw)["sample"])
        pipe.load_ip_adapter(adapters[0], scale=0.75)
        pipe.load_ip_adapter(adapters[1], scale=0.5, add=True)
        unet.install_ip_adapter(adapters[0])
        unet.install_ip_adapter(adapters[1], add=True)
        unet.ip_scales = [0.75, 0.5]
        tokens = torch.cat([unet.ip_image_tokens(eb, 0), unet.ip_image_tokens(ep, 1)], dim=1)
        txt = torch.cat([text, tokens], dim=1).contiguous()
        # masks through the product's own launch: 6 view rows of a 96 x 80 latent
        masks = C.u8_masks(1, 2, 96, 80, seed=4)
        wy, wx = _i32([0, 0, 16, 16, 32, 32]), _i32([0, 16, 0, 16, 0, 16])
        m = ops.ip_mask_rows(masks.to(DEV), None, None, None, 0, 0, 0, 0, wy.to(DEV), wx.to(DEV), S, S, 0, 0, S, S, 2)
        assert tuple(m.shape) == (6, 2, ops.ip_mask_layout(S, S)[1])
        ops.TIMER.start()
        try:
            got = forward(txt, (m, S, S))
        finally:
            timed = ops.TIMER.stop()
        n_cross = len(unet.ip_attentions())
        assert timed["ed_flash_attention_ipm"][0] == n_cross and "ed_flash_attention_ipn" not in timed
        want = unet(x, t, encoder_hidden_states=txt, ip_masks=(m.cpu(), S, S), **kw)["sample"]
        rel = R.rel_l2(got, want)
        unmasked = unet(x, t, encoder_hidden_states=txt, **kw)["sample"]
        print(f"real-arch {sd} fp16 masked forward vs fp32 CPU: rel-L2 {rel:.3e} (text-only {rel0:.3e}); masks move the fp32 forward "
              f"by {R.rel_l2(want, unmasked):.3e}")
        assert bool(torch.isfinite(got).all()) and rel <= 2.0 * rel0, (rel, rel0)
        assert R.rel_l2(want, unmasked) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# pipeline: graphs and library convolutions in their deterministic algorithms (section 23.6's fixture)
# ---------------------------------------------------------------------------------------------------------------------
SMALL_RUN = dict(height=512, width=512, num_inference_steps=2, guidance_scale=10.0, resampling_steps=1, new_p=0.3, rrg_stop_t=0.4,
                 rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
H_PX, W_PX = 512, 512


def _small_pipe(dtype=torch.float16, adapters=True, scales=(0.7, 0.4)):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from tests import realarch as R
    unet, vae, _ = R.build_small("1.5")
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=copy.deepcopy(unet).to(dtype), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(False))
    if adapters:
        ads = _adapters_for("1.5")
        pipe.load_ip_adapter(ads[0], scale=scales[0])
        pipe.load_ip_adapter(ads[1], scale=scales[1], add=True)
    return pipe


def _run(pipe, seed=3, **kw):
    from tests import realarch as R
    pipe.text_encoder = R.embed_fn(False)
    pipe.seed_everything(seed)
    return pipe.generate_latents("p", "", **SMALL_RUN, **kw).clone()


def _ip_kw():
    (eb, ep), neg = _embeds(1)
    return dict(ip_adapter_image_embeds=[eb, ep], ip_adapter_negative_image_embeds=neg)


def _left_right():
    left = np.zeros((H_PX, W_PX), np.uint8)
    left[:, :W_PX // 2] = 255
    left[:, W_PX // 2 - 16:W_PX // 2 + 16] = 128                       # a graded band
    return left, (W_PX // 2, 0, W_PX, H_PX)


def test_pipeline_limits_of_the_masks(monkeypatch):
    """all-255 masks == the run without the keyword; all-0 masks == the run at weights [0, 0]; a box over the whole picture == the
    all-255 mask -- bit for bit; real masks move the result"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    ip = _ip_kw()
    pipe = _small_pipe()
    plain = _run(pipe, **ip)
    full = np.full((H_PX, W_PX), 255, np.uint8)
    assert torch.equal(_run(pipe, ip_adapter_masks=[full, torch.full((H_PX // 8, W_PX // 8), 255, dtype=torch.uint8)], **ip), plain)
    assert torch.equal(_run(pipe, ip_adapter_masks=[(0, 0, W_PX, H_PX), None], **ip), plain)
    zeros = _run(pipe, ip_adapter_masks=[np.zeros((H_PX, W_PX), np.uint8)] * 2, **ip)
    masked = _run(pipe, ip_adapter_masks=list(_left_right()), **ip)
    assert pipe._runner.stats()["eager"] == 0
    pipe.set_ip_adapter_scale([0.0, 0.0])
    assert torch.equal(zeros, _run(pipe, **ip))
    from tests import realarch as R
    assert R.rel_l2(masked, plain) > 1e-3 and R.rel_l2(masked, zeros) > 1e-3


def test_new_masks_replay_the_captured_graphs(monkeypatch):
    """three images with masks, then new masks, one more image: no entry added or dropped, nothing captured again, nothing eager,
    and the image is a fresh pipeline's with those masks, bit for bit"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    ip = _ip_kw()
    left, right_box = _left_right()
    pipe = _small_pipe()
    imgs = [_run(pipe, seed, ip_adapter_masks=[left, right_box], **ip) for seed in (3, 4, 5)]
    entries, stats = len(pipe._runner.entries), pipe._runner.stats()
    assert entries >= 1 and stats["eager"] == 0 and stats["captured"] >= 1
    new = [(0, 0, W_PX, H_PX // 2), np.ascontiguousarray(left.T)]
    after = _run(pipe, 3, ip_adapter_masks=new, **ip)
    assert len(pipe._runner.entries) == entries and pipe._runner.stats()["eager"] == 0
    assert pipe._runner.stats()["captured"] == stats["captured"]
    assert not torch.equal(after, imgs[0])
    assert torch.equal(after, _run(_small_pipe(), 3, ip_adapter_masks=new, **ip))
    # a run without masks uses graphs of its own: the masked entries stay
    _run(pipe, 3, **ip)
    assert len(pipe._runner.entries) > entries and pipe._runner.stats()["eager"] == 0


def test_single_adapter_with_a_mask_follows_a_change_of_scale(monkeypatch):
    """one adapter with a mask runs the device-weights path: the UNet allocates its fp32 weight tensor, and a new scale gives the
    image of a fresh pipeline loaded at that scale, bit for bit"""
    from tests import realarch as R
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    (eb, _), _ = _embeds(1)
    ip = dict(ip_adapter_image_embeds=eb)
    pipe = _small_pipe(adapters=False)
    pipe.load_ip_adapter(_adapters_for("1.5")[0], scale=0.7)
    left, _ = _left_right()
    a = _run(pipe, ip_adapter_masks=[left], **ip)
    assert pipe.unet.ip_weights is not None and float(pipe.unet.ip_weights[0]) == pytest.approx(0.7)
    pipe.set_ip_adapter_scale(0.2)
    b = _run(pipe, ip_adapter_masks=[left], **ip)
    fresh = _small_pipe(adapters=False)
    fresh.load_ip_adapter(_adapters_for("1.5")[0], scale=0.2)
    assert torch.equal(b, _run(fresh, ip_adapter_masks=[left], **ip)) and not torch.equal(a, b)
    assert R.rel_l2(a, b) > 1e-3 and pipe._runner.stats()["eager"] == 0


def test_the_rows_a_phase_is_handed_are_the_restatement_of_its_picks(monkeypatch):
    """every ops.ip_mask_rows launch of a run, recorded with its gather arguments (the phase's own picks): the buffer equals the
    torch-CPU restatement fed with them, and the masks are fp32(u8) / 255 of the latent-size masks"""
    from elasticdiffusion_official_amd import ops
    ip = _ip_kw()
    pipe = _small_pipe()
    calls = []
    real = ops.ip_mask_rows

    def recording(masks, *args, **kw):
        out = real(masks, *args, **kw)
        calls.append((masks.cpu(), tuple(a.cpu() if isinstance(a, torch.Tensor) else a for a in args), out.cpu()))
        return out
    monkeypatch.setattr(ops, "ip_mask_rows", recording)
    lat = torch.randint(0, 256, (H_PX // 8, W_PX // 8), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    _run(pipe, ip_adapter_masks=[lat, None], **ip)
    steps = SMALL_RUN["num_inference_steps"]
    assert len(calls) >= steps                                            # one launch per model call
    picks, with_picks = set(), 0
    for masks, args, out in calls:
        assert tuple(masks.shape) == (1, 2, H_PX // 8, W_PX // 8)
        assert torch.equal(masks[0, 0], lat.float() / 255.0) and torch.equal(masks[0, 1], torch.ones(H_PX // 8, W_PX // 8))
        assert torch.equal(out.view(torch.int32), C.mask_rows(masks, *args).view(torch.int32))
        if args[0] is not None:
            picks.add(args[0].numpy().tobytes())
            with_picks += 1
    assert with_picks >= steps and len(picks) == with_picks               # every phase drew its own picks


def test_two_jobs_in_flight_one_masked_one_not():
    from tests import realarch as R
    pipe = _small_pipe(torch.float32, scales=(1.0, 0.5))
    left, right_box = _left_right()
    jobs = []
    for k, (prompt, seed) in enumerate((("p", 11), ("q", 12))):
        e, neg = _embeds(1, seed=20 + k)
        jobs.append(dict(prompts=prompt, seed=seed, ip_adapter_image_embeds=e, ip_adapter_negative_image_embeds=neg))
    jobs[0]["ip_adapter_masks"] = [left, right_box]
    alone = []
    for j in jobs:
        pipe.text_encoder = R.embed_fn(False)
        pipe.seed_everything(j["seed"])
        alone.append(pipe.generate_latents(j["prompts"], "", **SMALL_RUN, **{k: v for k, v in j.items() if k not in ("prompts", "seed")}).clone())
    pipe.text_encoder = R.embed_fn(False)
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **SMALL_RUN)
    for z, want in zip(got, alone):
        assert R.rel_l2(z, want) < 1e-5, R.rel_l2(z, want)


def test_command_line_takes_two_masks(tmp_path):
    import glob
    from PIL import Image
    from safetensors.torch import save_file
    from elasticdiffusion_official_amd import models as M
    from tests import ip_adapter_spec as IS
    from tests import procs
    cfg = M.UNET_CONFIGS[M.family("1.5")]
    base = IS.random_adapter(cfg, NI_BASE, CLIP_DIM, seed=1, dtype=torch.float16)
    plus = MS.random_plus_adapter(cfg, NI_PLUS, EMBED_DIM, seed=2, dtype=torch.float16)
    save_file({k: v.contiguous() for k, v in base.items()}, str(tmp_path / "base.safetensors"))
    save_file({k: v.contiguous() for k, v in plus.items()}, str(tmp_path / "plus.safetensors"))
    (eb, ep), neg = _embeds(1)
    torch.save(eb, str(tmp_path / "e0.pt")), torch.save(ep, str(tmp_path / "e1.pt")), torch.save(neg[1], str(tmp_path / "n1.pt"))
    Image.fromarray(_left_right()[0]).save(str(tmp_path / "left.png"))
    r = procs.run([procs.PY, "-m", "elasticdiffusion_official_amd", "--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2",
                   "--resampling_steps", "1", "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--view_batch_size", "4",
                   "--ip_adapter", f"{tmp_path / 'base.safetensors'}:0.7", "--ip_adapter", f"{tmp_path / 'plus.safetensors'}:0.4",
                   "--ip_adapter_embeds", str(tmp_path / "e0.pt"), "--ip_adapter_embeds", str(tmp_path / "e1.pt"),
                   "--ip_adapter_negative_embeds", "none", "--ip_adapter_negative_embeds", str(tmp_path / "n1.pt"),
                   "--ip_adapter_mask", str(tmp_path / "left.png"), "--ip_adapter_mask", "256,0,512,512"],
                  timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    saved = glob.glob(os.path.join(str(tmp_path), "t", "*"))
    assert len(saved) == 1 and os.path.exists(os.path.join(saved[0], "0.png"))
