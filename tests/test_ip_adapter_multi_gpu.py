"""-m gpu: several IP-Adapters at once on the device -- the one-launch A-segment decoupled cross attention
against its fp32 / fp64 statement, its limits (all weights zero, one segment alone), its memory behaviour, its rejections, the
adversarial families of tests/attention_cases.py extended to A segments, the dispatch of models.Attention, the reduced-width XL
forward with a base and a Plus adapter, the product loop against the oracle, graph replay across a change of scales, the encoder
path, jobs in flight and the command line."""
import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import attention_cases as A
from tests import ip_adapter_multi_spec as MS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
SEGMENTATIONS = [(1, 1), (4, 4), (16, 16), (3, 5), (13, 19), (4, 16, 4), (1, 30, 1), (8, 8, 8, 8), (31, 1)]
WEIGHTS = (0.6, 1.0, -0.5, 0.3)
ABS = {torch.bfloat16: 3e-2, torch.float16: 6e-3}     # test_flash_attention_never_reads_past_the_keys' bar for |v| ~ 1


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _w(values):
    return torch.tensor(list(values), dtype=torch.float32, device=DEV)


def _heads(t, H):
    return t.reshape(t.shape[0], -1, H, 64).transpose(1, 2)


def _sdpa(q, k, v, H):
    return F.scaled_dot_product_attention(_heads(q, H), _heads(k, H), _heads(v, H), scale=0.125).transpose(1, 2).reshape(q.shape)


def _plain(q, k, v, H, nt, segs, w):
    """the plain route: A + 1 SDPA calls and the axpys in the same dtype"""
    out = _sdpa(q, k[:, :nt], v[:, :nt], H)
    for a, (lo, hi) in enumerate(MS.segments(nt, segs)[1:]):
        out = out + w[a] * _sdpa(q, k[:, lo:hi], v[:, lo:hi], H)
    return out


def _qkv(B, H, Nq, N, dtype, seed):
    """test_ip_adapter_gpu._qkv: k | v as the column halves of one [B, N, 2 inner] tensor"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, device=DEV, generator=g).mul(1.5).to(dtype)
    kv = torch.randn(B, N, 2 * H * 64, device=DEV, generator=g)
    kv[..., :H * 64] *= 1.5
    kv = kv.to(dtype)
    return q, kv[..., :H * 64], kv[..., H * 64:]


# ---- kernel vs fp32 statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H", [(2, 3), (1, 10)])
@pytest.mark.parametrize("Nq", [1, 100, 513])
@pytest.mark.parametrize("Nt", [1, 77, 96, 97, 154, 160])
def test_multi_adapter_attention_against_fp32(dtype, B, H, Nq, Nt):
    """ops.flash_attention_ipn vs A + 1 fp32 softmaxes under test_decoupled_cross_attention_against_fp32's bar, relative to the
    plain route measured here (A + 1 SDPA calls and the axpys in the same dtype); strided k / v give the contiguous bits."""
    ops = _ops()
    for segs in SEGMENTATIONS:
        w = WEIGHTS[:len(segs)]
        q, k, v = _qkv(B, H, Nq, Nt + sum(segs), dtype, Nq * 7 + Nt * 3 + sum(segs) + 100 * len(segs))
        got = ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w))
        ref = MS.multi_ref(q, k, v, H, Nt, segs, w, torch.float32)
        plain = _plain(q, k, v, H, Nt, segs, w)
        assert got.shape == (B, Nq, H * 64) and got.dtype == dtype and got.is_contiguous() and bool(torch.isfinite(got).all())
        err, err_p = float((got.float() - ref).abs().max()), float((plain.float() - ref).abs().max())
        rel, rel_p = float((got.float() - ref).norm() / ref.norm()), float((plain.float() - ref).norm() / ref.norm())
        print(f"ipn {dtype} B{B} H{H} Nq{Nq} Nt{Nt} segs{segs}: max|err| {err:.2e} (plain {err_p:.2e})  rel {rel:.2e} (plain {rel_p:.2e})")
        assert rel < 1.5 * rel_p + 1e-4, (segs, rel, rel_p)
        assert err < 3.0 * err_p + 4e-3, (segs, err, err_p)
        assert torch.equal(got, ops.flash_attention_ipn(q, k.contiguous(), v.contiguous(), H, Nt, segs, _w(w)))


# ---- all weights zero -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nt", [77, 154])
@pytest.mark.parametrize("segs", [(4, 4), (16, 16), (8, 8, 8, 8)])
def test_all_weights_zero_is_the_text_only_kernel_bit_for_bit(dtype, Nt, segs):
    ops = _ops()
    for B, H, Nq in ((2, 3, 513), (1, 10, 100)):
        q, k, v = _qkv(B, H, Nq, Nt + sum(segs), dtype, Nt + sum(segs))
        got = ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w([0.0] * len(segs)))
        assert torch.equal(got, ops.flash_attention(q, k[:, :Nt], v[:, :Nt], H, v_path=8))


# ---- one segment alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_text_values_and_a_unit_weight_leave_that_segment_alone(dtype):
    """v_t = 0 and w = e_a: out = rn16(sum_j v_j p^_j) with p^_j = rn16(e_j * inv_a), where the small-KV kernel on segment a alone
    stores rn16((sum_j v_j e^_j) * inv_a) with e^_j = rn16(e_j).  Both sums run over the same e_j (same MFMA chains on the same
    scores, same maximum), so with eps = half an ulp of the 16-bit type, relative:
      * the packed factors differ by (1 + d_j) / (1 + d'_j), |d|, |d'| <= eps: the sums differ by <= 2 eps * sum_j |v_j| p_j;
      * each result is rounded once to 16 bit: eps * (|out| + |alone|);
      * fp32: fl(w * inv) and fl(e * c) (2 roundings of 2^-24 per factor) and <= 32 accumulation steps per sum, twice:
        < 2^-18 * sum_j |v_j| p_j;
      * fp16 only: a factor below 2^-14 is subnormal, rounded to 2^-25 absolute in either kernel: 2 * 2^-25 * sum_j |v_j|,
        and a stored value below 2^-14 likewise: 2 * 2^-25.
    1 % is allowed for second-order terms.  The other segments' p_j are finite values times zero: exact zeros."""
    ops = _ops()
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    H = 3
    for Nt, segs in ((77, (4, 4)), (154, (16, 16)), (96, (13, 19)), (77, (8, 8, 8, 8)), (154, (1, 30, 1))):
        q, k, v = _qkv(2, H, 300, Nt + sum(segs), dtype, 5 * Nt + sum(segs))
        v = v.clone()
        v[:, :Nt] = 0
        for a, (lo, hi) in enumerate(MS.segments(Nt, segs)[1:]):
            w = [0.0] * len(segs)
            w[a] = 1.0
            got = ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w)).double()
            alone = ops.flash_attention(q, k[:, lo:hi].contiguous(), v[:, lo:hi].contiguous(), H, v_path=8).double()
            s_abs = MS.softmax_v(q, k[:, lo:hi], v[:, lo:hi].abs(), H)                   # sum_j |v_j| p_j, float64
            bound = 1.01 * ((2.0 * eps + 2.0 ** -18) * s_abs + eps * (got.abs() + alone.abs()))
            if dtype == torch.float16:
                bound = bound + 2.0 ** -24 * (v[:, lo:hi].double().abs().sum(1, keepdim=True) + 1.0)
            over = float(((got - alone).abs() - bound).max())
            print(f"alone {dtype} Nt{Nt} segs{segs} a{a}: max|d| {float((got - alone).abs().max()):.2e}, max(d - bound) {over:.2e}")
            assert over <= 0.0, (Nt, segs, a, over)


# ---- never reads past the keys ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nt", [129, 154])
@pytest.mark.parametrize("segs", [(4, 4), (13, 18), (8, 8, 8, 8)])
def test_multi_adapter_attention_never_reads_past_the_keys(dtype, Nt, segs):
    """NaN / Inf in 64 rows in front of the first text key and in 192 rows behind the last image key of EVERY batch entry
    (attention_cases.poisoned): the masked rows of the text blocks and of the image block come from the row check, not from
    memory.  Bar: test_decoupled_cross_attention_never_reads_past_the_keys' (the dtype's absolute bar times 1 + sum |w|)."""
    ops = _ops()
    B, H, Nq, N = 2, 3, 256, Nt + sum(segs)
    w = WEIGHTS[:len(segs)]
    q, k, v = A.gaussian(dtype, 64, B, H, Nq, N, N, DEV)
    kp, vp = A.poisoned(k, v, 64, 3 * 64)
    got = ops.flash_attention_ipn(q, kp, vp, H, Nt, segs, _w(w))
    assert bool(torch.isfinite(got).all())
    ref = MS.multi_ref(q, k, v, H, Nt, segs, w)
    assert float((got.double() - ref).abs().max()) < (1.0 + sum(abs(x) for x in w)) * ABS[dtype]
    assert torch.equal(got, ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w)))


# ---- fault isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_keys_in_one_batch_entry_leave_the_others_bit_equal(dtype):
    ops = _ops()
    B, H, Nq, Nt, segs = 3, 3, 200, 77, (4, 16, 4)
    q, k, v = _qkv(B, H, Nq, Nt + sum(segs), dtype, 41)
    w = _w(WEIGHTS[:3])
    clean = ops.flash_attention_ipn(q, k, v, H, Nt, segs, w)
    k2, v2 = k.clone(), v.clone()
    k2[1, 5], k2[1, Nt + 6], v2[1, Nt + 21] = float("nan"), float("inf"), float("nan")
    got = ops.flash_attention_ipn(q, k2, v2, H, Nt, segs, w)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    assert not bool(torch.isfinite(got[1]).all())


# ---- rejections -----------------------------------------------------------------------------------------------------------------------
def test_shapes_outside_the_multi_kernel_are_rejected_and_the_next_launch_is_clean():
    import ctypes
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    q = torch.randn(1, 64, 128, device=DEV).half()
    kv = torch.randn(1, 200, 128, device=DEV).half()
    w4 = _w(WEIGHTS)
    cases = [(77, ()), (77, (4, 4, 4, 4, 4)), (77, (4, 0)), (77, (16, 17)), (161, (4, 4))]
    for nt, segs in cases:                    # A = 0; A = 5; a zero-length segment; 33 image keys; Nt = 161
        n = nt + sum(segs)
        with pytest.raises(RuntimeError):
            ops.flash_attention_ipn(q, kv[:, :n], kv[:, :n], 2, nt, segs, torch.zeros(len(segs), device=DEV))
    q40, kv40 = torch.randn(1, 64, 80, device=DEV).half(), torch.randn(1, 85, 80, device=DEV).half()
    with pytest.raises(RuntimeError):
        ops.flash_attention_ipn(q40, kv40, kv40, 2, 77, (4, 4), w4[:2])                   # head dimension 40
    with pytest.raises(RuntimeError):
        ops.flash_attention_ipn(q.float(), kv[:, :85].float(), kv[:, :85].float(), 2, 77, (4, 4), w4[:2])   # a 32-bit dtype
    with pytest.raises(RuntimeError):
        ops.flash_attention_ipn(q, kv[:, :85], kv[:, :85], 2, 77, (4, 4), w4[:2].cpu())   # host weights
    # the C entry point refuses the same by itself, before any launch
    out = torch.empty_like(q)
    for nt, segs, hd, code in [(nt, segs, 64, 1) for nt, segs in cases] + [(77, (4, 4), 40, 1), (77, (4, 4), 64, 0)]:
        ni = (ctypes.c_int32 * max(1, len(segs)))(*segs)
        err = _hip.lib().ed_flash_attention_ipn(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), out.data_ptr(), code, 1, 2, 64, nt, len(segs),
                                                ctypes.addressof(ni), hd, q.stride(0), q.stride(1), kv.stride(0), kv.stride(1),
                                                kv.stride(0), kv.stride(1), out.stride(0), out.stride(1), 0.125, w4.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        assert err == 1, (nt, segs, hd, code, err)                                         # hipErrorInvalidValue
    torch.cuda.synchronize()
    k = kv[:, :85].contiguous()
    got = ops.flash_attention_ipn(q, k, k, 2, 77, (4, 4), w4[:2])
    torch.cuda.synchronize()
    assert float((got.double() - MS.multi_ref(q, k, k, 2, 77, (4, 4), WEIGHTS)).abs().max()) < 2.6 * ABS[torch.float16]


# ---- adversarial families, extended to A segments -----------------------------------------------------------------------------------
def _with_segments(dtype, q, kt, vt, H, segs, seed, builder=A.gaussian, outlier_in=None):
    """image rows of ``builder`` behind the text rows; ``outlier_in`` = a: late_outlier's query row scores 180 against the LAST key
    of segment a (its softmax is one-hot: that segment contributes w[a] times one V row)"""
    _, ki, vi = builder(dtype, 64, kt.shape[0], H, A.MIN_NQ, sum(segs), seed, DEV)
    ki, vi = ki.clone(), vi.clone()
    if outlier_in is not None:
        b, h, row = A._at("late_outlier", q.shape[0], H)
        qr = q[b, row, h * 64:(h + 1) * 64].float()
        key = sum(segs[:outlier_in + 1]) - 1
        ki[b, key, h * 64:(h + 1) * 64] = (qr * (180.0 * 8.0 / float(qr.pow(2).sum()))).to(dtype)
    return torch.cat([kt, ki], 1), torch.cat([vt, vi], 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nt", [1, 33, 64, 65, 77, 96, 97, 160])
def test_multi_kernel_on_planted_rows(Nt, dtype):
    """attention_cases.combined without the creeping maximum (a one-pass kernel) at both ends of every text key class: outlier key,
    first-tile maximum, all-negative row and uniform row on the text side, an outlier key inside one image segment, against
    float64.  Four launches give the same bits (the LDS-race screen)."""
    ops = _ops()
    B, H, Nq = 1, 3, 100
    q, kt, vt = A.combined(dtype, 64, B, H, Nq, Nt, 11 + Nt, DEV, creeping=False)
    for segs, hot in (((1, 1), 1), ((13, 19), 0), ((4, 16, 4), 1), ((8, 8, 8, 8), 3)):
        w = WEIGHTS[:len(segs)]
        k, v = _with_segments(dtype, q, kt, vt, H, segs, 500 + sum(segs), outlier_in=hot)
        got = ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w))
        for _ in range(3):
            assert torch.equal(ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w)), got)
        ref = MS.multi_ref(q, k, v, H, Nt, segs, w)
        bar = ABS[dtype] * (1.0 + sum(abs(x) for x in w))
        err = float((got.double() - ref).abs().max())
        print(f"planted {dtype} Nt{Nt} segs{segs}: max|err| {err:.2e} (bar {bar:.2e})")
        assert bool(torch.isfinite(got).all()) and err < bar
        # rows whose value is known without a reference: q = 0 gives the mean of V per segment ...
        b2, _, row2 = A._at("uniform_row", B, H)
        mean = v[b2, :Nt].double().mean(0)
        for a, (lo, hi) in enumerate(MS.segments(Nt, segs)[1:]):
            mean = mean + w[a] * v[b2, lo:hi].double().mean(0)
        assert float((got[b2, row2].double() - mean).abs().max()) < min(2e-2, ABS[dtype]) * (1.0 + sum(abs(x) for x in w))
        # ... and the outlier row: one text V row, one V row of the hot segment, the other segments' softmaxes
        b, h, row = A._at("late_outlier", B, H)
        hs = slice(h * 64, (h + 1) * 64)
        want = vt[b, A.outlier_key(Nt), hs].double()
        for a, (lo, hi) in enumerate(MS.segments(Nt, segs)[1:]):
            if a == hot:
                want = want + w[a] * v[b, hi - 1, hs].double()
            else:
                want = want + w[a] * MS.softmax_v(q[b:b + 1, row:row + 1, hs], k[b:b + 1, lo:hi, hs], v[b:b + 1, lo:hi, hs], 1)[0, 0]
        assert float((got[b, row, hs].double() - want).abs().max()) < bar


def test_multi_kernel_large_values_stay_finite():
    """fp16, |v| up to 3e4 in the text rows and in every segment; weights with 1 + sum |w| = 1.9, so every exact output stays below
    65504.  The error is linear in V: the absolute bar times max |v|."""
    ops = _ops()
    dtype, B, H, Nq, Nt = torch.float16, 1, 3, 100, 77
    q, kt, vt = A.large_v(dtype, 64, B, H, Nq, Nt, 5, DEV)
    for segs, w in (((16, 16), (0.6, -0.3)), ((4, 16, 4), (0.3, -0.3, 0.3))):
        k, v = _with_segments(dtype, q, kt, vt, H, segs, 900 + len(segs), builder=A.large_v)
        got = ops.flash_attention_ipn(q, k, v, H, Nt, segs, _w(w))
        assert bool(torch.isfinite(got).all())
        ref = MS.multi_ref(q, k, v, H, Nt, segs, w)
        err = float((got.double() - ref).abs().max())
        print(f"large v segs{segs}: max|err| {err:.3e}")
        assert err < ABS[dtype] * A.V_LARGE * 1.9
        assert float(got.float().abs().max()) <= A.V_LARGE * 1.9


# ---- dispatch: launch counts from ops.TIMER ---------------------------------------------------------------------------------------
def _attention_with_two_adapters(dim, heads, head_dim, cross, segs, w, seed):
    from elasticdiffusion_official_amd import models as M
    torch.manual_seed(seed)
    a = M.Attention(dim, heads, head_dim, cross_dim=cross)
    lin = lambda: torch.nn.Linear(cross, heads * head_dim, bias=False)   # noqa: E731
    a.set_ip_adapter(lin(), lin(), segs[0])
    a.add_ip_adapter(lin(), lin(), segs[1], torch.tensor(w, dtype=torch.float32))
    return a.eval().requires_grad_(False)


@pytest.mark.parametrize("head_dim,want", [(64, {"ed_flash_attention_ipn": 1}), (40, {"ed_flash_attention": 3})])
def test_attention_module_takes_one_launch_with_two_adapters_where_the_kernel_applies(head_dim, want):
    ops = _ops()
    heads, segs, w = (10 if head_dim == 64 else 8), (4, 16), (0.75, 0.5)
    a32 = _attention_with_two_adapters(heads * head_dim, heads, head_dim, 64, segs, w, 3)
    a16 = copy.deepcopy(a32).to(DEV, torch.float16)
    a16.ip_weights = a32.ip_weights.to(DEV)                                # (the UNet owns this tensor; a bare module is handed it)
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(2, 1024, heads * head_dim, device=DEV, generator=g).half()
    ctx = torch.randn(2, 77 + sum(segs), 64, device=DEV, generator=g).half()
    ops.TIMER.start()
    try:
        with torch.no_grad():
            got = a16(x, ctx)
    finally:
        timed = ops.TIMER.stop()
    seen = {k: v[0] for k, v in timed.items() if k.startswith("ed_flash_attention")}
    assert seen == want, seen
    with torch.no_grad():
        assert torch.equal(got, a16(x, ctx, kv=a16.project_kv(ctx)))
        a32 = a32.to(DEV)
        a32.ip_weights = a16.ip_weights
        ref = a32(x.float(), ctx.float())                                  # fp32: the plain torch path
    assert float((got.float() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    # the device weights are read at run time, on either path
    a16.ip_weights.copy_(torch.tensor([0.0, 0.0]))
    with torch.no_grad():
        zero = a16(x, ctx)
        a16.set_ip_adapter()
        text_only = a16(x, ctx[:, :77].contiguous())
    assert float((zero.float() - text_only.float()).abs().max()) <= 1e-3 * float(ref.abs().max())
    assert float((got.float() - text_only.float()).abs().max()) > 1e-2 * float(ref.abs().max())   # (ten times the bar above: the adapters show)


# ---- reduced-width architectures with a base and a Plus adapter -------------------------------------------------------------------
NI_BASE, NI_PLUS, CLIP_DIM, EMBED_DIM, SEQ = 4, 16, 48, 80, 10


def _adapters_for(sd, dtype=torch.float32, gain=4.0):
    from elasticdiffusion_official_amd import models as M
    from tests import ip_adapter_spec as IS
    cfg = M.SMALL_UNET_CONFIGS["sdxl" if sd.startswith("XL") else "sd15"]
    return [IS.random_adapter(cfg, NI_BASE, CLIP_DIM, seed=5, dtype=dtype, gain=gain),
            MS.random_plus_adapter(cfg, NI_PLUS, EMBED_DIM, seed=6, dtype=dtype, gain=gain)]


def _embeds(B=1, seed=8):
    """([base, Plus] embeddings, [None, Plus] negative embeddings)"""
    g = torch.Generator().manual_seed(seed)
    e = [torch.randn(B, CLIP_DIM, generator=g), 2.0 * torch.randn(B, SEQ, EMBED_DIM, generator=g)]
    return e, [None, 2.0 * torch.randn(1, SEQ, EMBED_DIM, generator=g)]


def _install_both(unet, adapters, scales):
    unet.install_ip_adapter(adapters[0])
    unet.install_ip_adapter(adapters[1], add=True)
    unet.ip_scales = scales
    return unet


def test_real_architecture_forward_with_two_adapters(monkeypatch):
    """One fp16 6-row forward of the reduced-width XL UNet with a base (4 tokens) and a Plus (16 tokens) adapter on 77 + 20 and
    154 + 20 tokens against its own fp32 CPU forward: rel-L2 at most twice the same forward's text-only figure, measured here
    (section 24.6's factor); hoisted and in-forward k|v agree bit for bit."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    from tests import realarch as R
    sd = "XL1.0"
    unet, vae, _ = R.build_small(sd)
    adapters = _adapters_for(sd)
    S = unet.config.sample_size // 2
    g = torch.Generator().manual_seed(21)
    x = torch.randn(6, 4, S, S, generator=g)
    text = torch.randn(6, 154, 64, generator=g)
    pooled = torch.randn(6, 32, generator=g)
    (eb, ep), _ = _embeds(6)
    t = torch.tensor(500)
    kw = {"added_cond_kwargs": {"text_embeds": pooled, "time_ids": torch.zeros(6, 6)}}
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    pipe = ElasticDiffusion(DEV, sd, view_batch_size=4, unet=copy.deepcopy(unet).to(torch.float16), vae=copy.deepcopy(vae),
                            text_encoder=lambda s: None, use_graphs=False)

    def forwards(txt):
        outs = []
        for once in (True, False):
            pipe.TEXT_KV_ONCE = once
            txt16 = txt.to(DEV, torch.float16)
            kv = pipe._text_kv(txt16)
            assert (kv is not None) == once
            outs.append(pipe._forward_rows(x.to(DEV, torch.float16), t.to(DEV), txt16, pooled.to(DEV, torch.float16), None, kv).float().cpu())
        return outs
    rel0 = {}
    with torch.no_grad():
        for n in (77, 154):
            txt = text[:, :n].contiguous()
            rel0[n] = R.rel_l2(forwards(txt)[0], unet(x, t, encoder_hidden_states=txt, **kw)["sample"])
        pipe.load_ip_adapter(adapters[0], scale=0.75)
        pipe.load_ip_adapter(adapters[1], scale=0.5, add=True)
        assert pipe.ip_adapters == [("ip_adapter", 0.75, NI_BASE, "base"), ("ip_adapter", 0.5, NI_PLUS, "plus")]
        assert pipe.ip_adapter == ("ip_adapter", 0.75, NI_BASE)
        _install_both(unet, adapters, [0.75, 0.5])
        tokens = torch.cat([unet.ip_image_tokens(eb, 0), unet.ip_image_tokens(ep, 1)], dim=1)
        for n in (77, 154):
            txt = torch.cat([text[:, :n], tokens], dim=1).contiguous()
            want = unet(x, t, encoder_hidden_states=txt, **kw)["sample"]
            outs = forwards(txt)
            rel = R.rel_l2(outs[0], want)
            print(f"real-arch {sd} fp16 forward with two adapters on {n}+{NI_BASE}+{NI_PLUS} tokens vs fp32 CPU: rel-L2 {rel:.3e} "
                  f"(text-only {rel0[n]:.3e})")
            assert bool(torch.isfinite(outs[0]).all()) and rel <= 2.0 * rel0[n], (n, rel, rel0[n])
            assert torch.equal(outs[0], outs[1])


def _ip_embed_fn(xl, un_tok, co_tok):
    from tests import realarch as R
    base = R.embed_fn(xl)
    state = {"n": 0}

    def fn(p):
        e, pooled = base(p)
        state["n"] += 1
        tok = un_tok if state["n"] % 2 == 1 else co_tok
        return torch.cat([e, tok.to(e.dtype)], dim=1), pooled
    return fn


@pytest.mark.parametrize("case", ["cfg2_sd_512x1024", "cfg3_xl_1024x2048"])
def test_product_loop_with_two_adapters_against_the_oracle(case):
    """The fp32 product with a base and a Plus adapter against ElasticOracle driven with [text | tokens 0 | tokens 1] and the same
    UNet on the CPU: the project's per-step 1e-3 with the RNG tail equal; all weights zero within 1e-5 of text-only, weights (1, 1)
    more than 1e-3 away."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    from oracle.ddim import DDIMOracle
    from oracle.elastic_oracle import ElasticOracle
    from tests import realarch as R
    c = R.REAL_CASES[case]
    xl = c["sd"].startswith("XL")
    unet, vae, _ = R.build_small(c["sd"])
    adapters = _adapters_for(c["sd"])
    (eb, ep), neg = _embeds(1)
    run = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **R.LOOP_KW)
    cpu = _install_both(copy.deepcopy(unet), adapters, [1.0, 1.0])
    un_tok = torch.cat([cpu.ip_image_tokens(torch.zeros_like(eb), 0), cpu.ip_image_tokens(neg[1], 1)], dim=1)
    co_tok = torch.cat([cpu.ip_image_tokens(eb, 0), cpu.ip_image_tokens(ep, 1)], dim=1)
    orc = ElasticOracle(cpu, vae, DDIMOracle(), _ip_embed_fn(xl, un_tok, co_tok), sd_version=c["sd"], view_batch_size=c["vbs"],
                        pooled_dim=32 if xl else None)
    orc.seed_everything(c["seed"])
    want = []
    orc.generate_latent("p", "", trace=want, **run)
    tail = torch.rand(4)
    pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=copy.deepcopy(unet), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(xl))

    def product(**kw):
        pipe.text_encoder = R.embed_fn(xl)
        pipe.seed_everything(c["seed"])
        trace = []
        pipe.generate_latents("p", "", trace=trace, **run, **kw)
        return [z.cpu() for z in trace], torch.rand(4)
    text_only, _ = product()
    pipe.load_ip_adapter(adapters[0], scale=1.0)
    pipe.load_ip_adapter(adapters[1], scale=1.0, add=True)
    ip = dict(ip_adapter_image_embeds=[eb, ep], ip_adapter_negative_image_embeds=neg)
    got, t1 = product(**ip)
    rels = [R.rel_l2(a, b) for a, b in zip(got, want)]
    print(f"{case} fp32 loop with two adapters vs oracle, per step: {['%.2e' % r for r in rels]}")
    assert len(got) == len(want) == c["steps"] and max(rels) < 1e-3, rels
    assert torch.equal(t1, tail)
    pipe.set_ip_adapter_scale([0.0, 0.0])
    zero, _ = product(**ip)
    d0, d1 = R.rel_l2(zero[-1], text_only[-1]), R.rel_l2(got[-1], text_only[-1])
    print(f"{case}: weights (0, 0) vs text-only {d0:.2e}, weights (1, 1) vs text-only {d1:.2e}")
    assert d0 < 1e-5 and d1 > 1e-3
    assert pipe._runner.stats()["eager"] == 0


# ---- graphs, the encoder path, jobs in flight, the command line ---------------------------------------------------------------------
SMALL_RUN = dict(height=512, width=512, num_inference_steps=2, guidance_scale=10.0, resampling_steps=1, new_p=0.3, rrg_stop_t=0.4,
                 rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)


def _small_pipe(dtype=torch.float16):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from tests import realarch as R
    unet, vae, _ = R.build_small("1.5")
    return ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=copy.deepcopy(unet).to(dtype), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(False))


def test_a_change_of_scales_replays_the_captured_graphs(monkeypatch):
    """Three images through the graphs with two adapters, set_ip_adapter_scale([...]), one more: no entry is added or dropped,
    nothing runs eagerly, and the image equals the one a fresh pipeline loaded at those scales gives, bit for bit (deterministic
    library algorithms, section 23.6); after unload_ip_adapter() the text-only image is the first one again."""
    from tests import realarch as R
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    adapters = _adapters_for("1.5")
    (eb, ep), neg = _embeds(1)
    ip = dict(ip_adapter_image_embeds=[eb, ep], ip_adapter_negative_image_embeds=neg)

    def run(pipe, seed=3, **kw):
        pipe.text_encoder = R.embed_fn(False)
        pipe.seed_everything(seed)
        return pipe.generate_latents("p", "", **SMALL_RUN, **kw).clone()
    pipe = _small_pipe()
    first = run(pipe)
    pipe.load_ip_adapter(adapters[0], scale=0.7)
    pipe.load_ip_adapter(adapters[1], scale=0.4, add=True)
    imgs = [run(pipe, seed, **ip) for seed in (3, 4, 5)]
    entries, stats = len(pipe._runner.entries), pipe._runner.stats()
    assert entries >= 1 and stats["eager"] == 0 and stats["captured"] >= 1
    pipe.set_ip_adapter_scale([0.3, 0.9])
    assert len(pipe._runner.entries) == entries
    after = run(pipe, 3, **ip)
    assert len(pipe._runner.entries) == entries and pipe._runner.stats()["eager"] == 0
    assert pipe._runner.stats()["captured"] == stats["captured"]           # replayed, not captured again
    assert [a[1] for a in pipe.ip_adapters] == [0.3, 0.9]
    fresh = _small_pipe()
    fresh.load_ip_adapter(adapters[0], scale=0.3)
    fresh.load_ip_adapter(adapters[1], scale=0.9, add=True)
    assert torch.equal(after, run(fresh, 3, **ip)) and not torch.equal(after, imgs[0])
    pipe.set_ip_adapter_scale(0.7, name="ip_adapter")                       # by name: the first adapter of that name
    assert [a[1] for a in pipe.ip_adapters] == [0.7, 0.9]
    with pytest.raises(ValueError, match="fifth"):
        for _ in range(3):
            pipe.load_ip_adapter(adapters[0], add=True)
    pipe.unload_ip_adapter()
    assert pipe.ip_adapter is None and pipe.ip_adapters == [] and pipe.unet.ip_tokens == 0
    assert torch.equal(run(pipe), first)


def test_plus_adapter_through_an_encoder_callable(monkeypatch):
    """ip_adapter_image with a Plus adapter: the callable sees the all-zero picture once and the real picture once, and the result
    equals the embeds form (with the zero picture's output as negative embeddings) bit for bit"""
    from tests import realarch as R
    from tests.test_ip_adapter import picture
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    pipe = _small_pipe()
    plus = _adapters_for("1.5")[1]
    proj = torch.randn(SEQ * EMBED_DIM, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen = []

    def encoder(pixels):
        seen.append(pixels)
        return (pixels.mean((2, 3)) @ proj.t() + 0.1).reshape(pixels.shape[0], SEQ, EMBED_DIM)
    pipe.load_ip_adapter(plus, scale=1.0, image_encoder=encoder)
    assert pipe.ip_adapters == [("ip_adapter", 1.0, NI_PLUS, "plus")]
    pipe.seed_everything(3)
    a = pipe.generate_latents("p", "", ip_adapter_image=torch.from_numpy(picture("landscape")), **SMALL_RUN).clone()
    assert len(seen) == 2 and sorted(bool(s.any()) for s in seen) == [False, True]
    real = seen[0] if bool(seen[0].any()) else seen[1]
    pipe.text_encoder = R.embed_fn(False)
    pipe.seed_everything(3)
    b = pipe.generate_latents("p", "", ip_adapter_image_embeds=encoder(real), ip_adapter_negative_image_embeds=encoder(torch.zeros_like(real)),
                              **SMALL_RUN)
    assert torch.equal(a, b)


def test_interleaved_jobs_with_their_own_lists():
    from tests import realarch as R
    pipe = _small_pipe(torch.float32)
    adapters = _adapters_for("1.5")
    pipe.load_ip_adapter(adapters[0], scale=1.0)
    pipe.load_ip_adapter(adapters[1], scale=0.5, add=True)
    jobs = []
    for k, (prompt, seed) in enumerate((("p", 11), ("q", 12))):
        e, neg = _embeds(1, seed=20 + k)
        jobs.append(dict(prompts=prompt, seed=seed, ip_adapter_image_embeds=e, ip_adapter_negative_image_embeds=neg))
    alone = []
    for j in jobs:
        pipe.text_encoder = R.embed_fn(False)
        pipe.seed_everything(j["seed"])
        alone.append(pipe.generate_latents(j["prompts"], "", ip_adapter_image_embeds=j["ip_adapter_image_embeds"],
                                           ip_adapter_negative_image_embeds=j["ip_adapter_negative_image_embeds"], **SMALL_RUN).clone())
    assert R.rel_l2(alone[0], alone[1]) > 1e-3
    pipe.text_encoder = R.embed_fn(False)
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **SMALL_RUN)
    for z, want in zip(got, alone):
        assert R.rel_l2(z, want) < 1e-5, R.rel_l2(z, want)


def test_command_line_takes_two_adapters(tmp_path):
    import glob
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
    r = procs.run([procs.PY, "-m", "elasticdiffusion_official_amd", "--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2",
                   "--resampling_steps", "1", "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--view_batch_size", "4",
                   "--ip_adapter", f"{tmp_path / 'base.safetensors'}:0.7", "--ip_adapter", f"{tmp_path / 'plus.safetensors'}:0.4",
                   "--ip_adapter_embeds", str(tmp_path / "e0.pt"), "--ip_adapter_embeds", str(tmp_path / "e1.pt"),
                   "--ip_adapter_negative_embeds", "none", "--ip_adapter_negative_embeds", str(tmp_path / "n1.pt")],
                  timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "installed at scale 0.7: 4 image tokens (base)" in r.stdout and "installed at scale 0.4: 16 image tokens (plus)" in r.stdout
    saved = glob.glob(os.path.join(str(tmp_path), "t", "*"))
    assert len(saved) == 1 and os.path.exists(os.path.join(saved[0], "0.png"))
