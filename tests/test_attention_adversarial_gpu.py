"""-m gpu: every attention kernel instantiation ops can reach (tests/attention_cases.py: TARGETS) on the adversarial inputs that
tests/test_unet_kernels.py holds the head-dim-64 online-softmax kernels to -- planted rows for the running maximum, NaN / Inf
around EVERY batch entry of K and V, finite rows of another softmax next to them, block mappings with a partial group behind full
ones, strided operands, |v| at the end of fp16 -- against the float64 reference of tests/attention_cases.py, whose CPU test
(tests/test_attention_cases.py) proves that the inputs have the properties claimed here.

Bars (the project's own): Gaussian data under test_flash_attention's SDPA-relative bar; planted rows and poisoned layouts under
test_flash_attention_never_reads_past_the_keys' absolute bar (3e-2 bf16 / 6e-3 fp16 for |v| ~ 1), times 1 + ip_scale for the IP
kernel (test_ip_adapter_gpu.py) and times max|v| for large_v (the error is linear in V).  gen, small-KV and IP launch four times
wherever they run here and must give the same bits (the LDS-race screen of the GEMM tests)."""
import pytest
import torch
import torch.nn.functional as F

from tests import attention_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
ABS = {torch.bfloat16: 3e-2, torch.float16: 6e-3}
IP_SCALE = 0.6
B, H, NQ = 1, 3, 100
ONLINE_NK = 313
ONE_PASS_NK = (1, 33, 64, 65, 77, 96, 97, 160)
IDS = [t.name for t in A.TARGETS]


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _sdpa(q, k, v, heads, scale):
    Bn, Nq, HD = q.shape
    qh, kh, vh = (t.contiguous().reshape(Bn, -1, heads, HD // heads).transpose(1, 2) for t in (q, k, v))
    return F.scaled_dot_product_attention(qh, kh, vh, scale=scale).transpose(1, 2).reshape(Bn, Nq, HD)


def _library(t, q, k, v, heads, n_text=None, ip_scale=None):
    """what the kernel replaces: SDPA, for the IP kernel two SDPA calls and the axpy in the same dtype"""
    if t.ip:
        return (_sdpa(q, k[:, :n_text], v[:, :n_text], heads, t.scale)
                + ip_scale * _sdpa(q, k[:, n_text:], v[:, n_text:], heads, t.scale))
    return _sdpa(q, k, v, heads, t.scale)


def _run(t, q, k, v, heads, **kw):
    """one launch; four with equal bits for the kernels that have no such check elsewhere"""
    got = t.run(_ops(), q, k, v, heads, **kw)
    if t.family in ("k_flash_attn_gen", "k_flash_attn_smallkv", "k_flash_attn_ip"):
        for _ in range(3):
            assert torch.equal(t.run(_ops(), q, k, v, heads, **kw), got), f"{t.name}: two launches differ"
    assert got.shape == q.shape and got.is_contiguous() and got.dtype == q.dtype
    return got


def _measure(tag, t, got, q, k, v, heads, **kw):
    """-> err, rel of the kernel and of the library against float64, printed side by side"""
    ref = t.ref64(q, k, v, heads, **kw)
    lib = _library(t, q, k, v, heads, **kw)
    err, err_l = float((got.double() - ref).abs().max()), float((lib.double() - ref).abs().max())
    rel, rel_l = float((got.double() - ref).norm() / ref.norm()), float((lib.double() - ref).norm() / ref.norm())
    print(f"{tag} {t.name} {str(q.dtype)[6:]} B{q.shape[0]} H{heads} Nq{q.shape[1]} Nk{k.shape[1]}: "
          f"max|err| {err:.2e} (sdpa {err_l:.2e})  rel {rel:.2e} (sdpa {rel_l:.2e})")
    assert bool(torch.isfinite(got).all()), tag
    return ref, err, rel, err_l, rel_l


def _absolute(tag, t, got, q, k, v, heads, bar, **kw):
    ref, err, _, _, _ = _measure(tag, t, got, q, k, v, heads, **kw)
    assert err < bar, (tag, t.name, err, bar)
    return ref


def _sdpa_relative(tag, t, got, q, k, v, heads, **kw):
    _, err, rel, err_l, rel_l = _measure(tag, t, got, q, k, v, heads, **kw)
    assert rel < 1.5 * rel_l + 1e-4, (tag, t.name, rel, rel_l)
    assert err < 3.0 * err_l + 4e-3, (tag, t.name, err, err_l)


def _with_image_rows(t, dtype, k, v, Ni, seed, builder=A.gaussian):
    """the IP kernel's K / V: ``Ni`` image rows behind the text rows"""
    if not t.ip:
        return k, v, {}
    _, ki, vi = builder(dtype, 64, k.shape[0], k.shape[2] // 64, A.MIN_NQ, Ni, seed, DEV)
    return torch.cat([k, ki], 1), torch.cat([v, vi], 1), dict(n_text=k.shape[1], ip_scale=IP_SCALE)


def _planted_rows_hold(t, got, v, Nk, bar_scale=1.0, image_v=None):
    """the two rows whose value is known without a reference: the outlier's V row and the mean of V (bars of
    test_flash_attention_strided_inputs_and_outlier_rows, never above the dtype's absolute bar)"""
    hd, dtype = t.head_dim, got.dtype
    b, h, row = A._at("late_outlier", got.shape[0], H)
    want = v[b, A.outlier_key(Nk), h * hd:(h + 1) * hd].double()
    b2, _, row2 = A._at("uniform_row", got.shape[0], H)
    mean = v[b2, :Nk].double().mean(0)
    if image_v is not None:
        mean = mean + IP_SCALE * image_v[b2].double().mean(0)          # q = 0: the image softmax is uniform too
        assert float((got[b2, row2].double() - mean).abs().max()) < min(2e-2, ABS[dtype]) * bar_scale
        return
    assert float((got[b, row, h * hd:(h + 1) * hd].double() - want).abs().max()) < min(3e-2, ABS[dtype]) * bar_scale
    assert float((got[b2, row2].double() - mean).abs().max()) < min(2e-2, ABS[dtype]) * bar_scale


# ---- online softmax -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t", A.ONLINE, ids=[t.name for t in A.ONLINE])
def test_online_softmax_on_planted_rows(t, dtype):
    """late_outlier, creeping_max, first_tile_max, uniform_row and all_negative in one tensor; four full tiles and a ragged one"""
    q, k, v = A.combined(dtype, t.head_dim, B, H, NQ, ONLINE_NK, 11, DEV)
    q = t.prep_q(q)                                                   # v_path 6 is judged on the queries it is given
    got = _run(t, q, k, v, H)
    _absolute("online", t, got, q, k, v, H, ABS[dtype])
    _planted_rows_hold(t, got, v, ONLINE_NK)


# ---- one pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nk", ONE_PASS_NK)
@pytest.mark.parametrize("kind", ["smallkv", "ip"])
def test_one_pass_kernels_on_planted_rows(kind, Nk, dtype):
    """the same rows without the creeping maximum, at both ends of every key class (NKB = 2, 3, 5)"""
    t = A.one_pass_target(kind, Nk)
    q, kt, vt = A.combined(dtype, 64, B, H, NQ, Nk, 11 + Nk, DEV, creeping=False)
    for Ni in ((1, 32) if t.ip else (0,)):
        k, v, kw = _with_image_rows(t, dtype, kt, vt, Ni, 500 + Ni)
        got = _run(t, q, k, v, H, **kw)
        scale = 1.0 + IP_SCALE if t.ip else 1.0
        _absolute(f"one-pass Ni{Ni}", t, got, q, k, v, H, ABS[dtype] * scale, **kw)
        _planted_rows_hold(t, got, vt, Nk, scale, image_v=v[:, Nk:] if t.ip else None)


# ---- poison around every batch entry ----------------------------------------------------------------------------------------------
def _poison_sizes(t):
    if t.ip:
        return [(n, ni) for n in (1, 64, 77, 96, 97) if t.takes(n) for ni in (1, 4, 31, 32)]
    if t.family == "k_flash_attn_smallkv":
        return [(n, 0) for n in (1, 33, 64, 65, 77, 96, 129, 160) if t.takes(n)]
    if t.family == "k_flash_attn_gen":
        return [(n, 0) for n in (1, 77, 130, 200)]
    return [(130, 0), (200, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t", A.TARGETS, ids=IDS)
def test_no_kernel_reads_a_row_outside_its_batch_entry(t, dtype):
    """NaN / Inf in 64 rows in front of batch 0 and in 192 rows behind EVERY batch entry: a row read before 0 or past Nk from any
    entry -- not only from the last one, where the earlier poison tests have it -- turns the output non-finite"""
    Bn, Nq = 2, 130
    sizes = _poison_sizes(t)
    assert sizes
    for Nk, Ni in sizes:
        q, k, v = A.gaussian(dtype, t.head_dim, Bn, H, Nq, Nk, 3 * Nk + Ni, DEV)
        k, v, kw = _with_image_rows(t, dtype, k, v, Ni, 700 + Nk + Ni)
        q = t.prep_q(q)
        kp, vp = A.poisoned(k, v, 64, 3 * 64)
        got = _run(t, q, kp, vp, H, **kw)
        _absolute(f"poison Ni{Ni}", t, got, q, k, v, H, ABS[dtype] * (1.0 + IP_SCALE if t.ip else 1.0), **kw)
        assert torch.equal(got, t.run(_ops(), q, k, v, H, **kw))           # and the layout changes no bit


# ---- finite neighbours: the IP-Adapter fallback's row slices --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [40, 64])
def test_row_slices_next_to_the_other_softmax_rows(hd, dtype):
    """models.Attention without the fused IP kernel: flash_attention(q, k[:, :77]) and (q, k[:, 77:]) on one [B, 81, inner]
    tensor.  The rows of the other softmax (here +-100) are finite, so a row read from them would pass every poison test"""
    ops = _ops()
    t = A.BY_NAME["gen/40"] if hd == 40 else A.one_pass_target("smallkv", 77)
    Bn, Nq = 2, 130
    q, kt, vt = A.gaussian(dtype, hd, Bn, H, Nq, 77, 21, DEV)
    _, ki, vi = A.gaussian(dtype, hd, Bn, H, Nq, 4, 22, DEV)
    seen, orig = [], ops._call

    def spy(name, *a):
        if name == "ed_flash_attention":
            seen.append(a[-2])
        return orig(name, *a)
    for k, v, front, behind in ((kt, vt, 0, 4), (ki, vi, 77, 0)):
        kn, vn = A.neighbours(k, v, front, behind, 100.0)
        ops._call = spy
        try:
            got = ops.flash_attention(q, kn, vn, H)
        finally:
            ops._call = orig
        for _ in range(3):
            assert torch.equal(ops.flash_attention(q, kn, vn, H), got)
        assert torch.equal(got, ops.flash_attention(q, kn.contiguous(), vn.contiguous(), H))
        _sdpa_relative(f"neighbours {front}|{behind}", t, got, q, k, v, H)
    assert seen == ([0, 0] if hd == 40 else [8, 8]), seen            # head dim 64: the default dispatch is the small-KV kernel


# ---- block mapping ----------------------------------------------------------------------------------------------------------------
MAPPED = [A.BY_NAME["gen/40"], A.BY_NAME["gen/80"], A.BY_NAME["gen/160"], A.one_pass_target("smallkv", 77), A.one_pass_target("ip", 77)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bn,Hn", [(1, 1), (1, 7), (1, 8), (3, 3), (1, 19)])
@pytest.mark.parametrize("t", MAPPED, ids=[t.name for t in MAPPED])
def test_block_mapping(t, Bn, Hn, dtype):
    """B * H = 9 and 19 put a partial group of (batch, head) pairs behind full groups of 8 in gen's mapping (its tail branch was
    reached at B * H = 2, 3 only); Nq = 513 and 1100 cross the 512 rows one small-KV / IP workgroup walks"""
    for Nq in (1, 129, 512, 513, 1100):
        q, k, v = A.gaussian(dtype, t.head_dim, Bn, Hn, Nq, 77, Nq + 31 * Bn * Hn, DEV)
        k, v, kw = _with_image_rows(t, dtype, k, v, 4, 900 + Nq)
        got = _run(t, q, k, v, Hn, **kw)
        _sdpa_relative("mapping", t, got, q, k, v, Hn, **kw)


# ---- strides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [40, 80, 160])
def test_gen_takes_fused_columns_and_every_second_batch_without_changing_a_bit(hd, dtype):
    t = A.BY_NAME[f"gen/{hd}"]
    for builder, Nq, Nk in ((A.fused_columns, 256, 256), (A.fused_columns, 200, 77), (A.every_second_batch, 200, 77)):
        q, k, v = builder(dtype, hd, 2, H, Nq, Nk, 41, DEV)
        assert not k.is_contiguous() and not v.is_contiguous()
        got = _run(t, q, k, v, H)
        assert torch.equal(got, t.run(_ops(), q.contiguous(), k.contiguous(), v.contiguous(), H))
        _sdpa_relative(builder.__name__, t, got, q, k, v, H)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Nk", [33, 77, 154])
@pytest.mark.parametrize("kind", ["smallkv", "ip"])
def test_one_pass_kernels_take_every_second_batch_without_changing_a_bit(kind, Nk, dtype):
    t = A.one_pass_target(kind, Nk)
    Ni = 4 if t.ip else 0
    q, k, v = A.every_second_batch(dtype, 64, 2, H, 200, Nk + Ni, 43, DEV)
    kw = dict(n_text=Nk, ip_scale=IP_SCALE) if t.ip else {}
    assert not q.is_contiguous() and not k.is_contiguous()
    got = _run(t, q, k, v, H, **kw)
    assert torch.equal(got, t.run(_ops(), q.contiguous(), k.contiguous(), v.contiguous(), H, **kw))
    _sdpa_relative("every_second_batch", t, got, q, k, v, H, **kw)


# ---- |v| at the end of fp16 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", A.TARGETS, ids=IDS)
def test_large_values_stay_finite(t):
    """fp16, |v| up to 3e4, at each target's smallest key count with more than one block and a ragged last one: an output is a
    convex combination of V rows, whatever order the kernel sums them in"""
    dtype, Nk = torch.float16, t.ragged_nk
    q, k, v = A.large_v(dtype, t.head_dim, B, H, NQ, Nk, 17, DEV)
    vt = v
    k, v, kw = _with_image_rows(t, dtype, k, v, 5, 18, builder=A.large_v)
    q = t.prep_q(q)
    got = _run(t, q, k, v, H, **kw)
    vmax = float(v.float().abs().max())
    assert vmax == A.V_LARGE
    bar = ABS[dtype] * vmax * (1.0 + IP_SCALE if t.ip else 1.0)
    _absolute("large_v", t, got, q, k, v, H, bar, **kw)
    assert float(got.float().abs().max()) <= A.V_LARGE * (1.0 + IP_SCALE if t.ip else 1.0)
    _planted_rows_hold(t, got, vt, Nk, vmax * (1.0 + IP_SCALE if t.ip else 1.0), image_v=v[:, Nk:] if t.ip else None)


# ---- K / V beyond 32-bit byte offsets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_token_stride_runs_the_64_bit_kernels(dtype):
    """130 keys with a token stride of 4.2 M elements: (Nk + 128) * stride * 2 bytes >= 2^31, so ops._flash_variant must leave the
    pipelined kernels (32-bit byte offsets) for k_flash_attn_fwd, whose load_row16 addresses with 64 bits; ed_flash_attention
    refuses an explicit pipelined v_path before it launches anything.  Only the 130 rows of the two 1.1 GB buffers are written."""
    ops = _ops()
    if torch.cuda.mem_get_info(torch.device(DEV))[0] < 8 * 2 ** 30:
        pytest.skip("needs 8 GiB of free device memory for two sparse 1.1 GB buffers")
    Bn, Hn, Nq, Nk, stride = 1, 2, 256, 130, 4_200_000
    t = A.BY_NAME["fwd/0"]
    q, k, v = A.gaussian(dtype, 64, Bn, Hn, Nq, Nk, 77, DEV)
    wide = []
    for src in (k, v):
        pool = torch.empty((Nk - 1) * stride + Hn * 64, dtype=dtype, device=DEV)
        view = pool.as_strided((Bn, Nk, Hn * 64), (pool.numel(), stride, 1))
        view.copy_(src)
        wide.append(view)
    kw_, vw = wide
    assert not ops._pipe_fits(Nk, stride)
    seen, orig = [], ops._call

    def spy(name, *a):
        if name == "ed_flash_attention":
            seen.append(a[-2])
        return orig(name, *a)
    ops._call = spy
    try:
        got = ops.flash_attention(q, kw_, vw, Hn)
    finally:
        ops._call = orig
    assert seen == [0], seen                                           # a k_flash_attn_fwd variant
    _sdpa_relative("wide stride", t, got, q, k, v, Hn)
    assert torch.equal(got, ops.flash_attention(q, k, v, Hn, v_path=0))
    with pytest.raises(RuntimeError):
        ops.flash_attention(q, kw_, vw, Hn, v_path=5)
    torch.cuda.synchronize()
    again = ops.flash_attention(q, k, v, Hn)                           # the next ordinary launch is clean
    torch.cuda.synchronize()
    _sdpa_relative("after the refusal", A.BY_NAME["pipe/5"], again, q, k, v, Hn)
