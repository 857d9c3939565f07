"""CPU: the adversarial attention inputs of tests/attention_cases.py really have the properties their docstrings state (judged by
the float64 reference alone), the layouts around K and V change no value, TARGETS names every kernel instantiation of
csrc/attention_kernels.hip that ops can reach, and ops._flash_variant leaves the pipelined kernels when K / V do not fit 32-bit
byte offsets.  The shapes are the ones tests/test_attention_adversarial_gpu.py runs."""
import math

import pytest
import torch

from tests import attention_cases as A

DTYPES = [torch.bfloat16, torch.float16]
HEAD_DIMS = [40, 64, 80, 160]
B, H, NQ = 1, 3, 100
ONLINE_NK = 313                                    # four full tiles and a ragged one
ONE_PASS_NK = (1, 33, 64, 65, 77, 96, 97, 160)
LOG2E = 1.4426950408889634


def _row(name, Bn, Hn):
    return A._at(name, Bn, Hn)


def _check_rows(names, q, k, v, hd, scale, Nk):
    """every planted row's property, from the float64 reference and scores (``q`` as the kernel gets it)"""
    Bn = q.shape[0]
    ref = A.attention_ref64(q, k, v, H, scale)
    assert bool(torch.isfinite(ref).all())
    if "late_outlier" in names:
        b, h, row = _row("late_outlier", Bn, H)
        s = A.scores64(q, k, H, b, h, row, scale)
        key = A.outlier_key(Nk)
        assert A.margin(s, key) > 100.0
        assert key >= (Nk // A.TILE - 1) * A.TILE if Nk >= A.TILE else key == Nk - 1      # in the last FULL tile
        assert key < Nk // A.TILE * A.TILE or Nk < A.TILE
        assert float((ref[b, row, h * hd:(h + 1) * hd] - v[b, key, h * hd:(h + 1) * hd].double()).abs().max()) < 1e-12
    if "first_tile_max" in names:
        b, h, row = _row("first_tile_max", Bn, H)
        s = A.scores64(q, k, H, b, h, row, scale)
        assert int(s.argmax()) < A.TILE and int(s.argmax()) == A.first_key(Nk)
        assert A.margin(s, A.first_key(Nk)) > 5.0
    if "creeping_max" in names:
        b, h, row = _row("creeping_max", Bn, H)
        mx = A.tile_maxima(A.scores64(q, k, H, b, h, row, scale))
        steps = [(b_ - a_) * LOG2E for a_, b_ in zip(mx, mx[1:])]
        assert len(mx) == math.ceil(Nk / A.TILE)
        assert all(0.0 < d < 6.0 for d in steps), steps
        assert all(abs(d - A.CREEP_STEP * LOG2E) < 0.1 for d in steps), steps
    if "uniform_row" in names:
        b, _, row = _row("uniform_row", Bn, H)
        assert float((ref[b, row] - v[b].double().mean(0)).abs().max()) < 1e-12
    if "all_negative" in names:
        b, h, row = _row("all_negative", Bn, H)
        s = A.scores64(q, k, H, b, h, row, scale)
        assert -60.0 <= float(s.min()) and float(s.max()) <= -20.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_every_builder_delivers_its_property(dtype, hd):
    for name in ("late_outlier", "creeping_max", "first_tile_max", "uniform_row", "all_negative"):
        for Nk in (ONLINE_NK, 77):
            q, k, v = getattr(A, name)(dtype, hd, B, H, NQ, Nk, 7)
            assert q.dtype == dtype and q.shape == (B, NQ, H * hd) and k.shape == v.shape == (B, Nk, H * hd)
            _check_rows([name], q, k, v, hd, hd ** -0.5, Nk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_the_combined_tensor_keeps_every_property(dtype, hd):
    """the online-softmax test's tensor, and the one-pass tests' (no creeping maximum) at every key count they run"""
    q, k, v = A.combined(dtype, hd, B, H, NQ, ONLINE_NK, 11)
    _check_rows(A.planted_rows(), q, k, v, hd, hd ** -0.5, ONLINE_NK)
    if hd == 64:                                                   # v_path 6 is judged on the converted queries
        _check_rows(A.planted_rows(), A.exp2_q(q), k, v, hd, A.LN2, ONLINE_NK)
        for Nk in ONE_PASS_NK:
            q, k, v = A.combined(dtype, hd, B, H, NQ, Nk, 11 + Nk, creeping=False)
            _check_rows(A.planted_rows(False), q, k, v, hd, hd ** -0.5, Nk)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_creeping_maximum_passes_the_deferred_rescale_threshold_in_total(dtype):
    """every step stays under 2^6, the sum over 16 tiles exceeds it (what test_flash_attention_deferred_rescale_branches builds)"""
    for hd in HEAD_DIMS:
        q, k, v = A.creeping_max(dtype, hd, 1, 2, 32, 1024, 3)
        b, h, row = _row("creeping_max", 1, 2)
        mx = A.tile_maxima(A.scores64(q, k, 2, b, h, row, hd ** -0.5))
        steps = [(b_ - a_) * LOG2E for a_, b_ in zip(mx, mx[1:])]
        assert len(steps) == 15 and all(0.0 < d < 6.0 for d in steps) and sum(steps) > 6.0, steps


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_large_v_reaches_the_end_of_fp16_and_its_reference_stays_finite(hd):
    for Nk in (33, 65, 97, 129):
        q, k, v = A.large_v(torch.float16, hd, 1, 2, 64, Nk, 5)
        assert float(v.float().max()) == A.V_LARGE and float(v.float().min()) == -A.V_LARGE
        ref = A.attention_ref64(q, k, v, 2, hd ** -0.5)
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) <= A.V_LARGE
        b, h, row = _row("late_outlier", 1, 2)
        assert float((ref[b, row, :hd] - v[b, A.outlier_key(Nk), :hd].double()).abs().max()) < 1e-6
        b, _, row = _row("uniform_row", 1, 2)
        assert float((ref[b, row] - v[b].double().mean(0)).abs().max()) < 1e-9
    with pytest.raises(AssertionError):
        A.large_v(torch.bfloat16, hd, 1, 2, 64, 65, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_builders_hold_the_contiguous_values(dtype):
    for hd in HEAD_DIMS:
        for Nq, Nk in ((64, 64), (50, 77)):
            plain = A.gaussian(dtype, hd, 2, 2, Nq, Nk, 9)
            fused = A.fused_columns(dtype, hd, 2, 2, Nq, Nk, 9)
            assert all(torch.equal(a, b_) for a, b_ in zip(plain, fused))
            inner = 2 * hd
            assert fused[1].stride(1) == fused[2].stride(1) == (3 if Nq == Nk else 2) * inner and not fused[1].is_contiguous()
            assert fused[0].stride(1) == (3 * inner if Nq == Nk else inner)
            assert all(t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 for t in fused)
        second = A.every_second_batch(dtype, hd, 2, 2, 50, 77, 9)
        assert all(t.shape[0] == 2 and t.stride(0) == 2 * t.shape[1] * t.shape[2] for t in second)
        assert bool(torch.isfinite(A.attention_ref64(*second, 2, hd ** -0.5)).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [40, 64])
def test_poisoned_and_neighbour_views_hold_the_same_values_and_the_stated_layout(dtype, hd):
    Bn, Hn, Nk, front, gap = 2, 3, 77, 64, 3 * 64
    q, k, v = A.gaussian(dtype, hd, Bn, Hn, 32, Nk, 4)
    ref = A.attention_ref64(q, k, v, Hn, hd ** -0.5)
    HD = Hn * hd
    kp, vp = A.poisoned(k, v, front, gap)
    for t, src in ((kp, k), (vp, v)):
        assert torch.equal(t, src) and t.stride() == ((Nk + gap) * HD, HD, 1) and t.stride(0) > Nk * t.stride(1)
        assert t.storage_offset() == front * HD and t.data_ptr() % 16 == 0
        pool = torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
        assert pool.numel() == front * HD + Bn * (Nk + gap) * HD               # poison in front, behind EVERY entry, the last too
        mask = torch.ones_like(pool, dtype=torch.bool)
        for b in range(Bn):
            a = front * HD + b * (Nk + gap) * HD
            mask[a:a + Nk * HD] = False
        bad = pool[mask]
        assert int(mask.sum()) == (front + Bn * gap) * HD
        assert bool(torch.isinf(bad[0::2]).all()) or bool(torch.isinf(bad[1::2]).all())
        assert not bool(torch.isfinite(bad).any()) and bool(torch.isnan(bad).any())
        assert not bool(torch.isfinite(pool[:front * HD]).any()) and not bool(torch.isfinite(pool[-gap * HD:]).any())
    assert torch.equal(A.attention_ref64(q, kp, vp, Hn, hd ** -0.5), ref)
    assert torch.equal(A.attention_ref64(q, kp.contiguous(), vp.contiguous(), Hn, hd ** -0.5), ref)
    for n_front, n_behind in ((0, 4), (77, 0), (3, 5)):
        kn, vn = A.neighbours(k, v, n_front, n_behind, 100.0)
        for t, src in ((kn, k), (vn, v)):
            assert torch.equal(t, src) and t.stride() == ((n_front + Nk + n_behind) * HD, HD, 1) and t.data_ptr() % 16 == 0
            big = torch.as_strided(t, (Bn, n_front + Nk + n_behind, HD), t.stride(), 0)
            rest = torch.cat([big[:, :n_front], big[:, n_front + Nk:]], dim=1)
            assert bool((rest.float().abs() == 100.0).all()) and bool((rest[..., 0] > 0).all()) and bool((rest[..., 1] < 0).all())
        assert torch.equal(A.attention_ref64(q, kn, vn, Hn, hd ** -0.5), ref)
        assert torch.equal(A.attention_ref64(q, kn.contiguous(), vn.contiguous(), Hn, hd ** -0.5), ref)


def test_ip_reference_is_two_softmaxes():
    q, k, v = A.gaussian(torch.float16, 64, 2, 2, 20, 81, 1)
    two = A.attention_ref64(q, k[:, :77], v[:, :77], 2, 0.125) + 0.6 * A.attention_ref64(q, k[:, 77:], v[:, 77:], 2, 0.125)
    assert torch.equal(A.ip_ref64(q, k, v, 2, 77, 0.6), two)
    one = A.attention_ref64(q, k, v, 2, 0.125)
    assert float((two - one).abs().max()) > 1e-2                    # not one softmax over all 81 keys


def test_targets_name_every_instantiation():
    """one entry per row of (kernel family) x (instantiation reachable from ops), spelled out: a kernel added to
    attention_kernels.hip without a target -- so without the adversarial cases -- fails here when its name is added to this set."""
    from elasticdiffusion_official_amd import ops
    want = {"fwd/0", "fwd/1", "fwd/2", "fwd/3",
            "pipe/4", "pipe/5", "pipe/6", "pipe/7", "pipe/9", "pipe/10",
            "smallkv/2", "smallkv/3", "smallkv/5",
            "ip/2", "ip/3", "ip/5",
            "gen/40", "gen/80", "gen/160"}
    assert {t.name for t in A.TARGETS} == want and len(A.TARGETS) == len(want)
    assert {t.family for t in A.TARGETS} == {"k_flash_attn_fwd", "k_flash_attn_pipe", "k_flash_attn_smallkv", "k_flash_attn_ip",
                                             "k_flash_attn_gen"}
    # every v_path the entry point takes (0 .. 10) has a target, 8 once per key class
    assert sorted(t.v_path for t in A.TARGETS if t.v_path is not None) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 9, 10]
    assert sorted({t.head_dim for t in A.TARGETS}) == sorted(ops.FLASH_HEAD_DIMS)
    assert {t.name for t in A.ONLINE} == {n for n in want if n.split("/")[0] in ("fwd", "pipe", "gen")}
    for kind, top in (("smallkv", ops.SMALLKV_MAX_KEYS), ("ip", ops.IP_MAX_TEXT_KEYS)):
        # the three key classes tile 1 .. 160 without a hole, as the entry points' Nk <= 64 / <= 96 / else do
        names = [A.one_pass_target(kind, n).name for n in range(1, top + 1)]
        assert names == [f"{kind}/2"] * 64 + [f"{kind}/3"] * 32 + [f"{kind}/5"] * 64
        assert not any(t.takes(top + 1) for t in A.ONE_PASS if t.name.startswith(kind))
    assert [A.BY_NAME[f"pipe/{p}"].nk_min for p in (4, 5, 6, 7, 9, 10)] == [1, 1, 128, 64, 64, 64]
    assert {t.name: t.ragged_nk for t in A.TARGETS} == {
        "fwd/0": 65, "fwd/1": 65, "fwd/2": 65, "fwd/3": 65, "pipe/4": 65, "pipe/5": 65, "pipe/6": 129, "pipe/7": 65, "pipe/9": 65,
        "pipe/10": 65, "smallkv/2": 33, "smallkv/3": 65, "smallkv/5": 97, "ip/2": 33, "ip/3": 65, "ip/5": 97, "gen/40": 65,
        "gen/80": 65, "gen/160": 65}
    assert [t.name for t in A.TARGETS if t.exp2] == ["pipe/6"] and A.BY_NAME["pipe/6"].scale == A.LN2
    assert A.BY_NAME["gen/40"].scale == 40 ** -0.5


def test_flash_variant_leaves_the_pipelined_kernels_when_offsets_do_not_fit_32_bits():
    """K / V with a token stride of 4.2 M elements (meta tensors: no memory): (Nk + 128) * stride * 2 >= 2^31 from Nk = 128 on, so
    the default dispatch must fall back to a k_flash_attn_fwd variant, whose load_row16 addresses with 64-bit offsets; the small-KV
    kernel (64-bit offsets too) keeps the short prompts."""
    from elasticdiffusion_official_amd import ops
    stride = 4_200_000

    def kv(Bn, Nk, inner=128):
        return torch.empty_strided((Bn, Nk, inner), (Nk * stride, stride, 1), dtype=torch.float16, device="meta")
    for Nk in (128, 130, 200, 1024):
        t = kv(1, Nk)
        assert not ops._pipe_fits(Nk, stride) and ops._pipe_fits(Nk, 128)
        assert ops._flash_variant(1, 2, 256, Nk, t, t) == 0                      # not enough work for the 64-row variant
        dense = torch.empty((1, Nk, 128), dtype=torch.float16, device="meta")
        assert ops._flash_variant(1, 2, 256, Nk) == ops._flash_variant(1, 2, 256, Nk, dense, dense) == ops.FLASH_DEFAULT_PIPE
    big = kv(20, 1024, 640)
    assert ops._flash_variant(20, 10, 4096, 1024, big, big) == 2                 # the fallback keeps its own 64-row rule
    assert ops._flash_variant(20, 10, 4096, 1024, big, torch.empty((20, 1024, 640), device="meta")) == 2   # one wide operand is enough
    for Nk in (1, 77, 96):
        t = kv(1, Nk)
        assert ops._flash_variant(1, 2, 256, Nk, t, t) == 8
    for Nk in (97, 127):                                                          # neither small-KV by default nor pipelined: as before
        t = kv(1, Nk)
        assert ops._flash_variant(1, 2, 256, Nk, t, t) == 0
    with pytest.raises(RuntimeError):                                             # exponent-domain q has no fallback kernel
        ops._flash_variant(1, 2, 256, 130, kv(1, 130), kv(1, 130), prescaled=True)
