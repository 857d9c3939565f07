"""CPU: the adversarial GEMM / convolution inputs of tests/gemm_cases.py have the properties the GPU tests
(tests/test_gemm_adversarial_gpu.py) rely on, the bar rests on fp32 stand-ins and not on the kernel, every target's shape selects the
instantiation its name says, and every class of fault the cases are there for is caught when a CPU stand-in commits it.  Run with -s to
see the measured figures."""
import itertools

import numpy as np
import pytest
import torch

from tests import gemm_cases as G

F16 = torch.float16
IDS = [t.name for t in G.TARGETS]


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _target(name):
    return next(t for t in G.TARGETS if t.name == name)


# ---- target selection -------------------------------------------------------------------------------------------------------------
def test_the_long_k_threshold_is_the_kernels():
    assert G.TWO_MIN_TILES == G.source_two_min_tiles() == 20


@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_each_targets_shape_selects_what_its_name_says(t):
    ops = _ops()
    for combo in t.combos:
        kernel, add, loop = t.selects(ops, combo=combo)
        assert kernel == ("k_geglu_persist" if t.op == "geglu" else "k_gemm_8phase")
        assert add == t.add and loop == t.loop, (t.name, combo, add, loop)
    K = G.k_len(t.op, t.shape)
    assert K // 64 >= 2 and (t.loop != "two" or K // 64 >= 20) and (t.loop not in ("8phase", "half", "rows") or t.op not in G.CONVS or K // 64 < 20)
    M = G.make(t).M
    assert M % 128 != 0                                                           # a ragged last tile at both tile heights
    if t.op in G.CONVS:
        assert M // t.shape[0] < (128 if t.op == "conv" else 256) and t.shape[0] > 1     # a sample seam inside the first tile (256 rows but for conv)


def test_the_targets_are_every_instantiation_the_launcher_can_pick():
    """launch(): k_gemm_8phase<T, EPI 1, CONV, ADD, OUT32, TWO, ROWS> -- ROWS for the plain projection and the stride-1 convolution only
    (and then never TWO), ADD not for the up / down-samplers, OUT32 in fp16 only, TWO for convolutions only; and k_geglu_persist<T>."""
    want = set()
    for d in ("f16", "bf16"):
        want.add(("geglu", d, False, "persist"))
        for add in (False, True):
            want |= {("linear", d, add, "8phase"), ("linear", d, add, "rows")}
            want |= {("conv", d, add, loop) for loop in ("8phase", "two", "rows")}
        want |= {(op, d, False, loop) for op in ("up2x", "s2") for loop in ("8phase", "two")}
    want |= {("f32out", "f16", add, loop) for add in (False, True) for loop in ("8phase", "two")}
    want |= {("f32out_s2", "f16", False, loop) for loop in ("8phase", "two")}
    have = {(t.op, G.SHORT[t.dtype], t.add, t.loop) for t in G.TARGETS}
    assert want <= have and {h for h in have - want} == {(op, d, False, "half") for op in ("linear", "conv") for d in ("f16", "bf16")}
    assert len(IDS) == len(set(IDS))


def test_the_sweep_holds_the_shapes_the_kernel_can_go_wrong_at():
    ops = _ops()
    for t in G.TARGETS:
        if not t.sweep:
            continue
        shapes = G.sweep_shapes(t)
        if t.op in G.CONVS:
            assert {s[:3] for s in shapes} >= set(G.CONV_GEOM) and {s[3] for s in shapes} == set(G.CONV_CIN) and {s[4] for s in shapes} == set(G.CONV_N)
            assert all(s[:3] == (5, 1, 1) and s[4] == 8 for s in shapes if s[3] >= 960)
            loops = {t.selects(ops, s)[2] for s in shapes}
            assert loops >= ({"rows"} if t.loop == "rows" else {"8phase", "two", "half"}), (t.name, loops)
            assert {G.k_len(t.op, s) // 64 % 2 for s in shapes} == {0, 1}          # odd and even K-tile counts: both exits of the unrolled loops
        else:
            assert {s[0] for s in shapes} == set(G.GEMM_M) and {s[1] for s in shapes} == set(G.GEMM_K)
            assert {s[1] // 64 for s in shapes} >= {1, 2, 3}
            if t.op == "linear":
                assert {s[2] for s in shapes} == set(G.GEMM_N)
    assert all(t.sweep == (t.loop in ("persist", "8phase", "rows")) for t in G.TARGETS)      # one per instantiation family and tile height


# ---- the builders at the shapes the GPU tests use -----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_builders_hold_their_properties_at_the_gpu_shapes(t):
    shares, rates = [], []
    for combo in t.combos:
        for s in G.SCALES[t.dtype]:
            G.scaled(t, s, combo=combo)
        if combo[1] or combo[2]:
            c = G.cancelling(t, combo)
            rates.append(G.fail_share(c, G.double_rounded(c)))
            assert rates[-1] > 0.8, (t.name, combo, rates[-1])          # the case can still tell a double rounding
        if t.dtype == F16 and t.op not in G.OUT32 and combo[0]:
            c = G.near_max(t, combo)
            shares.append(c.note["share"])
            assert c.note["share"] <= 0.01 and min(c.note["over"], c.note["under"]) >= 32
        if t.dtype == F16 and (t.op != "geglu" or combo[0]):
            for which in "xw":
                c = G.subnormal(t, combo, which)
                assert G.fail_share(c, G.flushed(c)) > 0.9                # a flushed operand is refused almost everywhere
        for which in "xw":
            for shape in G.nonfinite_shapes(t) if combo == t.combos[0] else [t.shape]:
                c = G.nonfinite(t, combo, which, shape)
                G.judge(c, G.ref64(c, torch.float32).to(c.out_dtype), c.note["finite"])      # the fp32 reference passes its own case
    full = max(t.combos, key=sum)
    if t.op == "geglu":
        G.gate_tails(t)
    if t.op not in G.CONVS:
        for shape in (t.shape, (2400, 64, 384 if t.op == "geglu" else 264)):
            G.coded_gemm(t, full, shape)
    else:
        for tap in range(9):
            G.coded_conv(t, full, tap)
    if t.sweep:
        for shape in G.sweep_shapes(t):
            G.scaled(t, 1.0, shape, full)
    for shape in (s for s in G.guard_shapes(t) if s[0] < 20000):       # (the 261-tile GEGLU grid is built on the GPU machine only: its builder asserts there)
        c = G.scaled(t, 1.0, shape, full)
        a = G.guarded(c, "cpu")
        assert all(hi - lo >= G.GUARD_BYTES for _, lo, hi, _ in a.out_bands) and bool(torch.isnan(a.out).all())
        G.guard_check(a, c)
    pct = lambda v: f"{v:.2%}" if v is not None else "n/a"
    print(f"\n{t.name}: double-rounding detection {pct(min(rates, default=None))} (> 80 %), near_max exclusion share "
          f"{pct(max(shares, default=None))} (<= 1 %)")


# ---- the bar rests on fp32 stand-ins --------------------------------------------------------------------------------------------------
KAPPA_CASES = [("linear/f16/add/8phase", None), ("linear/f16/plain/8phase", (300, 640, 136)), ("linear/bf16/plain/8phase", (129, 5120, 72)),
               ("geglu/f16/plain/persist", None), ("conv/f16/add/8phase", None), ("conv/bf16/add/two", None), ("conv/f16/plain/8phase", (5, 1, 1, 960, 8)),
               ("conv/f16/plain/8phase", (5, 1, 1, 2560, 8)), ("up2x/f16/plain/two", None), ("s2/bf16/plain/8phase", None),
               ("f32out/f16/add/two", None), ("f32out_s2/f16/plain/8phase", None)]


@pytest.mark.parametrize("name,shape", KAPPA_CASES, ids=[f"{n}-{s}" for n, s in KAPPA_CASES])
def test_fp32_stand_ins_stay_below_half_of_kappa(name, shape):
    """torch's blocked fp32 matmul / conv2d and a strictly sequential fp32 sum against float64, in units of 2^-24 absprod64, on the
    builders' data: at most 4 (KAPPA = 8 leaves the matrix instruction's own order a factor 2)."""
    t = _target(name)
    cases = [G.scaled(t, 1.0, shape, max(t.combos, key=sum)), G.scaled(t, 2.0 ** -7, shape)]
    if t.add and shape is None:
        cases.append(G.cancelling(t, t.combos[-1]))
    worst = {"blocked": 0.0, "sequential": 0.0}
    for c in cases:        # the operation up to its one rounding: fp32 accumulator, fp32 sums of the addends (GEGLU: the two pre-activations)
        want, unit = G.contraction(c) + G.addends(c), G.EPS32 * G.absprod64(c)
        for label, acc in (("blocked", G.contraction(c, torch.float32)), ("sequential", G.sequential_fp32(c))):
            got = acc + G.addends(c, torch.float32)
            err = (got.double() - want).abs()
            if c.out_dtype == torch.float32:       # an fp32 output IS this fp32 value: its one rounding is the bar's u |ref64| term, not KAPPA's
                err = (err - G.U[torch.float32] * want.abs()).clamp_min(0)
            worst[label] = max(worst[label], float((err / unit.clamp_min(1e-300)).max()))
    print(f"\nkappa stand-ins {name} {shape or t.shape}: blocked fp32 {worst['blocked']:.2f}, sequential fp32 {worst['sequential']:.2f} (<= 4)")
    assert max(worst.values()) <= 4.0, worst


def test_the_gelu_fit_in_exact_fp32_is_within_its_figure():
    """geglu_one's 5-term erfc fit in fp32 with an exact division and exp2 against float64 over 2M gates in [-12, 12]: at most
    3.4e-7 (GELU_FIT = 5e-7 is that with a factor 1.5 for the two 1-ulp hardware approximations)."""
    g = np.linspace(-12.0, 12.0, 2_000_001).astype(np.float32)
    g = np.concatenate([g, np.array(G.GATES, dtype=np.float32)])
    want = G.gelu64(torch.from_numpy(g).double()).numpy()
    err = float(np.abs(G.gelu_fit_fp32(g).astype(np.float64) - want).max())
    print(f"\ngelu fit in exact fp32 vs float64 over [-12, 12]: {err:.3e} (<= {G.GELU_FIT_EXACT:.1e})")
    assert err <= G.GELU_FIT_EXACT < G.GELU_FIT
    assert float(np.abs(np.gradient(want[:-len(G.GATES)], g[:-len(G.GATES)].astype(np.float64))).max()) <= G.GELU_SLOPE


# ---- every class of fault is caught -----------------------------------------------------------------------------------------------------
CONV = "conv/f16/plain/8phase"


def test_the_stand_in_itself_passes_every_case():
    t = _target("conv/f16/add/8phase")
    for c in (G.scaled(t, 1.0, combo=t.combos[-1]), G.cancelling(t, t.combos[-1])):
        G.judge(c, G.conv_standin(c))
    for which in "xw":
        c = G.nonfinite(t, t.combos[-1], which)
        G.judge(c, G.conv_standin(c), c.note["finite"])
    for tap in range(9):
        c = G.coded_conv(t, t.combos[-1], tap)
        assert torch.equal(G.conv_standin(c), c.note["want"])


@pytest.mark.parametrize("geom", [(3, 5, 7), (3, 1, 9), (3, 9, 1), (2, 12, 20), (4, 2, 2), (5, 1, 1)])
def test_non_zero_padding_is_caught(geom):
    """a border tap that loads the clamped neighbour and multiplies by a mask: the same numbers on finite data, NaN next to an Inf"""
    t = _target(CONV)
    shape = geom + (64, 72)
    fin = G.scaled(t, 1.0, shape)
    assert torch.equal(G.conv_standin(fin, "mask_multiply"), G.conv_standin(fin))           # invisible on finite data
    c = G.nonfinite(t, t.combos[0], "x", shape)
    with pytest.raises(AssertionError, match="isfinite"):
        G.judge(c, G.conv_standin(c, "mask_multiply"), c.note["finite"])


@pytest.mark.parametrize("geom", [(3, 5, 7), (3, 1, 9), (2, 12, 20), (4, 2, 2), (5, 1, 1)])
def test_a_cross_sample_read_is_caught(geom):
    t = _target(CONV)
    shape = geom + (64, 72)
    c = G.scaled(t, 1.0, shape)
    with pytest.raises(AssertionError, match="outside the bar"):
        G.judge(c, G.conv_standin(c, "cross_sample"))
    c = G.nonfinite(t, t.combos[0], "x", shape)
    with pytest.raises(AssertionError, match="isfinite"):
        G.judge(c, G.conv_standin(c, "cross_sample"), c.note["finite"])


def test_a_wrong_tap_direction_is_caught():
    t = _target(CONV)
    c = G.scaled(t, 1.0)
    with pytest.raises(AssertionError, match="outside the bar"):
        G.judge(c, G.conv_standin(c, "wrong_tap"))
    for tap in range(9):
        c = G.coded_conv(t, t.combos[0], tap)
        assert torch.equal(G.conv_standin(c, "wrong_tap"), c.note["want"]) == (tap % 3 == 1)     # (the middle column has no direction)
    for op in ("up2x", "s2", "f32out_s2"):              # every variant's coded image tells its 9 taps apart
        tt = next(x for x in G.TARGETS if x.op == op)
        wants = [G.coded_conv(tt, tt.combos[0], tap).note["want"] for tap in range(9)]
        assert not any(torch.equal(a, b) for a, b in itertools.combinations(wants, 2))


def test_double_rounding_is_caught():
    for name in ("linear/f16/add/8phase", "linear/bf16/add/rows", "conv/f16/add/two", "conv/bf16/add/8phase", "f32out/f16/add/two"):
        t = _target(name)
        for combo in t.combos:
            c = G.cancelling(t, combo)
            with pytest.raises(AssertionError, match="outside the bar"):
                G.judge(c, G.double_rounded(c))
            G.judge(c, G.ref64(c, torch.float32).to(c.out_dtype))             # fp32 sums and one rounding pass


def test_a_flushed_subnormal_is_caught():
    for name in ("linear/f16/plain/8phase", "conv/f16/plain/two", "f32out/f16/plain/two", "geglu/f16/plain/persist"):
        t = _target(name)
        for which in "xw":
            c = G.subnormal(t, t.combos[0], which)
            with pytest.raises(AssertionError, match="outside the bar"):
                G.judge(c, G.flushed(c))
            G.judge(c, G.ref64(c, torch.float32).to(c.out_dtype))


def test_an_overflow_that_saturates_or_comes_early_is_caught():
    t = _target("linear/f16/add/8phase")
    c = G.near_max(t, t.combos[0])
    once = G.round_to(G.ref64(c), F16)
    G.judge(c, once, ~c.note["inf"], c.note["skip"])
    with pytest.raises(AssertionError, match="isfinite"):
        G.judge(c, once.clamp(-G.F16_MAX, G.F16_MAX), ~c.note["inf"], c.note["skip"])         # saturating conversion
    with pytest.raises(AssertionError, match="isfinite"):
        G.judge(c, G.round_to(G.ref64(c) * (1 + 2.0 ** -10), F16), ~c.note["inf"], c.note["skip"])


def test_a_skipped_or_permuted_tile_is_caught():
    """guarded: the output is pre-filled with NaN, so a tile nobody writes cannot pass on what an earlier launch left in the same
    block; coded: a permuted row block is a mismatch"""
    t = _target("linear/f16/plain/8phase")
    c = G.scaled(t, 1.0, (300, 192, 264))
    a = G.guarded(c, "cpu")
    a.out.copy_(G.ref64(c).to(c.out_dtype))
    G.judge(c, a.out)
    G.guard_check(a, c)
    a.out[128:256, 256:] = float("nan")                  # the second column block's tile of rows 128..255 is never written
    with pytest.raises(AssertionError, match="isfinite"):
        G.judge(c, a.out)
    k = G.coded_gemm(t, t.combos[0], (300, 192, 264))
    swapped = k.note["want"].clone()
    swapped[0:128], swapped[128:256] = k.note["want"][128:256], k.note["want"][0:128]
    assert not torch.equal(swapped, k.note["want"])


@pytest.mark.parametrize("where", ["row M", "one element before", "x", "bias band"])
def test_a_store_outside_the_output_is_caught(where):
    t = _target("conv/bf16/add/8phase")
    c = G.scaled(t, 1.0, combo=t.combos[-1])
    a = G.guarded(c, "cpu")
    a.out.copy_(G.ref64(c).to(c.out_dtype))
    G.guard_check(a, c)
    flat = a.buf.view(torch.bfloat16)
    first = (a.out.data_ptr() - a.buf.data_ptr()) // 2
    if where == "row M":                                  # an off-by-one row: the 16-byte store of row M
        flat[first + a.out.numel():first + a.out.numel() + 8] = 1.0
    elif where == "one element before":
        flat[first - 1] = 1.0
    elif where == "x":
        a.case.x[0, 0, 0, 0] = 5.0
    else:
        flat[(a.case.bias.data_ptr() - a.buf.data_ptr()) // 2 - 1] = 0.0
    with pytest.raises(AssertionError, match="band|operand"):
        G.guard_check(a, c)
