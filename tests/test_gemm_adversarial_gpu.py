"""-m gpu: every instantiation of the MFMA main loop that launch() and ed_geglu_gemm can pick (tests/gemm_cases.py: TARGETS) on the
adversarial operands of tests/gemm_cases.py -- activation scales from 2^-7 to 180 (bf16: 2^+-100), addends that cancel the accumulator,
outputs on both sides of 65504, subnormal operands, gates in GEGLU's tails, Inf / NaN next to every border, seam and ragged row, coded
operands whose result is known exactly, and operands carved out of one guarded allocation -- against the float64 reference and the bar
of that module, whose CPU test (tests/test_gemm_cases.py) proves the inputs have the properties claimed and the bar rests on fp32
stand-ins.  Every launch runs twice more and must give equal bits.  Each case prints one line: the worst |err| / bar of the kernel and,
where there is one, of the library call it replaces."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [t.name for t in G.TARGETS]
F16 = torch.float16


def _some(pred):
    ts = [t for t in G.TARGETS if pred(t)]
    return pytest.mark.parametrize("t", ts, ids=[t.name for t in ts])


@pytest.fixture(autouse=True)
def any_grid(monkeypatch):
    """the model keeps the library call on grids too small to fill the chip; the tests want every shape"""
    from elasticdiffusion_official_amd import ops
    monkeypatch.setattr(ops, "GEMM_MIN_BLOCKS", 1)
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _launch(t, c, ops, monkeypatch, out=None):
    """three launches with equal bits (no atomics, no split K: a difference between launches would be an LDS race) -> the output on the CPU"""
    monkeypatch.setenv("ED_GEMM_ROWS", t.rows_env)
    d = c if out is not None else c.to(DEV)
    got = t.run(ops, d, out)
    assert tuple(got.shape) == c.out_shape and got.dtype == c.out_dtype
    first = _bits(got).clone()
    for _ in range(2):
        assert torch.equal(_bits(t.run(ops, d, out)), first), f"{t.name}: two launches differ"
    return got.cpu()


def _library(c):
    """the library call the kernel replaces, in the operands' type (f32out: the fp32 convolution of the upcast operands), on the GPU"""
    d = c.to(DEV)
    dt = torch.float32 if c.op in G.OUT32 else c.dtype
    if c.op not in G.CONVS:
        y = F.linear(d.x, d.w, d.bias)
        if c.op == "geglu":
            I = c.shape[2]
            return (y[:, :I] * F.gelu(y[:, I:])).cpu()
        return (y if d.residual is None else y + d.residual).cpu()
    x, w = d.x.to(dt).permute(0, 3, 1, 2), d.w.to(dt).permute(0, 3, 1, 2)
    if c.op == "up2x":
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if c.op in ("conv", "up2x", "f32out"):
        y = F.conv2d(x, w, None, padding=1)
    elif c.op == "s2":
        y = F.conv2d(x, w, None, stride=2, padding=1)
    else:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=2)
    y = y.permute(0, 2, 3, 1) * c.out_scale
    if d.bias is not None:
        y = y + d.bias
    if d.sample_bias is not None:
        y = y + d.sample_bias[:, None, None, :]
    if d.residual is not None:
        y = y + d.residual
    return y.to(dt).cpu()


def _ratio(c, y):
    """worst |err| / bar of ``y`` (never raises: the library is measured, not judged)"""
    ref, b = G.bar(c)
    e = (y.double().reshape(ref.shape) - ref).abs() / b.clamp_min(1e-300)
    return float(e[torch.isfinite(ref)].nan_to_num(float("inf")).max())


def _rel(y, ref):
    return float((y.double().reshape(ref.shape) - ref).norm() / ref.norm())


def _hold(t, c, got, what, library=True, **kw):
    """the bar, element for element; fp32 outputs also as tests/test_vae_split.py judges them: relative L2 no worse than
    max(2 x the library's fp32 convolution, 6e-7)"""
    worst = G.judge(c, got, what=f"{what} {t.name} {c.shape}", **kw)
    lib = _library(c) if library else None
    if c.op in G.OUT32 and library and not kw:
        ref = G.ref64(c)
        e, e_lib = _rel(got, ref), _rel(lib, ref)
        print(f"    {t.name} {c.shape}: relative L2 {e:.2e} (library fp32 {e_lib:.2e})")
        assert e <= max(2.0 * e_lib, 6e-7), (what, t.name, c.shape, e, e_lib)
    return worst, (_ratio(c, lib) if library else float("nan"))


def _line(what, t, worst, lib, extra=""):
    print(f"\n{what} {t.name}: worst |err| / bar {worst:.3f} (library {lib:.3f}){extra}")


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_scaled_operands(t, any_grid, monkeypatch):
    """small outputs are held to a bar that scales with them: uniform data at 2^-7, 1 and 180 (bf16 also 2^100 and 2^-100)"""
    worst = lib = 0.0
    for combo in t.combos:
        for s in G.SCALES[t.dtype]:
            c = G.scaled(t, s, combo=combo)
            a, b = _hold(t, c, _launch(t, c, any_grid, monkeypatch), f"scaled {s:g}")
            worst, lib = max(worst, a), max(lib, b)
    _line("scaled", t, worst, lib)


@_some(lambda t: t.sweep)
def test_the_shapes_the_kernel_can_go_wrong_at(t, any_grid, monkeypatch):
    """one axis at a time around the base shape: M 1 ... 300, 1, 2, 3 and 10 K tiles, ragged and half column blocks; images of 1 x 1,
    1 x W, H x 1 and 2 x 2, Cin to 2560 (40 K tiles per tap)"""
    worst = lib = 0.0
    combo = max(t.combos, key=sum)
    for shape in G.sweep_shapes(t):
        c = G.scaled(t, 1.0, shape, combo)
        a, b = _hold(t, c, _launch(t, c, any_grid, monkeypatch), "sweep")
        worst, lib = max(worst, a), max(lib, b)
    _line(f"sweep of {len(G.sweep_shapes(t))} shapes", t, worst, lib)


@_some(lambda t: t.add)
def test_addends_that_cancel_the_accumulator(t, any_grid, monkeypatch):
    """round16(acc + bias + sample_bias + residual) with fp32 sums and ONE rounding: a kernel that rounded in between fails here on
    more than 80 % of the elements (tests/test_gemm_cases.py)"""
    worst = lib = 0.0
    for combo in t.combos:
        c = G.cancelling(t, combo)
        a, b = _hold(t, c, _launch(t, c, any_grid, monkeypatch), "cancelling")
        worst, lib = max(worst, a), max(lib, b)
    _line("cancelling", t, worst, lib)


@_some(lambda t: t.dtype == F16 and t.op not in G.OUT32)
def test_outputs_on_both_sides_of_65504(t, any_grid, monkeypatch):
    """+-inf exactly where one rounding of the float64 result gives it, finite and within the bar elsewhere"""
    for combo in (k for k in t.combos if k[0]):
        c = G.near_max(t, combo)
        got = _launch(t, c, any_grid, monkeypatch)
        inf, skip = c.note["inf"], c.note["skip"]
        worst, _ = _hold(t, c, got, "near_max", library=False, expect_finite=~inf, skip=skip)
        sel = inf & ~skip
        assert torch.equal(got.double().reshape(inf.shape)[sel], G.round_to(G.ref64(c), F16)[sel])       # the sign of each infinity
        _line("near_max", t, worst, float("nan"), f" {c.note['over']} overflow, {c.note['under']} stay finite, {int(skip.sum())} undecidable left out")


@_some(lambda t: t.dtype == F16)
def test_subnormal_operands_are_not_flushed(t, any_grid, monkeypatch):
    worst = lib = 0.0
    for combo in (k for k in t.combos if k[0] or t.op != "geglu"):
        for which in "xw":
            c = G.subnormal(t, combo, which)
            a, b = _hold(t, c, _launch(t, c, any_grid, monkeypatch), f"subnormal {which}")
            worst, lib = max(worst, a), max(lib, b)
    _line("subnormal", t, worst, lib)


@_some(lambda t: t.op == "geglu")
def test_geglu_gate_tails(t, any_grid, monkeypatch):
    """geglu_one's erfc fit on planted gates over [-12, 12] with values to 1000; the unfused pair (F.linear, then ops.geglu) beside it"""
    c = G.gate_tails(t)
    got = _launch(t, c, any_grid, monkeypatch)
    worst, lib = _hold(t, c, got, "gate_tails")
    d = c.to(DEV)
    pair = _ratio(c, any_grid.geglu(F.linear(d.x, d.w), c.shape[2]).cpu())
    _line("gate_tails", t, worst, lib, f", unfused F.linear + ops.geglu {pair:.3f}")


@pytest.mark.parametrize("which", ["x", "w"])
@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_inf_and_nan_spoil_their_own_field_and_nothing_else(t, which, any_grid, monkeypatch):
    """zero padding, sample seams and the rows past M are zeros, not masked loads: isfinite(got) equals isfinite of the fp32 CPU
    reference element for element, and every finite element is within the bar"""
    shapes = G.nonfinite_shapes(t)
    worst = 0.0
    for shape in shapes:
        for combo in t.combos if shape == t.shape else t.combos[:1]:
            c = G.nonfinite(t, combo, which, shape)
            a, _ = _hold(t, c, _launch(t, c, any_grid, monkeypatch), f"nonfinite {which}", library=False, expect_finite=c.note["finite"])
            worst = max(worst, a)
    _line(f"nonfinite {which} ({len(shapes)} shapes)", t, worst, float("nan"))


@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_coded_operands_come_back_exactly(t, any_grid, monkeypatch):
    """GEMM: out[m, n] = a_m + b_n; convolution: the identity on each of the 9 taps returns the shifted, zero-padded image.  A
    permuted, skipped or repeated tile, row, column group or tap is a mismatch at a known index."""
    combo = max(t.combos, key=sum)
    shapes = [t.shape] + ([(2400, 64, 384 if t.op == "geglu" else 264)] if t.op not in G.CONVS else [])
    for shape in shapes:
        cases = [G.coded_gemm(t, combo, shape)] if t.op not in G.CONVS else [G.coded_conv(t, combo, tap, shape) for tap in range(9)]
        for tap, c in enumerate(cases):
            got, want = _launch(t, c, any_grid, monkeypatch), c.note["want"]
            if not torch.equal(got, want):
                i = tuple((got != want).nonzero()[0].tolist())
                raise AssertionError(f"coded {t.name} {c.shape} tap {tap}: {int((got != want).sum())} elements differ, first {i}: got {float(got[i])} want {float(want[i])}")
    print(f"\ncoded {t.name}: exact on {shapes}")


@pytest.mark.parametrize("t", G.TARGETS, ids=IDS)
def test_guarded_operands_and_output(t, any_grid, monkeypatch):
    """operands and output carved out of one allocation, NaN around the operands, NaN in the output, sentinels around it: every
    output element is written (and from no guard NaN), nothing outside [M, N] is"""
    combo = max(t.combos, key=sum)
    worst = 0.0
    for shape in G.guard_shapes(t):
        c = G.scaled(t, 1.0, shape, combo)
        a = G.guarded(c, DEV)
        got = _launch(t, a.case, any_grid, monkeypatch, out=a.out)
        torch.cuda.synchronize()
        G.guard_check(a, c)
        worst = max(worst, G.judge(c, got, what=f"guarded {t.name} {shape}"))
    _line(f"guarded ({len(G.guard_shapes(t))} shapes)", t, worst, float("nan"))
