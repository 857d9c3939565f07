"""Adversarial operands for the MFMA GEMM / convolution kernels (csrc/gemm_kernels.hip), the float64 statement of the operations they
are judged against, the bar, and the list of kernel instantiations ``launch()`` and ``ed_geglu_gemm`` can pick.  No tests here and
nothing that needs a GPU: the builders make their data with a CPU generator (so the CPU test of the builders, tests/test_gemm_cases.py,
sees the very tensors the GPU tests run); ``Case.to(device)`` moves them.

Layouts (all dense, the kernel's own): GEMM x [M, K], w [N, K] (GEGLU: w [2 I, K], value rows then gate rows); convolution x
[B, Hi, Wi, Cin] (NHWC), w [N, 3, 3, Cin], bias [N], sample_bias [B, N], residual / out [B, H, W, N].  A convolution shape is
``(B, H, W, Cin, N)`` with H x W the size of the stride-1 image, of the SOURCE of ``up2x`` (output 2H x 2W) and of the OUTPUT of ``s2``
/ ``f32out_s2`` (input 2H x 2W): every variant then has a sample seam inside a tile at the same ``(B, H, W)``.

A builder asserts the property its docstring states, in float64 on the tensors it returns: data that lost its property (another seed,
another shape) stops the test that asked for it instead of quietly checking nothing.

The bar (``bar``):   |got - ref64| <= u |ref64| + KAPPA 2^-24 absprod64 + tiny
u = one rounding to the output type, tiny = fp16's subnormal spacing, and KAPPA 2^-24 absprod64 the fp32 accumulation: two fp32
stand-ins (torch's blocked fp32 matmul / conv2d and a strictly sequential fp32 sum) stay at or below 4 x 2^-24 absprod64 on these
builders' data (re-measured by the CPU test), KAPPA = 8 is that with a factor 2 for the matrix instruction's own order.  The bar rests
on the reference and never on the kernel.
"""
import math
import re
from dataclasses import dataclass, field, replace
from pathlib import Path

import torch
import torch.nn.functional as F

KAPPA = 8.0
EPS32 = 2.0 ** -24
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0, torch.float32: 0.0}
GELU_FIT = 5e-7                # |geglu_one's gelu - gelu64| per unit of |v|: 3.4e-7 for the fit in exact fp32 (CPU test) x 1.5 for v_rcp / v_exp
GELU_FIT_EXACT = 3.4e-7
GELU_SLOPE = 1.13              # max |gelu'|
TWO_MIN_TILES = 20             # csrc/gemm_kernels.hip: convolutions of at least this many K tiles run the long-K loop
CONVS = ("conv", "up2x", "s2", "f32out", "f32out_s2")
OUT32 = ("f32out", "f32out_s2")
F16_MAX, F16_INF_FROM = 65504.0, 65520.0
SHORT = {torch.float16: "f16", torch.bfloat16: "bf16"}
KERNEL_SOURCE = Path(__file__).resolve().parents[1] / "elasticdiffusion_official_amd" / "csrc" / "gemm_kernels.hip"


def source_two_min_tiles():
    """TWO_MIN_TILES as csrc/gemm_kernels.hip states it (ops has no mirror of it)"""
    return int(re.search(r"constexpr int TWO_MIN_TILES = (\d+);", KERNEL_SOURCE.read_text()).group(1))


# ---- a case: the operands of one launch -----------------------------------------------------------------------------------------
@dataclass
class Case:
    op: str                        # geglu | linear | conv | up2x | s2 | f32out | f32out_s2
    dtype: torch.dtype             # of x and w
    shape: tuple                   # (M, K, N) / (M, K, I) / (B, H, W, Cin, N)
    x: torch.Tensor
    w: torch.Tensor
    bias: torch.Tensor = None
    sample_bias: torch.Tensor = None
    residual: torch.Tensor = None
    out_scale: float = 1.0         # f32out only (a power of two)
    note: dict = field(default_factory=dict)

    @property
    def out_dtype(self):
        return torch.float32 if self.op in OUT32 else self.dtype

    @property
    def add_dtype(self):           # of bias / sample_bias / residual
        return self.out_dtype

    @property
    def out_shape(self):
        if self.op not in CONVS:
            return (self.shape[0], self.shape[2])
        B, H, W, _, N = self.shape
        u = 2 if self.op == "up2x" else 1
        return (B, u * H, u * W, N)

    @property
    def M(self):
        return math.prod(self.out_shape[:-1])

    def tensors(self):
        return {k: getattr(self, k) for k in ("x", "w", "bias", "sample_bias", "residual") if getattr(self, k) is not None}

    def to(self, device):
        return replace(self, **{k: v.to(device) for k, v in self.tensors().items()})


def x_shape(op, shape):
    if op not in CONVS:
        return (shape[0], shape[1])
    B, H, W, Cin, _ = shape
    u = 2 if op in ("s2", "f32out_s2") else 1
    return (B, u * H, u * W, Cin)


def w_shape(op, shape):
    if op == "geglu":
        return (2 * shape[2], shape[1])
    return (shape[2], shape[1]) if op == "linear" else (shape[4], 3, 3, shape[3])


def k_len(op, shape):
    return 9 * shape[3] if op in CONVS else shape[1]


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def contraction(c, dt=torch.float64, absolute=False):
    """the accumulator: x w^T ([M, N]; GEGLU [M, 2 I]) or the variant's convolution times out_scale ([B, H, W, N]), in ``dt`` on the
    values as given; ``absolute``: on |x| and |w|"""
    x, w = c.x.to(dt), c.w.to(dt)
    if absolute:
        x, w = x.abs(), w.abs()
    if c.op not in CONVS:
        return x @ w.t()
    xi, wi = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    if c.op == "up2x":
        xi = xi.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if c.op in ("conv", "up2x", "f32out"):
        y = F.conv2d(xi, wi, padding=1)
    elif c.op == "s2":
        y = F.conv2d(xi, wi, stride=2, padding=1)
    else:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wi, stride=2)
    return y.permute(0, 2, 3, 1) * (abs(c.out_scale) if absolute else c.out_scale)


def addends(c, dt=torch.float64, absolute=False):
    """bias + sample_bias + residual, broadcast to the accumulator's shape (0.0 when there is none)"""
    s = 0.0
    for t, view in ((c.bias, lambda t: t), (c.sample_bias, lambda t: t[:, None, None, :]), (c.residual, lambda t: t)):
        if t is not None:
            t = view(t.to(dt))
            s = s + (t.abs() if absolute else t)
    return s


def gelu64(g):
    return g * 0.5 * torch.special.erfc(-g / math.sqrt(2.0))


def ref64(c, dt=torch.float64):
    """the operation in float64 on the 16-bit values as given (``dt`` = float32: the fp32 CPU reference of the non-finite cases)"""
    y = contraction(c, dt) + addends(c, dt)
    if c.op == "geglu":
        I = c.shape[2]
        return y[:, :I] * (gelu64(y[:, I:]) if dt == torch.float64 else F.gelu(y[:, I:]))
    return y


def absprod64(c):
    """the same contraction on |x| and |w|, plus |bias|, |sample_bias| and |residual|"""
    return contraction(c, absolute=True) + addends(c, absolute=True)


def bar(c):
    """-> (ref64, bar), both of the output's shape.  GEGLU: the KAPPA terms of the two projections propagated through the product
    (|gelu'| <= 1.13) and |v| GELU_FIT for the erfc fit."""
    u, tiny = U[c.out_dtype], TINY[c.out_dtype]
    if c.op != "geglu":
        ref = ref64(c)
        return ref, u * ref.abs() + KAPPA * EPS32 * absprod64(c) + tiny
    I = c.shape[2]
    y, d = contraction(c) + addends(c), KAPPA * EPS32 * absprod64(c)
    v, g, dv, dg = y[:, :I], y[:, I:], d[:, :I], d[:, I:]
    ge = gelu64(g)
    ref = v * ge
    return ref, u * ref.abs() + ge.abs() * dv + (v.abs() + dv) * (GELU_SLOPE * dg + GELU_FIT) + tiny


def judge(c, got, expect_finite=None, skip=None, what=""):
    """Hold ``got`` to the bar.  ``expect_finite`` (bool, output's shape; default: everywhere): ``isfinite(got)`` must equal it element
    for element, and every element finite in both is within the bar of ref64.  ``skip``: elements left out altogether (near_max's
    undecidable ones).  -> worst |err| / bar.  Raises AssertionError naming the first offender."""
    ref, b = bar(c)
    got = got.detach().cpu().double().reshape(ref.shape)
    fin = torch.ones_like(ref, dtype=torch.bool) if expect_finite is None else expect_finite.reshape(ref.shape)
    keep = torch.ones_like(fin) if skip is None else ~skip.reshape(ref.shape)
    wrong = (torch.isfinite(got) != fin) & keep
    assert not bool(wrong.any()), (f"{what}: isfinite(got) differs from the expectation at {int(wrong.sum())} of {wrong.numel()} elements, "
                                   f"first {tuple(wrong.nonzero()[0].tolist())} got {float(got[wrong][0])}")
    sel = fin & keep
    err, bb = (got - ref).abs()[sel], b[sel]
    bad = ~(err <= bb)
    if bool(bad.any()):
        i = tuple(sel.nonzero()[bad.nonzero()[0, 0]].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bar, first {i}: got {float(got[i])!r} "
                             f"ref64 {float(ref[i])!r} bar {float(b[i]):.3e}")
    return float((err / bb.clamp_min(1e-300)).max()) if err.numel() else 0.0


def fail_share(c, got, expect_finite=None):
    """share of the elements ``judge`` would refuse (for the stand-ins that must be caught)"""
    ref, b = bar(c)
    got = got.detach().cpu().double().reshape(ref.shape)
    fin = torch.ones_like(ref, dtype=torch.bool) if expect_finite is None else expect_finite.reshape(ref.shape)
    bad = (torch.isfinite(got) != fin) | (fin & ~((got - ref).abs() <= b))
    return float(bad.double().mean())


def round_to(t, dtype):
    """one rounding (RNE) of a float64 / float32 tensor to ``dtype``, returned as float64"""
    return t.to(dtype).double()


# ---- the kernel instantiations launch() and ed_geglu_gemm can pick ------------------------------------------------------------------
B_, S_, R_ = (True, False, False), (False, True, False), (False, False, True)


def _combo(*parts):
    return tuple(any(p[i] for p in parts) for i in range(3))


NONE = (False, False, False)
COMBOS = {   # (bias, sample_bias, residual) as the model calls each entry point
    ("geglu", False): (B_, NONE), ("linear", False): (B_, NONE), ("linear", True): (_combo(B_, R_), R_),
    ("conv", False): (B_, NONE), ("conv", True): (_combo(B_, S_), _combo(B_, R_), _combo(B_, S_, R_)),
    ("up2x", False): (B_, NONE), ("s2", False): (B_, NONE),
    ("f32out", False): (B_, NONE), ("f32out", True): (_combo(B_, R_), R_), ("f32out_s2", False): (B_, NONE),
}


@dataclass(frozen=True)
class Target:
    op: str
    dtype: torch.dtype
    add: bool            # the ADD instantiation (a sample_bias or a residual)
    loop: str            # persist | 8phase | two | half | rows: the main loop the base shape runs
    shape: tuple         # the smallest shape that picks it with a ragged M, >= 2 K tiles and a sample seam inside the tile
    sweep: bool = False  # runs the one-axis-at-a-time shape sweep (one target per instantiation family; the loop follows the shape)

    @property
    def name(self):
        return f"{self.op}/{SHORT[self.dtype]}/{'add' if self.add else 'plain'}/{self.loop}"

    @property
    def combos(self):
        return COMBOS[(self.op, self.add)]

    @property
    def rows_env(self):
        """ED_GEMM_ROWS for this target: the kernels with a 128-row instantiation are pinned to one height, the others ignore it"""
        return "1" if self.loop == "rows" else "0"

    def selects(self, ops, shape=None, combo=None):
        """what launch() picks for ``shape``, read back through the ops mirrors: (kernel, ADD, loop)"""
        shape = self.shape if shape is None else shape
        combo = self.combos[0] if combo is None else combo
        if self.op == "geglu":
            assert ops.geglu_gemm_ok(*shape)
            return "k_geglu_persist", False, "persist"
        N = shape[-1]
        M = math.prod(shape[:3]) * (4 if self.op == "up2x" else 1) if self.op in CONVS else shape[0]
        ncb = -(-N // (2 * ops.GEMM_BN))
        has_rows = self.op in ("linear", "conv")                     # launch(): !OUT32 && EPI == 1 && CONV < CONV_UP2X
        auto = ops.gemm_rows_mode(M, ncb)                           # the launcher's own choice (a grid this small: always 128-row tiles) ...
        rows = has_rows and (auto if self.rows_env is None else self.rows_env == "1")      # ... which ED_GEMM_ROWS overrides at every launch
        half = not rows and (ncb - 1) * 2 * ops.GEMM_BN + ops.GEMM_BN >= N     # the LAST column block: n0 + BN >= I
        two = self.op in CONVS and k_len(self.op, shape) // 64 >= TWO_MIN_TILES
        loop = "rows" if rows else "half" if (half and ncb == 1) else "two" if two else "8phase"
        return "k_gemm_8phase", bool(combo[1] or combo[2]), loop

    def run(self, ops, c, out=None):
        """one launch on device tensors.  ``out`` None: through the ops wrapper (which allocates); else through the C ABI into ``out``."""
        op, cl = self.op, (lambda t: None if t is None else t.permute(0, 3, 1, 2))
        if out is None:
            if op == "geglu":
                return ops.geglu_gemm(c.x, c.w, c.bias)
            if op == "linear":
                return ops.linear(c.x, c.w, c.bias, c.residual)
            x, w = cl(c.x), cl(c.w)
            if op == "conv":
                y = ops.conv3x3_nhwc(x, w, c.bias, c.sample_bias, cl(c.residual))
            elif op == "up2x":
                y = ops.conv3x3_nhwc_up2x(x, w, c.bias)
            elif op == "s2":
                y = ops.conv3x3_nhwc_s2(x, w, c.bias)
            elif op == "f32out":
                y = ops.conv3x3_f32out(x, w, c.bias, cl(c.residual), c.out_scale)
            else:
                y = ops.conv3x3_f32out_s2(x, w, c.bias, c.out_scale)
            return y.permute(0, 2, 3, 1)
        p = lambda t: None if t is None else t.data_ptr()
        code = ops._DTYPE[c.dtype]
        stream = torch.cuda.current_stream(c.x.device).cuda_stream
        if op == "geglu":
            ops._call("ed_geglu_gemm", p(c.x), p(c.w), p(c.bias), p(out), code, *c.shape, stream)
        elif op == "linear":
            ops._call("ed_linear", p(c.x), p(c.w), p(c.bias), p(c.residual), p(out), code, *c.shape, stream)
        else:
            B, H, W, N = c.out_shape
            Cin = c.shape[3]
            if op == "conv":
                ops._call("ed_conv3x3_nhwc", p(c.x), p(c.w), p(c.bias), p(c.sample_bias), p(c.residual), p(out), code, B, H, W, Cin, N, stream)
            elif op in ("up2x", "s2"):
                ops._call("ed_conv3x3_nhwc_" + op, p(c.x), p(c.w), p(c.bias), p(out), code, B, H, W, Cin, N, stream)
            elif op == "f32out":
                ops._call("ed_conv3x3_nhwc_f32out", p(c.x), p(c.w), p(c.bias), p(c.residual), p(out), code, B, H, W, Cin, N,
                          float(c.out_scale), None, stream)
            else:
                ops._call("ed_conv3x3_nhwc_f32out_s2", p(c.x), p(c.w), p(c.bias), p(out), code, B, H, W, Cin, N, float(c.out_scale), None, stream)
        return out


GEMM_BASE = (300, 192, 136)            # two row blocks (three of 128), 3 K tiles, a second column half of 8 columns
CONV_BASE = (3, 5, 7)                  # M = 105 (420 for up2x): two seams inside the first tile


def _targets():
    f16, bf16 = torch.float16, torch.bfloat16
    ts = [Target("geglu", d, False, "persist", (300, 192, 256), True) for d in (bf16, f16)]
    for d in (f16, bf16):
        for add in (False, True):
            ts.append(Target("linear", d, add, "8phase", GEMM_BASE, True))
            ts.append(Target("linear", d, add, "rows", GEMM_BASE, True))
        ts.append(Target("linear", d, False, "half", (300, 192, 72)))
    for d in (f16, bf16):
        for add in (False, True):
            ts.append(Target("conv", d, add, "8phase", CONV_BASE + (64, 136), True))
            ts.append(Target("conv", d, add, "two", CONV_BASE + (192, 136)))
            ts.append(Target("conv", d, add, "rows", CONV_BASE + (64, 136), True))
        ts.append(Target("conv", d, False, "half", CONV_BASE + (64, 72)))
    for op in ("up2x", "s2"):
        for d in (f16, bf16):
            ts.append(Target(op, d, False, "8phase", CONV_BASE + (64, 136), True))
            ts.append(Target(op, d, False, "two", CONV_BASE + (192, 136)))
    for add in (False, True):       # Cin' = 64: the only widths below TWO_MIN_TILES (a real split operand [hi | lo | hi] has Cin' = 3 Cin >= 192)
        ts.append(Target("f32out", f16, add, "8phase", CONV_BASE + (64, 136), True))
        ts.append(Target("f32out", f16, add, "two", CONV_BASE + (192, 136)))
    ts.append(Target("f32out_s2", f16, False, "8phase", CONV_BASE + (64, 136), True))
    ts.append(Target("f32out_s2", f16, False, "two", CONV_BASE + (192, 136)))
    return tuple(ts)


TARGETS = _targets()
GEMM_M, GEMM_K, GEMM_N = (1, 15, 127, 128, 129, 257, 300), (64, 128, 192, 640), (8, 72, 128, 136, 264)
CONV_GEOM = ((5, 1, 1), (3, 1, 9), (3, 9, 1), (4, 2, 2), (3, 5, 7), (2, 12, 20))
CONV_CIN, CONV_N = (64, 128, 192, 960, 2560), (8, 72, 136)


def sweep_shapes(t):
    """one axis at a time around the base shape; the long Cin with the smallest (B, H, W, N) only"""
    if t.op not in CONVS:
        M0, K0, N0 = t.shape
        ns = (128, 256, 384) if t.op == "geglu" else GEMM_N
        s = [(M, K0, N0) for M in GEMM_M] + [(M0, K, N0) for K in GEMM_K] + [(M0, K0, N) for N in ns]
    else:
        B0, H0, W0, C0, N0 = t.shape
        s = [g + (C0, N0) for g in CONV_GEOM] + [(B0, H0, W0, C, N0) for C in CONV_CIN if C < 960] \
            + [CONV_GEOM[0] + (C, CONV_N[0]) for C in CONV_CIN if C >= 960] + [(B0, H0, W0, C0, N) for N in CONV_N]
    return tuple(dict.fromkeys(s))


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def _uni(shape, g, scale=1.0):
    """uniform [-1, 1) times scale (asymmetric by construction: a transposed operand or store cannot pass)"""
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def make(t, shape=None, combo=None, seed=0, x_scale=1.0, w_scale=1.0, add_scale=1.0, out_scale=0.25):
    """uniform operands: x ~ x_scale, w ~ w_scale K^-1/2, addends ~ add_scale"""
    shape = t.shape if shape is None else shape
    combo = t.combos[0] if combo is None else combo
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    c = Case(t.op, t.dtype, tuple(shape), None, None)
    if t.op in OUT32:              # the split weights' power-of-two pre-scaling and the epilogue's out_scale that undoes it
        c.out_scale, w_scale = out_scale, w_scale / out_scale
    c.x = _uni(x_shape(t.op, shape), g, x_scale).to(t.dtype)
    c.w = _uni(w_shape(t.op, shape), g, w_scale * k_len(t.op, shape) ** -0.5).to(t.dtype)
    n_bias = c.w.shape[0]
    if combo[0]:
        c.bias = _uni((n_bias,), g, add_scale).to(c.add_dtype)
    if combo[1]:
        c.sample_bias = _uni((shape[0], n_bias), g, add_scale).to(c.add_dtype)
    if combo[2]:
        c.residual = _uni(c.out_shape, g, add_scale).to(c.add_dtype)
    return c


SCALES = {torch.float16: (2.0 ** -7, 1.0, 180.0), torch.bfloat16: (2.0 ** -7, 1.0, 180.0, 2.0 ** 100, 2.0 ** -100)}


def scaled(t, scale, shape=None, combo=None, seed=1):
    """Uniform data at activation scale ``scale``; the addends follow the scale.  bf16 at 2^100 / 2^-100: the weights are scaled the
    other way (and the addends are O(1)) so that the outputs stay finite.  GEGLU at 180 keeps an O(1) bias: its output is a product
    of two projections.  Asserts the median |ref64| (GEGLU: the upper quartile -- gelu sends half of the gates to nearly nothing) is
    within [1e-3, 4] of the scale the outputs should have, and that all is finite."""
    far = scale in (2.0 ** 100, 2.0 ** -100)
    assert not far or t.dtype == torch.bfloat16
    sw = 1.0 / scale if far else 1.0
    sa = 1.0 if far or (t.op == "geglu" and scale > 1) else scale
    c = make(t, shape, combo, seed, scale, sw, sa)
    ref = ref64(c)
    s_out = scale * sw
    want = s_out * s_out if t.op == "geglu" else s_out
    med = float(ref.abs().flatten().quantile(0.75)) if t.op == "geglu" else float(ref.abs().median())
    assert bool(torch.isfinite(ref).all()) and 1e-3 * want <= med <= 4 * want, (t.name, scale, med, want)
    if c.out_dtype == torch.float16:
        assert float(ref.abs().max()) < 60000, (t.name, scale, float(ref.abs().max()))
    c.note.update(median=med, scale=scale)
    return c


def cancelling(t, combo, shape=None, seed=2):
    """The addends cancel the accumulator.  With a residual: weights x 8 and residual = -(acc + bias + sample_bias) + uniform * 0.01
    rounded to 16 bits.  Without (bias + sample_bias): the two split a cancellation between them, bias ~ 64 and sample_bias = -bias +
    uniform * 0.01 on a small accumulator.  Asserts max |largest term| > 100 max |ref64| (note['big']: 'acc' or 'bias')."""
    assert combo[1] or combo[2]
    if combo[2]:
        c = make(t, shape, combo, seed, 1.0, 8.0, 1.0)
        part = replace(c, residual=None)
        acc = contraction(part) + addends(part)
        g = torch.Generator().manual_seed(77 + seed)
        c.residual = (-acc + _uni(acc.shape, g, 0.01)).to(c.add_dtype)
        big, which = contraction(c), "acc"
    else:
        c = make(t, shape, combo, seed, 1.0, 1.0 / 64, 64.0)
        g = torch.Generator().manual_seed(78 + seed)
        c.sample_bias = (-c.bias.double()[None, :] + _uni(c.sample_bias.shape, g, 0.01)).to(c.add_dtype)
        big, which = c.bias.double(), "bias"
    ref = ref64(c)
    assert float(big.abs().max()) > 100 * float(ref.abs().max()), (t.name, combo, float(big.abs().max()), float(ref.abs().max()))
    c.note.update(big=which, ratio=float(big.abs().max()) / float(ref.abs().max()))
    return c


def double_rounded(c):
    """the stand-in that `cancelling` must catch: fp32 sums, but the large term (the accumulator; for the bias / sample_bias case the
    accumulator + bias) is rounded to the 16-bit type before the rest is added"""
    f = torch.float32
    acc = contraction(c, f)
    if c.note["big"] == "acc":
        s = acc.to(c.dtype).to(f) + addends(c, f)
    else:
        s = (acc + c.bias.to(f)).to(c.dtype).to(f) + addends(replace(c, bias=None), f)
    return s.to(c.out_dtype)


def near_max(t, combo, shape=None, seed=3):
    """fp16: outputs planted on both sides of 65504.  A quarter of the columns carry bias = +65504, a quarter -65504, on an
    accumulator of sigma 16 (one fp16 step there is 32; a residual, where there is one, is O(1)); GEGLU: value bias 255, gate bias
    256.9 on those columns (gelu(g) = g there).  -> case with note['inf'] (where the one-rounding stand-in round16(ref64) is
    +-inf), note['skip'] (|ref64| within KAPPA 2^-24 absprod64 -- GEGLU: within the bar's accumulation terms -- of 65520: undecidable)
    and note['planted'].  Asserts at most 1 % of the planted elements are undecidable and at least 32 land on each side."""
    assert t.dtype == torch.float16 and t.op not in OUT32 and combo[0]
    c = make(t, shape, combo, seed, 1.0, 1.0 if t.op == "geglu" else 48.0, 1.0)
    n = c.out_shape[-1]
    cols = torch.arange(n)
    pos, neg = cols % 4 == 1, cols % 4 == 3
    b = c.bias.clone()
    if t.op == "geglu":
        b[:n][pos], b[:n][neg] = 255.0, -255.0
        b[n:][pos | neg] = 256.875
    else:
        b[pos], b[neg] = F16_MAX, -F16_MAX
    c.bias = b
    ref, bb = bar(c)
    margin = bb - U[torch.float16] * ref.abs()
    planted = torch.zeros_like(ref, dtype=torch.bool)
    planted[..., pos | neg] = True
    once = round_to(ref, torch.float16)
    inf = torch.isinf(once)
    skip = ((ref.abs() - F16_INF_FROM).abs() <= margin) & planted
    over, under = int((inf & ~skip).sum()), int((planted & ~inf & ~skip).sum())
    share = float(skip.sum()) / float(planted.sum())
    assert not bool((inf & ~planted).any()) and share <= 0.01 and over >= 32 and under >= 32, (t.name, share, over, under)
    c.note.update(inf=inf, skip=skip, planted=planted, share=share, over=over, under=under)
    return c


def subnormal(t, combo, which, shape=None, seed=4):
    """fp16: ``which`` = 'x': every activation below 2^-14 in magnitude (uniform * 2^-15) against weights ~ 2^10 K^-1/2; 'w': the
    other way round.  The addends are ~ 2^-8 (GEGLU: gate bias 1 + that, so the product stays a normal number).  Asserts the operand
    is entirely subnormal and mostly non-zero, and that the median |ref64| is a normal fp16 number (> 2^-10; GEGLU's product > 2^-14):
    a matrix instruction that flushed the operand would return the addends alone (``flushed``), which the bar refuses."""
    assert t.dtype == torch.float16 and (t.op != "geglu" or combo[0])
    sx, sw = (2.0 ** -15, 2.0 ** 10) if which == "x" else (2.0 ** 10, 2.0 ** -15 * k_len(t.op, t.shape if shape is None else shape) ** 0.5)
    c = make(t, shape, combo, seed, sx, sw, 2.0 ** -8, out_scale=1.0)
    if t.op == "geglu" and c.bias is not None:
        c.bias[c.shape[2]:] += 1.0
    small = c.x if which == "x" else c.w
    assert float(small.double().abs().max()) < 2.0 ** -14 and float(small.double().abs().median()) > 0
    ref = ref64(c)
    med = float(ref.abs().median())
    assert med > (2.0 ** -14 if t.op == "geglu" else 2.0 ** -10), (t.name, which, med)
    c.note.update(which=which, median=med)
    return c


def flushed(c):
    """the stand-in `subnormal` must catch: the subnormal operand read as zeros"""
    z = replace(c, **{c.note["which"]: torch.zeros_like(getattr(c, c.note["which"]))})
    return ref64(z).to(c.out_dtype)


GATES = (-12.0, -10.0, -8.0, -7.0, -6.0, -5.5, -5.0, -4.0, -3.0, -2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 5.5, 6.0, 8.0,
         10.0, 12.0, -11.5, -9.0, -6.5, -4.5, -3.5, -2.5, -1.5, 1.5, 2.5, 3.5, 4.5, 6.5, 9.0, 11.5)
VALUES = (1000.0, -1000.0, 1.0, -1.0, 0.5, 320.0, -77.0, 12.5, -0.0625, 640.0, 3.0)


def gate_tails(t, shape=None, seed=5):
    """GEGLU with the value and gate pre-activations planted by construction: row m of x is one hot at column m % K, so
    v[m, n] = w[n, m % K] and g[m, n] = w[I + n, m % K] exactly (no bias).  Gates cover [-12, 12] including +-0 (as weights: the
    sum with the other columns' +0 products is +0), -8, -6, -5, -3, 3 and 6 (all exact in bf16), values reach 1000.  Asserts the pre-activations are the planted ones, exactly."""
    assert t.op == "geglu"
    M, K, I = t.shape if shape is None else shape
    c = Case("geglu", t.dtype, (M, K, I), torch.zeros(M, K, dtype=t.dtype), None)
    c.x[torch.arange(M), torch.arange(M) % K] = 1.0
    n, k = torch.arange(I)[:, None], torch.arange(K)[None, :]
    gates, values = torch.tensor(GATES, dtype=torch.float64), torch.tensor(VALUES, dtype=torch.float64)
    g, v = gates[(7 * n + 13 * k + seed) % len(GATES)], values[(n + 3 * k) % len(VALUES)]
    c.w = torch.cat([v, g], 0).to(t.dtype)
    assert torch.equal(c.w.double(), torch.cat([v, g], 0))                      # every planted number is exact in the 16-bit type
    y = contraction(c)
    rows = torch.arange(M) % K
    assert torch.equal(y[:, :I], v.t()[rows]) and torch.equal(y[:, I:], g.t()[rows])
    seen = set(y[:, I:].flatten().tolist())
    assert all(s in seen for s in (-12.0, -8.0, -6.0, -5.0, -3.0, 0.0, 3.0, 6.0, 12.0))
    assert float(y[:, :I].abs().max()) >= 1000.0
    return c


def gelu_fit_fp32(g):
    """geglu_one's gelu(g) = max(g, 0) - |g| hq in fp32 with an exact division and exp2 (numpy; every step rounded to fp32, the fused
    multiply-adds computed in float64 and rounded once)"""
    import numpy as np
    f = np.float32
    g = g.astype(f)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f)
    z = np.abs(g) * f(0.70710678118654752)
    t = f(1.0) / fma(np.full_like(z, f(0.3275911)), z, f(1.0))
    p = fma(np.full_like(t, f(0.5) * f(1.061405429)), t, f(0.5) * f(-1.453152027))
    for coef in (1.421413741, -0.284496736, 0.254829592):
        p = fma(p, t, f(0.5) * f(coef))
    hq = (p * t) * np.exp2(((f(-1.4426950408889634) * z) * z).astype(np.float64)).astype(f)
    return np.maximum(g, f(0)) - np.abs(g) * hq


NONFINITE = (float("inf"), float("-inf"), float("nan"))


def nonfinite(t, combo, which, shape=None, seed=6):
    """+Inf, -Inf and NaN planted in ``which`` = 'x': the four corners of the middle sample, the last pixel of sample 0 and the first
    of sample 1 (images of at most four input pixels: every pixel of sample 1 instead), the last pixel of the last sample (row M - 1 of a ragged tile), pixels 128 and
    256 (the first row of the next tile), for s2 / f32out_s2 a pixel of the last input row and one of the last input column; GEMM:
    rows 0, 127, 128, 255, 256 and M - 1.  'w': row N - 1, the rows at the 128-column boundary and one bias element (convolutions:
    on the centre tap, which no output pixel has outside the image).  One channel each.
    -> note['finite']: isfinite of the fp32 CPU reference.  Asserts that it equals isfinite(ref64) and, for 'x', the planted pixels'
    3 x 3 (strided, upsampled) fields and nothing else; that at least 10 % of the elements are finite and some are not."""
    c = make(t, shape, combo, seed)
    conv = t.op in CONVS
    plant = c.x if which == "x" else c.w
    mark = torch.zeros(plant.shape, dtype=torch.float64)
    spots = []
    if which == "x" and conv:
        B, Hi, Wi, C = c.x.shape
        if Hi * Wi > 4:
            spots += [(B // 2, y, x) for y in (0, Hi - 1) for x in (0, Wi - 1)]
            spots += [(0, Hi - 1, Wi - 1), (1, 0, 0), (B - 1, Hi - 1, Wi - 1)]
        else:       # an image of one or four pixels is all corners: every pixel of sample 1 (its neighbours on both sides must stay finite)
            spots += [(1, y, x) for y in range(Hi) for x in range(Wi)] + [(B - 1, Hi - 1, Wi - 1)]
        spots += [(m // (Hi * Wi), m % (Hi * Wi) // Wi, m % Wi) for m in (128, 256) if m < B * Hi * Wi - Wi - 2]
        if t.op in ("s2", "f32out_s2") and Hi * Wi > 4:
            spots += [(B - 1, Hi - 1, Wi // 2 - 1), (0, Hi // 2 - 1, Wi - 1)]
    elif which == "x":
        spots += [(m,) for m in (0, 127, 128, 255, 256, c.shape[0] - 1) if m < c.shape[0]]
    else:
        N = c.out_shape[-1]
        rows = [N - 1] + [r for r in (127, 128) if r < N - 1]
        if t.op == "geglu":
            rows += [N, 2 * N - 1]
        spots += [(r, 1, 1) if conv else (r,) for r in rows]
    for i, s in enumerate(dict.fromkeys(spots)):
        ch = (7 * i + 3) % plant.shape[-1]
        plant[s + (ch,)] = NONFINITE[i % 3]
        mark[s + (ch,)] = 1.0
    if which == "w" and c.bias is not None:
        c.bias[3] = float("nan")
    fin32, fin64 = torch.isfinite(ref64(c, torch.float32)), torch.isfinite(ref64(c))
    assert torch.equal(fin32, fin64), (t.name, which)
    if which == "x":
        ind = replace(c, x=mark, w=torch.ones(c.w.shape, dtype=torch.float64), bias=None, sample_bias=None, residual=None, out_scale=1.0)
        hit = contraction(ind) > 0
        if t.op == "geglu":
            hit = hit[:, :c.shape[2]]
        assert torch.equal(~hit, fin64), (t.name, "the spoiled elements are not the planted pixels' fields")
    share = float(fin64.double().mean())
    assert 0.1 <= share < 1.0, (t.name, which, share)
    c.note.update(finite=fin32, share=share, which=which)
    return c


def coded_gemm(t, combo, shape=None):
    """x[m] = [a_m, 1, 0, ...], w[n] = [1, b_n, 0, ...]: out[m, n] = a_m + b_n exactly (fp16: a = m % 1024, b = n % 1024; bf16:
    a = m % 128, b = 128 (n % 2)); zero addends where the instantiation has them.  GEGLU: the gate rows are [0, 0, 16, 0, ...] against
    x[m, 2] = 1 (gelu(16) = 16 exactly in fp32: its erfc term underflows), so out = 16 (a_m + b_n).  -> note['want'] (output dtype).
    Asserts, in float64, that want is the operation's exact value and exact in the output type."""
    M, K, N = t.shape if shape is None else shape
    f16 = t.dtype == torch.float16
    a = (torch.arange(M) % (1024 if f16 else 128)).double()
    b = (torch.arange(N) % 1024).double() if f16 else 128.0 * (torch.arange(N) % 2).double()
    c = Case(t.op, t.dtype, (M, K, N), torch.zeros(M, K, dtype=t.dtype), torch.zeros(w_shape(t.op, (M, K, N)), dtype=t.dtype))
    c.x[:, 0], c.x[:, 1] = a.to(t.dtype), 1.0
    c.w[:N, 0], c.w[:N, 1] = 1.0, b.to(t.dtype)
    want = a[:, None] + b[None, :]
    if t.op == "geglu":
        c.x[:, 2], c.w[N:, 2] = 1.0, 16.0
        want = 16.0 * want
    if combo[0]:
        c.bias = torch.zeros(c.w.shape[0], dtype=c.add_dtype)
    if combo[2]:
        c.residual = torch.zeros(c.out_shape, dtype=c.add_dtype)
    ref = ref64(c)
    assert float((ref - want).abs().max()) < 1e-9 * 16 and torch.equal(want.to(c.out_dtype).double(), want)
    c.note["want"] = want.to(c.out_dtype)
    return c


def shifted_image(op, x, tap):
    """what an identity weight on ``tap`` (0..8, row-major) must give: the zero-padded input read at each variant's tap position,
    by index arithmetic alone.  x [B, Hi, Wi, C] -> [B, H, W, C]"""
    ty, tx = tap // 3, tap % 3
    if op == "up2x":
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    P = F.pad(x, (0, 0, 1, 1, 1, 1))
    B, Hp, Wp, C = P.shape
    s, off = (2, 0) if op == "s2" else (2, 1) if op == "f32out_s2" else (1, 0)
    H, W = (Hp - 2) // s, (Wp - 2) // s
    ys, xs = s * torch.arange(H) + ty + off, s * torch.arange(W) + tx + off
    return P[:, ys][:, :, xs]


def coded_conv(t, combo, tap, shape=None):
    """N = Cin and w = the identity over channels on tap ``tap``, zero elsewhere; x holds small integers ((31 m + 7 c) % 255 - 127,
    exact in bf16): the output is the shifted, zero-padded image, exactly (Cin < 136: 136 output columns, the ones past Cin with zero
    weights, so that the column block is a full one and not the `half` loop's).  Split widths (f32out, Cin' = 192): x = [hi | lo = 0 | hi],
    w = [wh | wh | wl = 0] with N = 64: the output is the hi part.  Zero addends.  -> note['want'].  Asserts that ref64 is that image."""
    B, H, W, Cin, _ = t.shape if shape is None else shape
    split = t.op in OUT32 and Cin % 192 == 0
    C1 = Cin // 3 if split else Cin
    N = max(C1, 136)
    shape = (B, H, W, Cin, N)
    xs = x_shape(t.op, shape)
    m, ch = torch.arange(math.prod(xs[:3])).reshape(xs[:3])[..., None], torch.arange(C1)
    hi = ((31 * m + 7 * ch) % 255 - 127).double()
    eye = torch.eye(C1, dtype=torch.float64)
    w = torch.zeros(N, 3, 3, Cin, dtype=torch.float64)
    if split:
        x = torch.cat([hi, torch.zeros_like(hi), hi], -1)
        w[:C1, tap // 3, tap % 3, :2 * C1] = torch.cat([eye, eye], 1)
    else:
        x = hi
        w[:C1, tap // 3, tap % 3] = eye
    c = Case(t.op, t.dtype, shape, x.to(t.dtype), w.to(t.dtype))
    if combo[0]:
        c.bias = torch.zeros(N, dtype=c.add_dtype)
    if combo[1]:
        c.sample_bias = torch.zeros(B, N, dtype=c.add_dtype)
    if combo[2]:
        c.residual = torch.zeros(c.out_shape, dtype=c.add_dtype)
    want = F.pad(shifted_image(t.op, hi, tap), (0, N - C1))
    assert torch.equal(ref64(c), want) and torch.equal(c.x.double(), x)
    c.note["want"] = want.to(c.out_dtype)
    return c


# ---- guarded: operands and output carved out of one allocation -----------------------------------------------------------------------
GUARD_BYTES = 4096
SENTINEL = 0x5A


@dataclass
class Arena:
    buf: torch.Tensor              # uint8, the one allocation
    case: Case                     # the operands as views into buf
    out: torch.Tensor              # the output view (pre-filled with NaN)
    bands: list                    # (name, lo, hi, snapshot) byte ranges that must not change
    out_bands: list                # the two sentinel bands around the output


def guarded(c, device):
    """One uint8 allocation on ``device`` holding, each 16-byte aligned: [NaN band] x [NaN band] w [NaN band] bias ... [NaN band]
    [sentinel band >= 4 KiB] out (NaN) [sentinel band >= 256 output rows].  The NaN bands are NaN in the dtype of the operand in
    front of them.  -> Arena; ``guard_check`` after the launch.  Nothing the kernel may touch lies outside the allocation."""
    ops = list(c.tensors().items())
    al = lambda n: -(-n // 16) * 16
    nbytes = lambda t: t.numel() * t.element_size()
    out_elem = torch.empty((), dtype=c.out_dtype).element_size()
    out_bytes = math.prod(c.out_shape) * out_elem
    tail = al(max(GUARD_BYTES, 256 * c.out_shape[-1] * out_elem))
    total = GUARD_BYTES + sum(al(nbytes(t)) + GUARD_BYTES for _, t in ops) + GUARD_BYTES + al(out_bytes) + tail
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    pos, views, bands = 0, {}, []

    def nan_band(dtype, name):
        nonlocal pos
        buf[pos:pos + GUARD_BYTES].view(dtype).fill_(float("nan"))
        bands.append((name, pos, pos + GUARD_BYTES))
        pos += GUARD_BYTES

    nan_band(ops[0][1].dtype, "before " + ops[0][0])
    for name, t in ops:
        n = nbytes(t)
        v = buf[pos:pos + n].view(t.dtype).view(t.shape)
        v.copy_(t)
        views[name] = v
        fill = al(n) - n
        pos += n
        if fill:
            buf[pos:pos + fill].view(torch.float16).fill_(float("nan"))
            bands.append(("pad after " + name, pos, pos + fill))
            pos += fill
        nan_band(t.dtype, "after " + name)
    lo = pos
    pos += GUARD_BYTES
    out = buf[pos:pos + out_bytes].view(c.out_dtype).view(c.out_shape)
    out.fill_(float("nan"))
    out_bands = [("before out", lo, pos), ("after out", pos + out_bytes, total)]
    assert total - (pos + out_bytes) >= 256 * c.out_shape[-1] * out_elem and out.data_ptr() % 16 == 0
    assert all(v.data_ptr() % 16 == 0 for v in views.values())
    snap = lambda bs: [(n, a, b, buf[a:b].clone()) for n, a, b in bs]
    return Arena(buf, replace(c, **views), out, snap(bands), snap(out_bands))


def guard_check(a, c):
    """after the launch: the operands and their NaN bands are untouched, both sentinel bands around the output are bit-identical"""
    for name, lo, hi, was in a.out_bands + a.bands:
        now = a.buf[lo:hi]
        if not torch.equal(now, was):
            i = int((now != was).nonzero()[0, 0])
            raise AssertionError(f"band '{name}' changed at byte {i} of {hi - lo} ({int(was[i])} -> {int(now[i])})")
    for name, t in c.tensors().items():
        v = getattr(a.case, name)
        assert torch.equal(v.view(torch.uint8).cpu(), t.contiguous().view(torch.uint8)), f"operand {name} was written"


GUARD_SHAPES = {    # ragged M; N = 8, 72 and 136; grids whose tile count and row-block count are no multiples of 8 (the XCD walk's remainder path)
    "linear": ((300, 192, 8), (300, 192, 72), (300, 192, 136), (2400, 64, 264)),
    "geglu": ((300, 192, 256), (2400, 64, 384), (22017, 64, 384)),     # the last: 261 tiles on at most 256 workgroups -- the persistent loop's second tile
    "conv": ((3, 5, 7, None, 8), (3, 5, 7, None, 72), (3, 5, 7, None, 136), (11, 12, 20, None, 264)),
}


def nonfinite_shapes(t):
    """the base shape; for the sweep targets also every image geometry / a one- and a two-K-tile GEMM with M just past a tile"""
    if t.sweep and t.op in CONVS:
        return [t.shape] + [g + t.shape[3:] for g in CONV_GEOM if g != t.shape[:3]]
    return [t.shape] + ([(129, 64, t.shape[2]), (257, 128, t.shape[2])] if t.sweep else [])


def guard_shapes(t):
    if t.op not in CONVS:
        return GUARD_SHAPES[t.op]
    out = []
    for B, H, W, _, N in GUARD_SHAPES["conv"]:
        if B == 11:       # 2640 output pixels: 11 row blocks of 256 (21 of 128) x 2 column blocks; always with the shortest K
            B, H, W = (11, 12, 20) if t.op in ("conv", "f32out") else (11, 6, 10) if t.op == "up2x" else (11, 12, 20)
            out.append((B, H, W, 64, N))
        else:
            out.append((B, H, W, t.shape[3], N))
    return tuple(out)


# ---- CPU stand-ins for the faults the cases must catch (tests/test_gemm_cases.py) -----------------------------------------------------
def conv_standin(c, fault=None):
    """The stride-1 convolution the way the kernel addresses it, in fp32 on the CPU: output pixel m reads flat pixel m + dy W + dx of
    the [M, Cin] image, a tap outside the image contributes zeros.  ``fault``: 'mask_multiply' (the clamped neighbour is loaded and
    multiplied by a 0 / 1 mask), 'cross_sample' (the vertical mask ignores sample seams), 'wrong_tap' (dx mirrored).  None: correct."""
    assert c.op == "conv"
    B, H, W, Cin, N = c.shape
    M, f = B * H * W, torch.float32
    x, w = c.x.to(f).reshape(M, Cin), c.w.to(f)
    m = torch.arange(M)
    py, px = m % (H * W) // W, m % W
    gy = m // W                                        # row of the batch seen as one tall image
    acc = torch.zeros(M, N, dtype=f)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        ok_y = ((gy + dy >= 0) & (gy + dy < B * H)) if fault == "cross_sample" else ((py + dy >= 0) & (py + dy < H))
        ok = ok_y & (px + dx >= 0) & (px + dx < W)
        src = (m + dy * W + (-dx if fault == "wrong_tap" else dx)).clamp(0, M - 1)
        rows = x[src]
        rows = rows * ok[:, None].to(f) if fault == "mask_multiply" else torch.where(ok[:, None], rows, torch.zeros((), dtype=f))
        acc += rows @ w[:, tap // 3, tap % 3].t()
    return (acc.reshape(B, H, W, N) + addends(c, f)).to(c.out_dtype)


def sequential_fp32(c):
    """a strictly sequential fp32 sum over k of the contraction (one element at a time along K, vectorised over the outputs)"""
    f = torch.float32
    if c.op in CONVS:
        x, w = c.x.to(f).permute(0, 3, 1, 2), c.w.to(f)
        if c.op == "up2x":
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        s, pad = (1, (1, 1, 1, 1)) if c.op in ("conv", "up2x", "f32out") else (2, (1, 1, 1, 1)) if c.op == "s2" else (2, (0, 1, 0, 1))
        cols = F.unfold(F.pad(x, pad), 3, stride=s)                              # [B, Cin * 9, L], k = channel-major then tap
        A = cols.transpose(1, 2).reshape(-1, cols.shape[1])
        Wm = w.permute(0, 3, 1, 2).reshape(w.shape[0], -1)
    else:
        A, Wm = c.x.to(f), c.w.to(f)
    acc = torch.zeros(A.shape[0], Wm.shape[0], dtype=f)
    for k in range(A.shape[1]):
        acc += A[:, k, None] * Wm[None, :, k]
    return acc.reshape(contraction(c, f).shape) * c.out_scale
