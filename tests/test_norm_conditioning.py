"""The normalisation kernels on data whose mean is large next to its spread.

Every GroupNorm entry point (ed_groupnorm plain and split path, ed_groupnorm_nhwc / _cat / _s32, ed_groupnorm_f32,
ed_groupnorm_nhwc_f32 plain and split) against an fp64 torch reference of the same operation on the same inputs, over five input
classes built with a seeded CPU generator (statistics are per (sample, group)):

  A  offset        m + s * randn
  B  outlier       randn with one channel of every group shifted (+50 in the 16-bit types, +1e4 in fp32): a large variance that is real
  C  per group     a different offset in every (sample, group): a shift or statistic taken from the wrong group / sample fails here
  D  constant      group 0 of sample 0 holds exactly one value, the rest is randn
  E  scale         fp32 only: randn * 2^40 and randn * 2^-20 (where eps dominates)

Bars.  16-bit outputs: every element |got - ref| <= 2 ulp |ref| + 4 ulp (the suite's GroupNorm bar; LayerNorm 1 ulp |ref| + 2 ulp).
fp32 outputs: every element |got - ref| <= 2 max|torch_fp32 - ref| + floor, floor = 4 rstd |gamma_c| ulp32(|mean|) + 2e-6: the first
term is what any implementation pays for holding the mean (and beta - a mean) in fp32, the constant is test_groupnorm_f32's.  torch's
error is measured at run time on the same device, and its maximum is taken per (sample, group) -- the stricter reading: a group where
torch is accurate does not borrow slack from one where it is not.  Every launch is repeated and must be bit-identical.

The unmarked tests at the end run an ideal implementation (torch's CPU fp32 GroupNorm, rounded once to the output type) against the
same bars: a bar the reference alone cannot meet would be a bug in this file.  (For fp32 inputs with a 16-bit output the ideal is the
centred fp32 form on correctly rounded statistics, and torch's figure is printed beside it: see that test.)
"""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NAME = {F16: "fp16", BF16: "bf16", F32: "fp32"}

# (class, parameters) per input type
CASES = {
    F16: [("A", 300.0, 1.0), ("A", 1000.0, 1.0), ("A", 64.0, 0.25), ("A", -200.0, 1.0), ("B",), ("C",), ("D", 0.75), ("D", 100.0)],
    BF16: [("A", 100.0, 1.0), ("A", -200.0, 2.0), ("A", 30.0, 0.25), ("B",), ("C",), ("D", 0.75), ("D", 100.0)],
    F32: [("A", 100.0, 1.0), ("A", 1e3, 1.0), ("A", 1e4, 1.0), ("A", -3e3, 5.0), ("A", 1e6, 100.0), ("B",), ("C",), ("D", 100.1),
          ("E", 2.0 ** 40), ("E", 2.0 ** -20)],
}
CLASS_A = {dt: [c for c in cs if c[0] == "A"] for dt, cs in CASES.items()}


def _id(v):
    if isinstance(v, torch.dtype):
        return NAME[v]
    if isinstance(v, tuple) and v and isinstance(v[0], str):
        return v[0] + "".join(f"_{p:g}" for p in v[1:])
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return str(v)


def typed_cases(dtypes):
    return [pytest.param(dt, c, id=f"{NAME[dt]}-{_id(c)}") for dt in dtypes for c in CASES[dt]]


def make_input(case, dtype, shape, G, seed=0):
    """[N, C, H, W] CPU tensor of ``dtype`` (NCHW-contiguous) of the given input class."""
    N, C, H, W = shape
    cpg = C // G
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + H * W + N)
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    wide = dtype == F32
    kind = case[0]
    if kind == "A":
        x = case[1] + case[2] * r
    elif kind == "B":       # the shifted channel is the group's first in some groups and a later one in others
        x = r.view(N, G, cpg, H, W).clone()
        for gi in range(G):
            x[:, gi, gi % cpg] += 1e4 if wide else 50.0
        x = x.view(N, C, H, W)
    elif kind == "C":
        n_i, g_i = torch.arange(N).view(N, 1), torch.arange(G).view(1, G)
        off = (1.0 - 2.0 * (g_i % 2)) * 40.0 * (1 + (g_i + 3 * n_i) % 5) * (100.0 if wide else 1.0)
        x = (r.view(N, G, cpg, H, W) + off.view(N, G, 1, 1, 1).double()).view(N, C, H, W)
    elif kind == "D":
        x = r.clone()
        x[0, :cpg] = case[1]
    elif kind == "E":
        x = r * case[1]
    else:
        raise ValueError(kind)
    return x.to(dtype).contiguous()


def make_affine(C, dtype, seed=0):
    g = torch.Generator().manual_seed(77 + C + seed)
    return (1 + 0.2 * torch.randn(C, generator=g)).to(dtype), (0.1 * torch.randn(C, generator=g)).to(dtype)


def ref64(x, G, w, b, eps, silu):
    """fp64 GroupNorm (+SiLU) of the values of x; also the reference mean and rstd per (sample, group)."""
    x64 = x.double()
    y = F.group_norm(x64, G, w.double(), b.double(), eps)
    if silu:
        y = F.silu(y)
    N = x.shape[0]
    grp = x64.reshape(N, G, -1)
    mean = grp.mean(-1)
    rstd = (grp.var(-1, unbiased=False) + eps).rsqrt()
    return y, mean, rstd


def ulp32(v):
    """spacing of fp32 at |v| (0 at 0)"""
    a = v.abs().double()
    _, e = torch.frexp(a)              # a = f 2^e, f in [0.5, 1)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 24), torch.zeros_like(a))


def floor32(shape, G, w, mean, rstd):
    """4 rstd |gamma_c| ulp32(|mean|) + 2e-6, broadcast to [N, C, 1, 1]"""
    N, C = shape[0], shape[1]
    per_group = (4.0 * rstd * ulp32(mean)).view(N, G, 1).expand(N, G, C // G).reshape(N, C)
    return (per_group * w.double().abs().view(1, C) + 2e-6).view(N, C, 1, 1)


def worst16(got, ref, dtype, k_rel=2.0, k_abs=4.0):
    """max over elements of |got - ref| / bar (<= 1 passes); non-finite output counts as infinitely bad"""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    u = ULP[dtype]
    return float(((got - ref).abs() / (k_rel * u * ref.abs() + k_abs * u)).max())


def worst32(got, ref, torch32, floor, G):
    """max over elements of |got - ref| / (2 max_group|torch32 - ref| + floor)"""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("nan")
    N, C = ref.shape[0], ref.shape[1]
    terr = (torch32.detach().cpu().double() - ref).abs().reshape(N, G, -1).amax(-1)          # [N, G]
    terr_c = terr.view(N, G, 1).expand(N, G, C // G).reshape(N, C).view(N, C, 1, 1)
    ratio = float(((got - ref).abs() / (2.0 * terr_c + floor)).max())
    return ratio, float(terr.max())


class Report:
    """collects (label, worst ratio) of one test, prints every figure, asserts at the end: a failing test still shows all of them"""

    def __init__(self, what):
        self.what, self.rows = what, []

    def add(self, label, ratio, note=""):
        self.rows.append((label, ratio))
        print(f"[norm-conditioning] {self.what} {label}: worst err/bar = {ratio:.3g} {note}")

    def check(self):
        bad = [(l, r) for l, r in self.rows if not r <= 1.0]
        assert not bad, f"{self.what}: over the bar (err/bar) {bad}"


def nchw(t):
    """logical NCHW values of a (possibly channels_last) tensor as a contiguous CPU tensor"""
    return t.detach().cpu().contiguous()


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a, b), "second launch differs from the first"
    return a


# ---- ed_groupnorm (NCHW 16-bit): plain and split path ------------------------------------------------------------------------------
GN_SHAPES = [((2, 320, 8, 8), 32), ((2, 64, 4, 2), 32), ((2, 128, 8, 8), 32), ((1, 16, 96, 96), 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,G", GN_SHAPES, ids=[_id(s) for s, _ in GN_SHAPES])
@pytest.mark.parametrize("dtype,case", typed_cases([F16, BF16]))
def test_groupnorm_nchw(dtype, case, shape, G):
    """cpg 10 / most threads idle / token layout / the split path ((C/G) HW = 73 728 > 65 536); class A also with the folded biases."""
    from elasticdiffusion_official_amd import ops
    N, C, H, W = shape
    x = make_input(case, dtype, shape, G)
    w, b = make_affine(C, dtype)
    if G == 2:
        assert ops._hip.lib().ed_groupnorm_workspace(N, C, H * W, G) > 0       # the split path is the one measured
    rep = Report(f"ed_groupnorm {NAME[dtype]} {_id(case)} {_id(shape)}")
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, _, _ = ref64(x, G, w, b, 1e-5, silu)
        t16 = F.group_norm(xd, G, wd, bd, 1e-5)
        t16 = F.silu(t16) if silu else t16
        for tokens in ((False, True) if (C // G) % 4 == 0 else (False,)):
            got = twice(lambda: ops.groupnorm(xd, wd, bd, G, 1e-5, silu=silu, tokens=tokens))
            r = ref.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else ref
            t = t16.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else t16
            rep.add(f"silu={silu} tokens={tokens}", worst16(got, r, dtype), f"(torch's 16-bit kernel: {worst16(t, r, dtype):.3g})")
    if case[0] == "A":      # statistics of the biased values: round16(round16(x + conv_bias) + chan_bias)
        g = torch.Generator().manual_seed(5)
        kb, cb = torch.randn(C, generator=g).to(dtype), torch.randn(N, C, generator=g).to(dtype)
        pre = (x + kb[None, :, None, None]) + cb[:, :, None, None]
        ref, _, _ = ref64(pre, G, w, b, 1e-5, True)
        got = twice(lambda: ops.groupnorm(xd, wd, bd, G, 1e-5, silu=True, chan_bias=cb.to(DEV), conv_bias=kb.to(DEV)))
        rep.add("silu=True folded biases", worst16(got, ref, dtype))
        assert torch.equal(got, ops.groupnorm(pre.to(DEV), wd, bd, G, 1e-5, silu=True))
    rep.check()


# ---- ed_groupnorm_nhwc (channels-last 16-bit) ----------------------------------------------------------------------------------------
NHWC_SHAPES = [(2, 320, 8, 8), (2, 256, 4, 2), (1, 320, 32, 32), (1, 2560, 8, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NHWC_SHAPES, ids=_id)
@pytest.mark.parametrize("dtype,case", typed_cases([F16, BF16]))
def test_groupnorm_nhwc(dtype, case, shape):
    """an 8-channel vector straddling two groups (cpg 10) / cpg 8 / several chunks per sample / two columns per thread (C = 2560)"""
    from elasticdiffusion_official_amd import ops
    N, C, H, W = shape
    G = 32
    x = make_input(case, dtype, shape, G)
    w, b = make_affine(C, dtype)
    rep = Report(f"ed_groupnorm_nhwc {NAME[dtype]} {_id(case)} {_id(shape)}")
    xd, wd, bd = cl(x), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, _, _ = ref64(x, G, w, b, 1e-5, silu)
        t16 = F.group_norm(x.to(DEV), G, wd, bd, 1e-5)
        t16 = F.silu(t16) if silu else t16
        got = twice(lambda: ops.groupnorm_nhwc(xd, wd, bd, G, 1e-5, silu=silu))
        rep.add(f"silu={silu}", worst16(nchw(got), ref, dtype), f"(torch's 16-bit kernel: {worst16(t16, ref, dtype):.3g})")
    if case[0] == "A":
        g = torch.Generator().manual_seed(5)
        kb, cb = torch.randn(C, generator=g).to(dtype), torch.randn(N, C, generator=g).to(dtype)
        pre = (x + kb[None, :, None, None]) + cb[:, :, None, None]
        ref, _, _ = ref64(pre, G, w, b, 1e-5, True)
        got = twice(lambda: ops.groupnorm_nhwc(xd, wd, bd, G, 1e-5, silu=True, chan_bias=cb.to(DEV), conv_bias=kb.to(DEV)))
        rep.add("silu=True folded biases", worst16(nchw(got), ref, dtype))
        assert torch.equal(got, ops.groupnorm_nhwc(cl(pre), wd, bd, G, 1e-5, silu=True))
    rep.check()


# ---- ed_groupnorm_nhwc_cat: the concatenation that is never written ------------------------------------------------------------------
CAT_SHAPES = [((2, 640, 320, 8, 8), 32), ((2, 64, 32, 7, 5), 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,G", CAT_SHAPES, ids=[_id(s) for s, _ in CAT_SHAPES])
@pytest.mark.parametrize("dtype,case", typed_cases([F16, BF16]))
def test_groupnorm_nhwc_cat(dtype, case, shape, G):
    """the seam inside a group (960 / 32 = 30 channels per group, seam at 21.33 groups) and G = 8; the two sources carry different
    offsets (class A: the second source has the mean negated and halved, so the seam group is bimodal)"""
    from elasticdiffusion_official_amd import ops
    N, C1, C2, H, W = shape
    C = C1 + C2
    x = make_input(case, dtype, (N, C, H, W), G)
    if case[0] == "A":
        other = make_input(("A", -0.5 * case[1], case[2]), dtype, (N, C, H, W), G, seed=1)
        x = torch.cat([x[:, :C1], other[:, C1:]], dim=1).contiguous()
    w, b = make_affine(C, dtype)
    rep = Report(f"ed_groupnorm_nhwc_cat {NAME[dtype]} {_id(case)} {_id(shape)}")
    x1, x2, wd, bd = cl(x[:, :C1]), cl(x[:, C1:]), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, _, _ = ref64(x, G, w, b, 1e-5, silu)
        t16 = F.group_norm(x.to(DEV), G, wd, bd, 1e-5)
        t16 = F.silu(t16) if silu else t16
        got = twice(lambda: ops.groupnorm_nhwc_cat(x1, x2, wd, bd, G, 1e-5, silu=silu))
        rep.add(f"silu={silu}", worst16(nchw(got), ref, dtype), f"(torch's 16-bit kernel: {worst16(t16, ref, dtype):.3g})")
        assert torch.equal(got, ops.groupnorm_nhwc(cl(x), wd, bd, G, 1e-5, silu=silu))
    rep.check()


# ---- ed_groupnorm_nhwc_s32: fp32 stream in, 16-bit out ---------------------------------------------------------------------------------
S32_SHAPES = [(2, 320, 8, 8), (1, 960, 16, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", S32_SHAPES, ids=_id)
@pytest.mark.parametrize("out_dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("case", CASES[F32], ids=_id)
def test_groupnorm_nhwc_s32(case, out_dtype, shape):
    """the fp32 input classes, judged at the 16-bit output's bar"""
    from elasticdiffusion_official_amd import ops
    N, C, H, W = shape
    G = 32
    x = make_input(case, F32, shape, G)
    w, b = make_affine(C, out_dtype)
    rep = Report(f"ed_groupnorm_nhwc_s32 {NAME[out_dtype]} {_id(case)} {_id(shape)}")
    xd, wd, bd = cl(x), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, _, _ = ref64(x, G, w, b, 1e-5, silu)
        t = F.group_norm(x.to(DEV), G, wd.float(), bd.float(), 1e-5)
        t = (F.silu(t) if silu else t).to(out_dtype)
        got = twice(lambda: ops.groupnorm_nhwc_s32(xd, wd, bd, G, 1e-5, silu=silu))
        assert got.dtype == out_dtype
        rep.add(f"silu={silu}", worst16(nchw(got), ref, out_dtype), f"(torch fp32, rounded once: {worst16(t, ref, out_dtype):.3g})")
    rep.check()


# ---- the fp32 kernels -------------------------------------------------------------------------------------------------------------------
def _bar32(x, G, w, b, eps, silu):
    ref, mean, rstd = ref64(x, G, w, b, eps, silu)
    t32 = F.group_norm(x.to(DEV), G, w.to(DEV), b.to(DEV), eps)
    t32 = F.silu(t32) if silu else t32
    return ref, t32, floor32(x.shape, G, w, mean, rstd)


F32_SHAPES = [((2, 128, 16, 16), 32), ((1, 8, 128, 160), 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,G", F32_SHAPES, ids=[_id(s) for s, _ in F32_SHAPES])
@pytest.mark.parametrize("case", CASES[F32], ids=_id)
def test_groupnorm_f32(case, shape, G):
    """1 K-element groups, and 81 920-element groups = two chunks per group, the second ragged"""
    from elasticdiffusion_official_amd import ops
    C = shape[1]
    x = make_input(case, F32, shape, G)
    w, b = make_affine(C, F32)
    rep = Report(f"ed_groupnorm_f32 {_id(case)} {_id(shape)}")
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, t32, floor = _bar32(x, G, w, b, 1e-6, silu)
        got = twice(lambda: ops.groupnorm_f32(xd, wd, bd, G, 1e-6, silu=silu))
        ratio, terr = worst32(got, ref, t32, floor, G)
        rep.add(f"silu={silu}", ratio, f"(torch fp32 max err {terr:.3g}, max err {float((got.cpu().double() - ref).abs().max()):.3g})")
    rep.check()


NHWC32_SHAPES = [(2, 128, 16, 16), (1, 128, 64, 64), (1, 2048, 4, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NHWC32_SHAPES, ids=_id)
@pytest.mark.parametrize("case", CASES[F32], ids=_id)
def test_groupnorm_nhwc_f32_plain_and_split(case, shape):
    """one chunk / many chunks / two columns per thread; split=True is judged as hi + lo, and keeps hi == fp16(y), hi == hi2"""
    from elasticdiffusion_official_amd import ops
    N, C, H, W = shape
    G = 32
    x = make_input(case, F32, shape, G)
    w, b = make_affine(C, F32)
    rep = Report(f"ed_groupnorm_nhwc_f32 {_id(case)} {_id(shape)}")
    xd, wd, bd = cl(x), w.to(DEV), b.to(DEV)
    for silu in (True, False):
        ref, t32, floor = _bar32(x, G, w, b, 1e-6, silu)
        y = twice(lambda: ops.groupnorm_nhwc_f32(xd, wd, bd, G, 1e-6, silu=silu))
        ratio, terr = worst32(nchw(y), ref, t32, floor, G)
        rep.add(f"silu={silu} plain", ratio, f"(torch fp32 max err {terr:.3g}, max err {float((nchw(y).double() - ref).abs().max()):.3g})")
        s = twice(lambda: ops.groupnorm_nhwc_f32(xd, wd, bd, G, 1e-6, silu=silu, split=True))
        hi, lo, hi2 = s[:, :C], s[:, C:2 * C], s[:, 2 * C:]
        assert torch.equal(hi, hi2) and torch.equal(hi, y.half())
        ratio, _ = worst32(nchw(hi).double() + nchw(lo).double(), ref, t32, floor, G)
        rep.add(f"silu={silu} hi+lo", ratio)
    rep.check()


# ---- controls: the LayerNorm kernels are two-pass on registers and pass unchanged ----------------------------------------------------
LN_SHAPES = [(5, 320), (77, 2048)]


def _ln_rows(m, s, shape, seed):
    g = torch.Generator().manual_seed(31 * seed + shape[1])
    return m + s * torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LN_SHAPES, ids=_id)
@pytest.mark.parametrize("dtype,case", [pytest.param(dt, c, id=f"{NAME[dt]}-{_id(c)}") for dt in (F16, BF16) for c in CLASS_A[dt]])
def test_layernorm_controls(dtype, case, shape):
    """class A along the row.  ed_layernorm / ed_add_layernorm on 16-bit rows; ed_layernorm_s32 / ed_add_layernorm_s32 on fp32 rows with
    the OUTPUT type's (m, s) pairs: the bar is in ulps of the 16-bit output, and a mean held in fp32 is already uncertain by
    ulp32(m) / 2 -- 5e-4 s at m / s = 1e4, a whole fp16 ulp of the normalised value -- so the fp32 pairs beyond m / s = 1e3 would ask
    of these kernels what no fp32 LayerNorm delivers."""
    from elasticdiffusion_official_amd import ops
    M, D = shape
    _, m, s = case
    w, b = make_affine(D, dtype)
    wd, bd = w.to(DEV), b.to(DEV)
    rep = Report(f"layernorm {NAME[dtype]} {_id(case)} {_id(shape)}")

    def ref_of(v):
        return F.layer_norm(v.double(), (D,), w.double(), b.double(), 1e-5)

    x = _ln_rows(m, s, shape, 1).to(dtype)
    got = twice(lambda: ops.layernorm(x.to(DEV), wd, bd, 1e-5))
    t16 = F.layer_norm(x.to(DEV), (D,), wd, bd, 1e-5)
    rep.add("ed_layernorm", worst16(got, ref_of(x), dtype, 1.0, 2.0), f"(torch's 16-bit kernel: {worst16(t16, ref_of(x), dtype, 1.0, 2.0):.3g})")
    # a + b with a the small branch result and b the offset stream; the sum is rounded to 16 bit by the kernel as by torch
    a = _ln_rows(0.0, 0.5, shape, 2).to(dtype)
    sm, ln = ops.add_layernorm(a.to(DEV), x.to(DEV), wd, bd, 1e-5)
    assert torch.equal(sm.cpu(), a + x)
    rep.add("ed_add_layernorm", worst16(ln, ref_of(a + x), dtype, 1.0, 2.0))
    assert torch.equal(ln, ops.add_layernorm(a.to(DEV), x.to(DEV), wd, bd, 1e-5)[1])
    x32 = _ln_rows(m, s, shape, 3).float()
    got = twice(lambda: ops.layernorm_s32(x32.to(DEV), wd, bd, 1e-5))
    rep.add("ed_layernorm_s32", worst16(got, ref_of(x32), dtype, 1.0, 2.0))
    sm, ln = ops.add_layernorm_s32(a.to(DEV), x32.to(DEV), wd, bd, 1e-5)
    assert torch.equal(sm.cpu(), a.float() + x32)
    rep.add("ed_add_layernorm_s32", worst16(ln, ref_of(a.float() + x32), dtype, 1.0, 2.0))
    assert torch.equal(ln, ops.add_layernorm_s32(a.to(DEV), x32.to(DEV), wd, bd, 1e-5)[1])
    rep.check()


# ---- no GPU: the bars are attainable ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,case", typed_cases([F16, BF16]))
def test_the_16bit_bar_is_attainable(dtype, case):
    """torch's CPU fp32 GroupNorm (+SiLU) on the 16-bit inputs, rounded once to the output type, sits inside the 16-bit bar on every class
    (cpg 10 and the 73 728-element groups of the split path)."""
    for shape, G in [((2, 320, 8, 8), 32), ((1, 16, 96, 96), 2)]:
        x = make_input(case, dtype, shape, G)
        w, b = make_affine(shape[1], dtype)
        for silu in (True, False):
            ref, _, _ = ref64(x, G, w, b, 1e-5, silu)
            y = F.group_norm(x.float(), G, w.float(), b.float(), 1e-5)
            y = (F.silu(y) if silu else y).to(dtype)
            r = worst16(y, ref, dtype)
            print(f"[norm-conditioning] ideal {NAME[dtype]} {_id(case)} {_id(shape)} silu={silu}: worst err/bar = {r:.3g}")
            assert r <= 1.0, (shape, silu, r)


@pytest.mark.parametrize("out_dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("case", CASES[F32], ids=_id)
def test_the_16bit_bar_is_attainable_from_an_fp32_stream(case, out_dtype):
    """fp32 inputs, 16-bit output (ed_groupnorm_nhwc_s32's cases).  The ideal here is plain fp32 arithmetic on correctly rounded
    statistics in the centred form, ((x - mean) rstd) gamma + beta, rounded once.  torch's CPU fp32 kernel is printed beside it and NOT
    asserted: it misses the fp16 bar at m / s = 1e4 and on class C (measured 1.01 ... 2.6 of the bar) through its own mean error and the
    rounding of beta - a mean, an fp32 number of the size of a mean / s.  The folded form a x + (beta - a mean) misses class C as well
    even with exact statistics (1.1 of the bar), which is why the kernel applies the centred form on the fp32 stream."""
    for shape in [(2, 320, 8, 8), (1, 960, 16, 16)]:
        N, C, G = shape[0], shape[1], 32
        x = make_input(case, F32, shape, G)
        w, b = make_affine(C, out_dtype)
        for silu in (True, False):
            ref, mean, rstd = ref64(x, G, w, b, 1e-5, silu)
            m32 = mean.float().view(N, G, 1).expand(N, G, C // G).reshape(N, C, 1, 1)
            r32 = rstd.float().view(N, G, 1).expand(N, G, C // G).reshape(N, C, 1, 1)
            y = ((x - m32) * r32) * w.float().view(1, C, 1, 1) + b.float().view(1, C, 1, 1)
            t = F.group_norm(x, G, w.float(), b.float(), 1e-5)
            if silu:
                y, t = F.silu(y), F.silu(t)
            r, rt = worst16(y.to(out_dtype), ref, out_dtype), worst16(t.to(out_dtype), ref, out_dtype)
            print(f"[norm-conditioning] ideal fp32->{NAME[out_dtype]} {_id(case)} {_id(shape)} silu={silu}: worst err/bar = {r:.3g} "
                  f"(torch CPU fp32: {rt:.3g})")
            assert r <= 1.0, (shape, silu, r)


@pytest.mark.parametrize("case", CASES[F32], ids=_id)
def test_the_fp32_floor_is_attainable(case):
    """torch's CPU fp32 GroupNorm (+SiLU) against the floor ALONE (no allowance for torch's own error: it is the implementation judged here),
    on 1 K-element and 81 920-element groups"""
    for shape, G in [((2, 128, 16, 16), 32), ((1, 8, 128, 160), 2)]:
        x = make_input(case, F32, shape, G)
        w, b = make_affine(shape[1], F32)
        for silu in (True, False):
            ref, mean, rstd = ref64(x, G, w, b, 1e-6, silu)
            y = F.group_norm(x, G, w, b, 1e-6)
            y = F.silu(y) if silu else y
            r = float(((y.double() - ref).abs() / floor32(shape, G, w, mean, rstd)).max())
            print(f"[norm-conditioning] ideal fp32 {_id(case)} {_id(shape)} silu={silu}: worst err/floor = {r:.3g}")
            assert r <= 1.0, (shape, silu, r)


def test_layernorm_bar_is_attainable():
    """torch's CPU fp32 LayerNorm on class A rows, rounded once, inside 1 ulp |ref| + 2 ulp -- for 16-bit rows and for fp32 rows with the
    output type's pairs (see test_layernorm_controls)"""
    for dtype in (F16, BF16):
        for _, m, s in CLASS_A[dtype]:
            for shape in LN_SHAPES:
                w, b = make_affine(shape[1], dtype)
                for x in (_ln_rows(m, s, shape, 1).to(dtype).float(), _ln_rows(m, s, shape, 3).float()):
                    ref = F.layer_norm(x.double(), (shape[1],), w.double(), b.double(), 1e-5)
                    y = F.layer_norm(x, (shape[1],), w.float(), b.float(), 1e-5).to(dtype)
                    assert worst16(y, ref, dtype, 1.0, 2.0) <= 1.0, (dtype, m, s, shape)
