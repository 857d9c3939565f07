"""-m gpu: the 16-bit and split-fp32 paths of models.py against the independent fp64 statement of the same forwards (tests/sd_spec.py).

Each case puts one dispatch path of models.py to work on a small shape, checks through ops.TIMER that the kernels of that path were
really launched, and compares with the spec in fp64 on the CPU.  The yardstick is independent of the code under test: the SAME spec
executed on the GPU in the same dtype with plain torch ops (``e_spec``).  Bar: e_prod <= 1.5 e_spec + floor, floor = 2 ulp of the
16-bit output dtype (ulp as in test_unet_kernels.py: 2^-11 fp16, 2^-8 bf16; relative to max |ref|), 2e-6 for fp32 outputs.  Blocks: per-element maximum of |got - ref| / max |ref|; whole
forwards: relative L2.  Parameters are randomised (no trivial affine, 0.2-sized biases: a lost bias is an error of order 10 %) and
rounded to the dtype BEFORE both sides read them.  Every launch sequence runs twice and must be bit-identical (``judge`` says how for the
cases on the library's convolutions).  The last section runs the same blocks and forwards on the fp32 residual stream of a 16-bit model
(``residual_fp32``: the dispatch tree the SD 1.x / 2.x family takes by default) under the same bar.
"""
import functools

import pytest
import torch

from tests import sd_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
HALF = [torch.float16, torch.bfloat16]
FACTOR = 1.5
ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture
def mods():
    from elasticdiffusion_official_amd import models as M, ops
    return M, ops


def _admit(monkeypatch, ops):
    """small grids run the GEMM kernels: every shape a kernel TAKES counts as one it wins on (restored by monkeypatch)"""
    monkeypatch.setattr(ops, "GEMM_MIN_BLOCKS", 1)
    monkeypatch.setattr(ops, "conv3x3_wins", ops.conv3x3_ok)
    monkeypatch.setattr(ops, "linear_wins", ops.linear_ok)
    monkeypatch.setattr(ops, "geglu_gemm_wins", ops.geglu_gemm_ok)


@pytest.fixture
def admit(monkeypatch, mods):
    _admit(monkeypatch, mods[1])


# ---- parameters, inputs, judgement ------------------------------------------------------------------------------------------------
def _rounded(module, seed, dtype):
    """seeded init + randomise, every value rounded to ``dtype``: the ONE set of values both sides read"""
    from elasticdiffusion_official_amd import models as M
    M._seeded_init(module, seed)
    return {k: v.to(dtype) for k, v in S.randomise(module.state_dict(), seed).items()}


def _load(module, sd, dtype, cl=False):
    module.load_state_dict(sd)
    module = module.to(DEV, dtype).eval().requires_grad_(False)
    return module.to(memory_format=CL) if cl else module


def _sides(sd, prefix="blk."):
    """(fp64 CPU state dict, same values on the GPU in their dtype) under the spec's name prefix"""
    return {prefix + k: v.double() for k, v in sd.items()}, {prefix + k: v.to(DEV) for k, v in sd.items()}


def _x(seed, shape, dtype, scale=1.0):
    """-> (fp64 CPU, ``dtype`` GPU) of the same rounded values"""
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)
    return x.double(), x.to(DEV)


def _listed(t):
    return list(t) if isinstance(t, (list, tuple)) else [t]


def _max_err(got, ref):
    return max(float((g.double().cpu() - r).abs().max() / r.abs().max()) for g, r in zip(_listed(got), _listed(ref)))


def _twice_on_deterministic_libraries(run):
    """Two runs with the library asked for deterministic solvers.  Only for cases that reach MIOpen's convolutions: its default choice
    for several of these small shapes (3 x 16 x 16 pixels: 3x3 from 256 or 384 channels, 1x1 at 256, fp32 3x3 at most widths) gives six
    different results in six calls of F.conv2d alone, which would drown the race screen of the project's kernels."""
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return run(), run()
    finally:
        torch.backends.cudnn.deterministic = keep


def judge(ops, name, run, run_spec, ref, expect=(), forbid=(), whole=False, floor=None, library_conv=False):
    """run the product (kernels launched? e_prod), run it again (bit-identical?), the spec once on the GPU (e_spec), and hold e_prod
    against e_spec.  Default settings throughout, and the second run is compared with the judged one -- except where the case reaches the
    library's convolutions (``library_conv``): there the judged run keeps the defaults and a pair of runs on deterministic solvers
    is compared with each other and held to the same bar."""
    with torch.no_grad():
        ops.TIMER.start()
        try:
            got = run()
        finally:
            stats = ops.TIMER.stop()
        first, again = _twice_on_deterministic_libraries(run) if library_conv else (got, run())
        spec = run_spec()
        torch.cuda.synchronize()
    launched = set(stats)
    assert set(expect) <= launched, (name, "missing", sorted(set(expect) - launched), "launched", sorted(launched))
    assert not set(forbid) & launched, (name, "unexpected", sorted(set(forbid) & launched))
    for a, b in zip(_listed(first), _listed(again)):
        assert torch.equal(a, b), (name, "two runs differ")
    for g, r in zip(_listed(got), _listed(ref)):
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), name
    out_dtype = _listed(got)[0].dtype
    if floor is None:
        floor = 2e-6 if out_dtype == torch.float32 else 2 * ULP[out_dtype]
    err = (lambda a: S.rel_l2(_listed(a), _listed(ref))) if whole else (lambda a: _max_err(a, ref))
    e_prod, e_spec = err(got), err(spec)
    print(f"{name}: e_prod {e_prod:.3e} e_spec {e_spec:.3e} ratio {e_prod / max(e_spec, 1e-300):.2f} "
          f"(bar {FACTOR} e_spec + {floor:.1e}) kernels {' '.join(sorted(n for n in launched))}")
    assert e_prod <= FACTOR * e_spec + floor, (name, e_prod, e_spec)
    if library_conv:
        assert err(first) <= FACTOR * e_spec + floor, (name, "deterministic solvers", err(first), e_spec)
    return stats


def _name(dtype):
    return str(dtype).replace("torch.", "")


# ---- ResnetBlock2D ----------------------------------------------------------------------------------------------------------------
TEMB = 256
RES_HW = (16, 16)


@functools.lru_cache(maxsize=None)
def _resnet_case(cin, cout, dtype, temb=TEMB, eps=1e-5, hw=RES_HW):
    from elasticdiffusion_official_amd import models as M
    sd = _rounded(M.ResnetBlock2D(cin, cout, temb, eps=eps), 100 + cin + cout, dtype)
    ref_sd, gpu_sd = _sides(sd)
    x64, x = _x(1, (3, cin) + hw, dtype)
    e64, emb = _x(2, (3, temb), dtype) if temb else (None, None)
    with torch.no_grad():
        ref = S.resnet(ref_sd, "blk", x64, e64, eps)
    return sd, gpu_sd, x, emb, ref


def _resnet(M, cin, cout, dtype, cl, temb=TEMB, eps=1e-5):
    sd, gpu_sd, x, emb, ref = _resnet_case(cin, cout, dtype, temb, eps)
    blk = _load(M.ResnetBlock2D(cin, cout, temb, eps=eps), sd, dtype, cl)
    xin = x.contiguous(memory_format=CL) if cl else x
    return blk, xin, emb, ref, (lambda: S.resnet(gpu_sd, "blk", x, emb, eps))


RES_SHAPES = [(256, 256), (256, 320)]


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_nchw_fused(cin, cout, dtype, mods):
    """NCHW: bias-free convolutions, conv1's bias + the time embedding folded into ed_groupnorm, conv2's (+ the shortcut's) into
    ed_bias_residual_add"""
    M, ops = mods
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=False)
    judge(ops, f"ResnetBlock2D NCHW fused {cin}->{cout} {_name(dtype)}", lambda: blk(x, emb), spec, ref,
          expect=("ed_groupnorm", "ed_bias_residual_add"), forbid=("ed_groupnorm_nhwc", "ed_conv3x3_nhwc"), library_conv=True)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_channels_last_library_convolutions(cin, cout, dtype, mods, monkeypatch):
    """channels-last, MIOpen's convolutions: both biases folded into ed_groupnorm_nhwc, the closing ed_bias_residual_add, the 1x1
    shortcut as a linear over the token view"""
    M, ops = mods
    monkeypatch.setattr(M, "HIP_CONV3X3", False)
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=True)
    judge(ops, f"ResnetBlock2D channels-last, library convolutions {cin}->{cout} {_name(dtype)}", lambda: blk(x, emb), spec, ref,
          expect=("ed_groupnorm_nhwc", "ed_bias_residual_add"), forbid=("ed_conv3x3_nhwc", "ed_groupnorm"), library_conv=True)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_channels_last_hip_convolutions(cin, cout, dtype, mods, admit):
    """channels-last, both convolutions ed_conv3x3_nhwc: bias + per-sample time embedding in conv1's epilogue, bias + residual in conv2's"""
    M, ops = mods
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=True)
    stats = judge(ops, f"ResnetBlock2D channels-last, ed_conv3x3_nhwc {cin}->{cout} {_name(dtype)}", lambda: blk(x, emb), spec, ref,
                  expect=("ed_groupnorm_nhwc", "ed_conv3x3_nhwc") + (("ed_linear",) if cin != cout else ()),
                  forbid=("ed_bias_residual_add", "ed_groupnorm"))
    assert stats["ed_conv3x3_nhwc"][0] == 2 and stats["ed_groupnorm_nhwc"][0] == 2


@functools.lru_cache(maxsize=None)
def _cat_case(c1, c2, cout, dtype):
    from elasticdiffusion_official_amd import models as M
    sd = _rounded(M.ResnetBlock2D(c1 + c2, cout, TEMB), 200 + cout, dtype)
    ref_sd, gpu_sd = _sides(sd)
    (x64, x), (s64, skip), (e64, emb) = _x(1, (3, c1) + RES_HW, dtype), _x(3, (3, c2) + RES_HW, dtype, 0.7), _x(2, (3, TEMB), dtype)
    with torch.no_grad():
        ref = S.resnet_cat(ref_sd, "blk", x64, s64, e64)
    return sd, gpu_sd, x, skip, emb, ref


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("shortcut", ["ed_linear", "addmm"])
@pytest.mark.parametrize("cout", [256, 320])
def test_resnet_on_a_concatenation_that_is_never_written(cout, shortcut, dtype, mods, admit, monkeypatch):
    """forward_cat: ed_groupnorm_nhwc_cat reads [x | skip] in place, the 1x1 shortcut is split along K -- its second half accumulates
    through ed_linear's residual epilogue, or through the library's addmm"""
    M, ops = mods
    c1, c2 = 256, 128
    if shortcut == "addmm":
        monkeypatch.setattr(ops, "linear_wins", lambda *a: False)
    sd, gpu_sd, x, skip, emb, ref = _cat_case(c1, c2, cout, dtype)
    blk = _load(M.ResnetBlock2D(c1 + c2, cout, TEMB), sd, dtype, cl=True)
    xc, sc = x.contiguous(memory_format=CL), skip.contiguous(memory_format=CL)
    judge(ops, f"ResnetBlock2D.forward_cat {c1}+{c2}->{cout} shortcut via {shortcut} {_name(dtype)}", lambda: blk.forward_cat(xc, sc, emb),
          lambda: S.resnet_cat(gpu_sd, "blk", x, skip, emb), ref, expect=("ed_groupnorm_nhwc_cat", "ed_groupnorm_nhwc", "ed_conv3x3_nhwc"),
          forbid=("ed_bias_residual_add",) + (("ed_linear",) if shortcut == "addmm" else ()))
    if shortcut == "ed_linear":
        with torch.no_grad():
            ops.TIMER.start()
            blk.forward_cat(xc, sc, emb)
            assert ops.TIMER.stop()["ed_linear"][0] == 2         # W_1 x, then W_2 skip onto it


@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_on_the_fp32_residual_stream(cin, cout, mods, admit):
    """fp16 block on an fp32 stream (residual_fp32): ed_groupnorm_nhwc_s32 reads the stream, conv2 closes through the fp32-output
    epilogue (ed_conv3x3_nhwc_f32out) -- the branch is never rounded to 16 bits, so it must not lose to the all-fp16 sequence"""
    M, ops = mods
    dtype = torch.float16
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=True)
    x32 = x.float().contiguous(memory_format=CL)                # the same (fp16-representable) values, carried as the fp32 stream
    judge(ops, f"ResnetBlock2D fp32 stream {cin}->{cout} float16", lambda: blk(x32, emb), spec, ref,
          expect=("ed_groupnorm_nhwc_s32", "ed_groupnorm_nhwc", "ed_conv3x3_nhwc", "ed_conv3x3_nhwc_f32out"),
          forbid=("ed_bias_residual_add",))
    with torch.no_grad():
        assert blk(x32, emb).dtype == torch.float32


@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_resnet_with_small_groups_falls_back_to_torch(dtype, mods, admit):
    """64 -> 128 channels, 2 and 4 channels per group: no channels-last kernel takes them, the block runs on torch ops and still matches"""
    M, ops = mods
    blk, x, emb, ref, spec = _resnet(M, 64, 128, dtype, cl=True)
    stats = judge(ops, f"ResnetBlock2D 64->128 (C/G < 8) {_name(dtype)}", lambda: blk(x, emb), spec, ref, library_conv=True)
    assert not stats, sorted(stats)


# ---- Transformer2DModel / BasicTransformerBlock / Attention ----------------------------------------------------------------------------
CROSS = 64
TR_HW = (16, 16)


@functools.lru_cache(maxsize=None)
def _transformer_case(C, heads, linear, dtype):
    from elasticdiffusion_official_amd import models as M
    sd = _rounded(M.Transformer2DModel(C, heads, 2, CROSS, linear), 300 + C + linear, dtype)
    ref_sd, gpu_sd = _sides(sd)
    (x64, x), (c64, ctx) = _x(1, (3, C) + TR_HW, dtype), _x(2, (3, S.CONTEXT_TOKENS, CROSS), dtype, S.CONTEXT_SCALE)
    with torch.no_grad():
        ref = S.transformer_2d(ref_sd, "blk", x64, c64, heads, 2, linear)
    return sd, gpu_sd, x, ctx, ref


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("mode", ["nchw", "nchw-kv", "channels-last", "channels-last-residual-linear"])
@pytest.mark.parametrize("linear", [True, False], ids=["linear-proj", "conv-proj"])
@pytest.mark.parametrize("C,heads", [(256, 4), (320, 8)], ids=["hd64", "hd40"])
def test_transformer_2d(C, heads, linear, mode, dtype, mods, monkeypatch):
    """Transformer2DModel, depth 2 (the second block's norm1 runs fused with the first block's pending add):
    nchw: default switches -- ed_groupnorm, ed_layernorm / ed_add_layernorm, ed_flash_attention, ed_geglu, ed_tokens_add_nchw;
    nchw-kv: the same with k|v of every cross-attention precomputed (cross_attention_kv);
    channels-last: GEMM kernels admitted -- ed_groupnorm_nhwc, ed_linear (with proj_out's closing add in its epilogue), ed_geglu_gemm;
    channels-last-residual-linear: FUSED_RESIDUAL_LINEAR -- every `x + branch` inside ed_linear, plain ed_layernorm only."""
    M, ops = mods
    cl = mode.startswith("channels-last")
    if cl:
        _admit(monkeypatch, ops)
        monkeypatch.setattr(M, "FUSED_RESIDUAL_LINEAR", mode.endswith("residual-linear"))
    sd, gpu_sd, x, ctx, ref = _transformer_case(C, heads, linear, dtype)
    m = _load(M.Transformer2DModel(C, heads, 2, CROSS, linear), sd, dtype, cl)
    xin = x.contiguous(memory_format=CL) if cl else x
    kv = None
    if mode == "nchw-kv":
        with torch.no_grad():
            kv = {id(b.attn2): b.attn2.project_kv(ctx) for b in m.transformer_blocks}
    cpg = C // 32
    if cl:
        expect = {"ed_groupnorm_nhwc", "ed_layernorm", "ed_flash_attention", "ed_geglu_gemm", "ed_linear"}
        forbid = {"ed_tokens_add_nchw", "ed_geglu", "ed_groupnorm"}
        if mode.endswith("residual-linear"):
            forbid.add("ed_add_layernorm")
        else:
            expect.add("ed_add_layernorm")
    else:
        expect = {"ed_layernorm", "ed_add_layernorm", "ed_flash_attention", "ed_geglu"}
        forbid = {"ed_linear", "ed_geglu_gemm", "ed_groupnorm_nhwc"}
        if not linear or cpg % 4 == 0:         # (the token-layout output of ed_groupnorm wants 4 | C / G: 320 channels take torch's)
            expect.add("ed_groupnorm")
        if linear:
            expect.add("ed_tokens_add_nchw")
        else:
            forbid.add("ed_tokens_add_nchw")
    stats = judge(ops, f"Transformer2DModel C={C} heads={heads} {'linear' if linear else 'conv'} projection, {mode}, {_name(dtype)}",
                  lambda: m(xin, ctx, kv), lambda: S.transformer_2d(gpu_sd, "blk", x, ctx, heads, 2, linear), ref, expect=expect, forbid=forbid,
                  library_conv=not linear)         # (proj_in / proj_out as the library's 1x1 convolutions)
    if mode.startswith("nchw"):      # per block: norm2 and norm3 fused with the add in front of them; block 2's norm1 with block 1's pending add
        assert stats["ed_add_layernorm"][0] == 5 and stats["ed_layernorm"][0] == 1, stats
    if mode == "channels-last-residual-linear":
        assert stats["ed_layernorm"][0] == 6, stats


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("C,heads,N,prescaled", [(128, 2, 256, True), (128, 2, 100, False), (320, 8, 256, False)],
                         ids=["hd64-256tokens-exponent-domain", "hd64-100tokens-natural", "hd40-256tokens-natural"])
def test_self_attention_with_the_scale_folded_into_the_query_weights(C, heads, N, prescaled, dtype, mods, monkeypatch):
    """Attention._fused_weight: where ops.flash_prescale returns a factor (pipelined kernel, head_dim 64, >= 128 keys) softmax scale *
    log2 e lives in the query rows of the fused q|k|v weight and the kernel works in the exponent domain; elsewhere q stays natural"""
    M, ops = mods
    monkeypatch.setattr(ops, "FLASH_EXP2", True)
    assert (ops.flash_prescale(N, N, 3 * C) is not None) == prescaled or C // heads != 64
    sd = _rounded(M.Attention(C, heads, C // heads), 400 + C + N, dtype)
    ref_sd, gpu_sd = _sides(sd)
    x64, x = _x(5, (3, N, C), dtype, 2.0)
    with torch.no_grad():
        ref = S.attention(ref_sd, "blk", x64, None, heads)
    m = _load(M.Attention(C, heads, C // heads), sd, dtype)
    judge(ops, f"self-attention C={C} heads={heads} tokens={N} {_name(dtype)}", lambda: m(x), lambda: S.attention(gpu_sd, "blk", x, None, heads),
          ref, expect=("ed_flash_attention",))
    folded = [k for k in m.__dict__.get("_derived", {}) if isinstance(k, tuple) and k[1] is not None]
    assert bool(folded) == prescaled, folded


# ---- samplers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("C", [128, 320])
def test_samplers_on_the_convolution_main_loop(C, dtype, mods, admit, monkeypatch):
    """Downsample2D as ed_conv3x3_nhwc_s2 (HIP_DOWNSAMPLE_CONV), Upsample2D as ONE ed_conv3x3_nhwc_up2x"""
    M, ops = mods
    monkeypatch.setattr(ops, "gemm_rows_mode", lambda *a: False)     # (neither kernel has a 128-row instantiation: the policy's mirror only)
    monkeypatch.setattr(M, "HIP_DOWNSAMPLE_CONV", True)
    for kind, ctor, hw, fn, kernel in (("Downsample2D", lambda: M.Downsample2D(C), (32, 32), S.downsample, "ed_conv3x3_nhwc_s2"),
                                       ("Upsample2D", lambda: M.Upsample2D(C), (16, 16), S.upsample, "ed_conv3x3_nhwc_up2x")):
        sd = _rounded(ctor(), 500 + C, dtype)
        ref_sd, gpu_sd = _sides(sd)
        x64, x = _x(7, (3, C) + hw, dtype)
        with torch.no_grad():
            ref = fn(ref_sd, "blk", x64)
        m = _load(ctor(), sd, dtype, cl=True)
        xc = x.contiguous(memory_format=CL)
        judge(ops, f"{kind}({C}) {_name(dtype)}", lambda: m(xc), lambda: fn(gpu_sd, "blk", x), ref, expect=(kernel,))


# ---- whole forwards ---------------------------------------------------------------------------------------------------------------
NET_HW = (16, 16)


def _to_dev(inp, dtype):
    added = None if inp["added"] is None else dict(text_embeds=inp["added"]["text_embeds"].to(DEV, dtype), time_ids=inp["added"]["time_ids"].to(DEV))
    return dict(sample=inp["sample"].to(DEV, dtype), t=inp["t"].to(DEV), context=inp["context"].to(DEV, dtype), added=added,
                cond=inp["cond"].to(DEV, dtype))


@functools.lru_cache(maxsize=None)
def _net_case(fam, dtype):
    """rounded parameters and inputs of the small UNet + ControlNet of ``fam`` and the spec's fp64 outputs (computed once per dtype)"""
    from elasticdiffusion_official_amd import models as M
    cfg = M.SMALL_UNET_CONFIGS[fam]
    usd, csd = _rounded(M.UNet2DConditionModel(**cfg), 21, dtype), _rounded(M.ControlNetModel(cfg), 22, dtype)
    raw = S.unet_inputs(cfg, NET_HW, seed=7)
    i64 = {k: (v.to(dtype).double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in raw.items()}
    if raw["added"] is not None:
        i64["added"] = dict(text_embeds=raw["added"]["text_embeds"].to(dtype).double(), time_ids=raw["added"]["time_ids"])
    u64, c64 = _sides(usd, "")[0], _sides(csd, "")[0]
    a = (i64["sample"], i64["t"], i64["context"])
    with torch.no_grad():
        down, mid = S.controlnet_forward(c64, cfg, *a, i64["cond"], S.CONDITIONING_SCALE, i64["added"])
        res = [d.to(dtype) for d in down], mid.to(dtype)        # the residuals BOTH sides feed the UNet, rounded like every input
        ref = {"controlnet": list(down) + [mid],
               "per-row": S.unet_forward(u64, cfg, *a, i64["added"]),
               "scalar": S.unet_forward(u64, cfg, i64["sample"], i64["t"][0], i64["context"], i64["added"]),
               "residuals": S.unet_forward(u64, cfg, *a, i64["added"], [d.double() for d in res[0]], res[1].double())}
    return cfg, usd, csd, i64, res, ref


def _whole_expect(M):
    return {"ed_groupnorm_nhwc" if M.CHANNELS_LAST else "ed_groupnorm", "ed_layernorm", "ed_add_layernorm", "ed_flash_attention"}


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("fam", ["sd15", "sdxl"])
def test_unet_forward(fam, dtype, mods):
    """the small UNet, default switches: per-row timesteps, a scalar timestep, and with ControlNet residuals"""
    M, ops = mods
    cfg, usd, _, i64, res, ref = _net_case(fam, dtype)
    m = _load(M.UNet2DConditionModel(**cfg), usd, dtype, cl=M.CHANNELS_LAST)
    gpu_sd = _sides(usd, "")[1]
    i = _to_dev(i64, dtype)
    down, mid = [d.to(DEV) for d in res[0]], res[1].to(DEV)
    for case, t, extra, sx in (("per-row", i["t"], {}, ()), ("scalar", i["t"][0], {}, ()),
                               ("residuals", i["t"], dict(down_block_additional_residuals=down, mid_block_additional_residual=mid), (down, mid))):
        judge(ops, f"{fam} UNet {_name(dtype)}, {case}",
              lambda: m(i["sample"], t, encoder_hidden_states=i["context"], added_cond_kwargs=i["added"], **extra).sample,
              lambda: S.unet_forward(gpu_sd, cfg, i["sample"], t, i["context"], i["added"], *sx), ref[case], expect=_whole_expect(M), whole=True, library_conv=True)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("fam", ["sd15", "sdxl"])
def test_controlnet_forward(fam, dtype, mods):
    M, ops = mods
    cfg, _, csd, i64, _, ref = _net_case(fam, dtype)
    m = _load(M.ControlNetModel(cfg), csd, dtype, cl=M.CHANNELS_LAST)
    gpu_sd = _sides(csd, "")[1]
    i = _to_dev(i64, dtype)

    def run():
        d, mid = m(i["sample"], i["t"], encoder_hidden_states=i["context"], controlnet_cond=i["cond"], conditioning_scale=S.CONDITIONING_SCALE,
                   added_cond_kwargs=i["added"])
        return list(d) + [mid]

    def spec():
        d, mid = S.controlnet_forward(gpu_sd, cfg, i["sample"], i["t"], i["context"], i["cond"], S.CONDITIONING_SCALE, i["added"])
        return list(d) + [mid]
    judge(ops, f"{fam} ControlNet {_name(dtype)}", run, spec, ref["controlnet"], expect=_whole_expect(M), whole=True, library_conv=True)


# ---- the fp32 VAE ----------------------------------------------------------------------------------------------------------------
F32 = torch.float32


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (128, 256)])
def test_vae_resnet_block(cin, cout, mods):
    """the fp32 VAE block.  The split-operand path (GroupNorm writes the fp16 (hi, lo) operand, both convolutions on the MFMA pipe with an
    fp32 epilogue) wants 4 | C / G on both norms: 128 channels and up.  A 64-channel norm (2 per group) keeps the block on the library's
    fp32 convolutions with ed_groupnorm_f32 -- the small VAE's case -- and must match just the same."""
    M, ops = mods
    blk, x, _, ref, spec = _resnet(M, cin, cout, F32, cl=False, temb=None, eps=1e-6)
    split = cin >= 128
    assert M._vae_split_ok(x, blk) == split
    judge(ops, f"VAE ResnetBlock2D {cin}->{cout} {'split operands' if split else 'library convolutions'}", lambda: blk(x), spec, ref,
          expect=("ed_groupnorm_nhwc_f32", "ed_conv3x3_nhwc_f32out") if split else ("ed_groupnorm_f32",),
          forbid=() if split else ("ed_conv3x3_nhwc_f32out",), library_conv=not split)


@pytest.mark.parametrize("scale", [1.0, 3.0e4], ids=["unit", "beyond-fp16-range"])
@pytest.mark.parametrize("kind", ["up", "down"])
def test_vae_samplers_on_split_operands(kind, scale, mods):
    """the raw stream is split with a per-tensor power-of-two scale: exact over the fp32 range, also where |x| exceeds fp16's 65504"""
    M, ops = mods
    C = 64
    ctor, fn, kernel = ((lambda: M.Upsample2D(C, vae=True)), S.vae_upsample, "ed_conv3x3_nhwc_f32out") if kind == "up" else \
        ((lambda: M.Downsample2D(C, padding=0)), S.vae_downsample, "ed_conv3x3_nhwc_f32out_s2")
    sd = _rounded(ctor(), 600, F32)
    ref_sd, gpu_sd = _sides(sd)
    x64, x = _x(9, (3, C, 16, 16), F32, scale)
    if scale > 1.0:
        assert float(x.abs().max()) > 65504.0
    with torch.no_grad():
        ref = fn(ref_sd, "blk", x64)
    m = _load(ctor(), sd, F32)
    judge(ops, f"VAE {kind}sampler split operands, input scale {scale:g}", lambda: m(x), lambda: fn(gpu_sd, "blk", x), ref,
          expect=("ed_absmax_f32", "ed_split_f32_nhwc", kernel))


def test_vae_attention(mods):
    M, ops = mods
    sd = _rounded(M._VaeAttention(64), 700, F32)
    ref_sd, gpu_sd = _sides(sd)
    x64, x = _x(11, (3, 64, 16, 16), F32)
    with torch.no_grad():
        ref = S.vae_attention(ref_sd, "blk", x64)
    m = _load(M._VaeAttention(64), sd, F32)
    judge(ops, "_VaeAttention", lambda: m(x), lambda: S.vae_attention(gpu_sd, "blk", x), ref, expect=("ed_softmax_rows",))


def test_vae_encode_and_decode(mods):
    M, ops = mods
    boc = tuple(M.SMALL_VAE_CHANNELS)
    sd = _rounded(M.AutoencoderKL(block_out_channels=boc), 800, F32)
    ref_sd, gpu_sd = _sides(sd, "")
    g = torch.Generator().manual_seed(12)
    img64 = (torch.rand(3, 3, 64, 64, generator=g, dtype=torch.float64) * 2 - 1).float().double()
    z64 = torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64).float().double()
    img, z = img64.to(DEV, F32), z64.to(DEV, F32)
    with torch.no_grad():
        ref_enc, ref_dec = list(S.vae_encode(ref_sd, boc, img64)), S.vae_decode(ref_sd, boc, z64)
    m = _load(M.AutoencoderKL(block_out_channels=boc), sd, F32)
    M.prepare_vae_split(m)

    def encode():
        d = m.encode(img).latent_dist
        return [d.mean, d.std]
    # (32 / 64 channels: 1 / 2 per group -- the blocks stay with the library, the 64-channel samplers take the split-operand kernels)
    common = ("ed_groupnorm_f32", "ed_absmax_f32", "ed_split_f32_nhwc", "ed_softmax_rows")
    judge(ops, "small VAE encode (mean, std)", encode, lambda: list(S.vae_encode(gpu_sd, boc, img)), ref_enc,
          expect=common + ("ed_conv3x3_nhwc_f32out_s2",), whole=True, library_conv=True)
    judge(ops, "small VAE decode", lambda: m.decode(z).sample, lambda: S.vae_decode(gpu_sd, boc, z), ref_dec,
          expect=common + ("ed_conv3x3_nhwc_f32out",), whole=True, library_conv=True)


# ---- the fp32 residual stream under a 16-bit model (UNet2DConditionModel.residual_fp32, the default of the SD 1.x / 2.x family) ---------
# The stream input of every case is the case's 16-bit-representable x carried as fp32; the yardstick stays the all-16-bit spec on the GPU.
# Every case also prints its error beside the plain-mode (16-bit stream) error of the same case: recorded, not asserted.
CONV3X3_KERNELS = ("ed_conv3x3_nhwc", "ed_conv3x3_nhwc_up2x", "ed_conv3x3_nhwc_s2", "ed_conv3x3_nhwc_f32out", "ed_conv3x3_nhwc_f32out_s2")
NHWC_KERNELS = CONV3X3_KERNELS + ("ed_groupnorm_nhwc", "ed_groupnorm_nhwc_s32", "ed_groupnorm_nhwc_cat")


def _as_stream(x, cl=True):
    """the same (16-bit-representable) values as the fp32 residual stream"""
    return x.float().contiguous(memory_format=CL) if cl else x.float().contiguous()


def _beside_plain(name, run32, run_plain, ref, whole=False):
    """print the stream32 error beside the plain-mode error of the same case (the ratio is a record, the asserted bar is ``judge``'s)"""
    err = (lambda a: S.rel_l2(_listed(a), _listed(ref))) if whole else (lambda a: _max_err(a, ref))
    with torch.no_grad():
        e32, e16 = err(run32()), err(run_plain())
    print(f"{name}: stream32 {e32:.3e} plain {e16:.3e} stream32/plain {e32 / max(e16, 1e-300):.2f}")
    return e32, e16


def _deterministic(run):
    """one run with the library asked for deterministic solvers: for bit-for-bit comparisons of runs that reach its convolutions"""
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            return run()
    finally:
        torch.backends.cudnn.deterministic = keep


@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_bf16_resnet_on_the_fp32_residual_stream(cin, cout, mods, admit):
    """bf16 has no fp32-output convolution: conv2 is the 16-bit ed_conv3x3_nhwc (bias in its epilogue), its result is added to the stream
    by ONE fp32 torch add, the shortcut (cin != cout) is ed_linear over the token view of the narrowed stream"""
    M, ops = mods
    dtype = torch.bfloat16
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=True)
    x32 = _as_stream(x)
    name = f"ResnetBlock2D fp32 stream {cin}->{cout} bfloat16"
    stats = judge(ops, name, lambda: blk(x32, emb), spec, ref,
                  expect=("ed_groupnorm_nhwc_s32", "ed_groupnorm_nhwc", "ed_conv3x3_nhwc") + (("ed_linear",) if cin != cout else ()),
                  forbid=("ed_conv3x3_nhwc_f32out", "ed_bias_residual_add"))
    assert stats["ed_conv3x3_nhwc"][0] == 2 and stats["ed_groupnorm_nhwc"][0] == 1 and stats["ed_groupnorm_nhwc_s32"][0] == 1, stats
    with torch.no_grad():
        out = blk(x32, emb)
    assert out.dtype == torch.float32 and ops.is_nhwc(out)
    _beside_plain(name, lambda: blk(x32, emb), lambda: blk(x, emb), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_on_the_fp32_residual_stream_default_policy(cin, cout, dtype, mods, monkeypatch):
    """no admission: at this size the policy leaves both convolutions with the library.  norm1 reads the stream (ed_groupnorm_nhwc_s32),
    conv1 keeps its bias, the time embedding is folded into norm2 (ed_groupnorm_nhwc's chan_bias), conv2's result and the shortcut's are
    summed in fp32 by torch"""
    M, ops = mods
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=True)
    x32 = _as_stream(x)
    folded = []
    inner = ops.groupnorm_nhwc

    def spy(*a, **k):
        folded.append((k.get("chan_bias") is not None, k.get("conv_bias") is not None))
        return inner(*a, **k)
    monkeypatch.setattr(ops, "groupnorm_nhwc", spy)
    name = f"ResnetBlock2D fp32 stream, default policy {cin}->{cout} {_name(dtype)}"
    stats = judge(ops, name, lambda: blk(x32, emb), spec, ref, expect=("ed_groupnorm_nhwc_s32", "ed_groupnorm_nhwc"),
                  forbid=CONV3X3_KERNELS + ("ed_bias_residual_add", "ed_groupnorm"), library_conv=True)
    assert stats["ed_groupnorm_nhwc_s32"][0] == 1 and stats["ed_groupnorm_nhwc"][0] == 1, stats
    assert folded and all(f == (True, False) for f in folded), folded     # the time embedding in the kernel; conv1's bias stayed in conv1
    with torch.no_grad():
        out = blk(x32, emb)
    assert out.dtype == torch.float32 and ops.is_nhwc(out)
    _beside_plain(name, lambda: blk(x32, emb), lambda: blk(x, emb), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("policy", ["default", "admitted"])
def test_resnet_with_small_groups_on_the_fp32_residual_stream(policy, dtype, mods, monkeypatch):
    """64 -> 128 channels, 2 and 4 channels per group, on the stream: torch's GroupNorm with fp32 parameters and the library's
    convolutions, nothing of ours launched.  With the GEMM kernels admitted no normalisation or convolution kernel takes the block either;
    the one launch is the 1x1 shortcut, which the stream path runs as a linear over the token view of the narrowed stream (ed_linear)."""
    M, ops = mods
    if policy == "admitted":
        _admit(monkeypatch, ops)
    blk, x, emb, ref, spec = _resnet(M, 64, 128, dtype, cl=True)
    x32 = _as_stream(x)
    name = f"ResnetBlock2D fp32 stream 64->128 (C/G < 8), {policy}, {_name(dtype)}"
    stats = judge(ops, name, lambda: blk(x32, emb), spec, ref, library_conv=True)
    assert set(stats) == ({"ed_linear"} if policy == "admitted" else set()), sorted(stats)
    if stats:
        assert stats["ed_linear"][0] == 1, stats
    with torch.no_grad():
        assert blk(x32, emb).dtype == torch.float32
    _beside_plain(name, lambda: blk(x32, emb), lambda: blk(x, emb), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cin,cout", RES_SHAPES)
def test_resnet_on_an_nchw_fp32_residual_stream(cin, cout, dtype, mods, admit, monkeypatch):
    """CHANNELS_LAST off: an NCHW-contiguous fp32 stream and NCHW weights.  No channels-last kernel may take it (even with the GEMM kernels
    admitted): torch's GroupNorm reads the stream, norm2 is the NCHW ed_groupnorm with the time embedding folded in"""
    M, ops = mods
    monkeypatch.setattr(M, "CHANNELS_LAST", False)
    blk, x, emb, ref, spec = _resnet(M, cin, cout, dtype, cl=False)
    x32 = _as_stream(x, cl=False)
    name = f"ResnetBlock2D NCHW fp32 stream {cin}->{cout} {_name(dtype)}"
    judge(ops, name, lambda: blk(x32, emb), spec, ref, expect=("ed_groupnorm",), forbid=NHWC_KERNELS + ("ed_linear", "ed_bias_residual_add"),
          library_conv=True)
    with torch.no_grad():
        out = blk(x32, emb)
    assert out.dtype == torch.float32 and out.is_contiguous()
    _beside_plain(name, lambda: blk(x32, emb), lambda: blk(x, emb), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("cout", [256, 320])
def test_resnet_on_a_concatenation_of_two_fp32_streams(cout, dtype, mods, admit):
    """forward_cat on fp32 x and skip: ed_groupnorm_nhwc_cat is a 16-bit kernel, so the concatenation is materialised (channels-last fp32)
    and the block runs its stream path on it -- ed_groupnorm_nhwc_s32, the HIP convolutions, the 384 -> cout shortcut through ed_linear"""
    M, ops = mods
    c1, c2 = 256, 128
    sd, gpu_sd, x, skip, emb, ref = _cat_case(c1, c2, cout, dtype)
    blk = _load(M.ResnetBlock2D(c1 + c2, cout, TEMB), sd, dtype, cl=True)
    x32, s32 = _as_stream(x), _as_stream(skip)
    xc, sc = x.contiguous(memory_format=CL), skip.contiguous(memory_format=CL)
    name = f"ResnetBlock2D.forward_cat on fp32 streams {c1}+{c2}->{cout} {_name(dtype)}"
    closing = ("ed_conv3x3_nhwc_f32out",) if dtype == torch.float16 else ()
    stats = judge(ops, name, lambda: blk.forward_cat(x32, s32, emb), lambda: S.resnet_cat(gpu_sd, "blk", x, skip, emb), ref,
                  expect=("ed_groupnorm_nhwc_s32", "ed_groupnorm_nhwc", "ed_conv3x3_nhwc", "ed_linear") + closing,
                  forbid=("ed_groupnorm_nhwc_cat", "ed_bias_residual_add") + (() if closing else ("ed_conv3x3_nhwc_f32out",)))
    assert stats["ed_groupnorm_nhwc_s32"][0] == 1 and stats["ed_linear"][0] == 1, stats
    with torch.no_grad():
        out = blk.forward_cat(x32, s32, emb)
        assert out.dtype == torch.float32 and ops.is_nhwc(out)
        assert torch.equal(out, blk(torch.cat([x32, s32], 1), emb))
    _beside_plain(name, lambda: blk.forward_cat(x32, s32, emb), lambda: blk.forward_cat(xc, sc, emb), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("mode", ["default", "admitted"])
@pytest.mark.parametrize("linear", [True, False], ids=["linear-proj", "conv-proj"])
@pytest.mark.parametrize("C,heads", [(256, 4), (320, 8)], ids=["hd64", "hd40"])
def test_transformer_2d_on_the_fp32_residual_stream(C, heads, linear, mode, dtype, mods, monkeypatch):
    """Transformer2DModel, depth 2, on a channels-last fp32 stream: the GroupNorm reads it (ed_groupnorm_nhwc_s32), the token stream is
    widened after proj_in, every LayerNorm is a stream kernel (ed_layernorm_s32 once, ed_add_layernorm_s32 for the five that follow an add),
    the token stream is narrowed before proj_out and the closing add is torch's in fp32.  ``admitted``: the projections through ed_linear /
    ed_geglu_gemm -- and with FUSED_RESIDUAL_LINEAR on as well no `x + branch` may ride in ed_linear's 16-bit residual epilogue while the
    residual is fp32: the result is bit-identical to the run with the switch off."""
    M, ops = mods
    if mode == "admitted":
        _admit(monkeypatch, ops)
    monkeypatch.setattr(M, "FUSED_RESIDUAL_LINEAR", False)
    sd, gpu_sd, x, ctx, ref = _transformer_case(C, heads, linear, dtype)
    m = _load(M.Transformer2DModel(C, heads, 2, CROSS, linear), sd, dtype, cl=True)
    x32, xc = _as_stream(x), x.contiguous(memory_format=CL)
    expect = {"ed_groupnorm_nhwc_s32", "ed_layernorm_s32", "ed_add_layernorm_s32", "ed_flash_attention"}
    forbid = {"ed_tokens_add_nchw", "ed_layernorm", "ed_add_layernorm", "ed_groupnorm", "ed_groupnorm_nhwc"}
    if mode == "admitted":
        expect |= {"ed_geglu_gemm", "ed_linear"}
        forbid.add("ed_geglu")
    else:
        expect.add("ed_geglu")
        forbid |= {"ed_geglu_gemm", "ed_linear"}
    name = f"Transformer2DModel fp32 stream C={C} heads={heads} {'linear' if linear else 'conv'} projection, {mode}, {_name(dtype)}"
    stats = judge(ops, name, lambda: m(x32, ctx), lambda: S.transformer_2d(gpu_sd, "blk", x, ctx, heads, 2, linear), ref,
                  expect=expect, forbid=forbid, library_conv=not linear)
    assert stats["ed_layernorm_s32"][0] == 1 and stats["ed_add_layernorm_s32"][0] == 5 and stats["ed_groupnorm_nhwc_s32"][0] == 1, stats
    off = _deterministic(lambda: m(x32, ctx))        # (conv-proj reaches the library's 1x1 convolutions: see judge)
    assert off.dtype == torch.float32 and ops.is_nhwc(off)
    residuals = []
    inner = ops.linear

    def spy(*a, **k):
        residuals.append(k.get("residual") is not None or len(a) > 3)
        return inner(*a, **k)
    monkeypatch.setattr(ops, "linear", spy)
    monkeypatch.setattr(M, "FUSED_RESIDUAL_LINEAR", True)
    ops.TIMER.start()
    try:
        on = _deterministic(lambda: m(x32, ctx))
    finally:
        on_stats = ops.TIMER.stop()
    assert not any(residuals), "an fp32 residual rode in ed_linear's 16-bit epilogue"
    assert (mode == "admitted") == bool(residuals)
    assert torch.equal(on, off), (name, "FUSED_RESIDUAL_LINEAR changes the stream path")
    assert on_stats["ed_add_layernorm_s32"][0] == 5 and "ed_layernorm" not in on_stats and "ed_add_layernorm" not in on_stats, on_stats
    monkeypatch.setattr(M, "FUSED_RESIDUAL_LINEAR", False)
    _beside_plain(name, lambda: m(x32, ctx), lambda: m(xc, ctx), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("C", [128, 320])
def test_samplers_on_the_fp32_residual_stream(C, dtype, mods, admit, monkeypatch):
    """Downsample2D / Upsample2D on a stream: narrow, the same convolution kernels as on a 16-bit activation, widen -- exactly"""
    M, ops = mods
    monkeypatch.setattr(ops, "gemm_rows_mode", lambda *a: False)     # as test_samplers_on_the_convolution_main_loop
    monkeypatch.setattr(M, "HIP_DOWNSAMPLE_CONV", True)
    for kind, ctor, hw, fn, kernel in (("Downsample2D", lambda: M.Downsample2D(C), (32, 32), S.downsample, "ed_conv3x3_nhwc_s2"),
                                       ("Upsample2D", lambda: M.Upsample2D(C), (16, 16), S.upsample, "ed_conv3x3_nhwc_up2x")):
        sd = _rounded(ctor(), 500 + C, dtype)
        ref_sd, gpu_sd = _sides(sd)
        x64, x = _x(7, (3, C) + hw, dtype)
        with torch.no_grad():
            ref = fn(ref_sd, "blk", x64)
        m = _load(ctor(), sd, dtype, cl=True)
        xc, x32 = x.contiguous(memory_format=CL), _as_stream(x)
        name = f"{kind}({C}) fp32 stream {_name(dtype)}"
        stats = judge(ops, name, lambda: m(x32), lambda: fn(gpu_sd, "blk", x), ref, expect=(kernel,))
        assert set(stats) == {kernel} and stats[kernel][0] == 1, stats
        with torch.no_grad():
            out, plain = m(x32), m(xc)
        assert out.dtype == torch.float32 and plain.dtype == dtype
        assert torch.equal(out, plain.float())       # widening is exact
        _beside_plain(name, lambda: m(x32), lambda: m(xc), ref)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("fam", ["sd15", "sdxl"])
def test_unet_forward_on_the_fp32_residual_stream(fam, dtype, mods):
    """test_unet_forward's three cases with ``residual_fp32`` on, against the same fp64 outputs: conv_in's result is widened, every block
    reads and writes the fp32 stream (ControlNet residuals are 16-bit tensors added onto fp32 skips), conv_norm_out reads it and the
    output is the model dtype again.  Switched off again, the model must compute bit for bit what it computed before the switch: the
    mode leaves nothing behind in the derived-weight caches."""
    M, ops = mods
    cfg, usd, _, i64, res, ref = _net_case(fam, dtype)
    m = _load(M.UNet2DConditionModel(**cfg), usd, dtype, cl=M.CHANNELS_LAST)
    gpu_sd = _sides(usd, "")[1]
    i = _to_dev(i64, dtype)
    down, mid = [d.to(DEV) for d in res[0]], res[1].to(DEV)
    expect = {"ed_layernorm_s32", "ed_add_layernorm_s32", "ed_flash_attention"} | ({"ed_groupnorm_nhwc_s32"} if M.CHANNELS_LAST else set())
    for case, t, extra, sx in (("per-row", i["t"], {}, ()), ("scalar", i["t"][0], {}, ()),
                               ("residuals", i["t"], dict(down_block_additional_residuals=down, mid_block_additional_residual=mid), (down, mid))):
        def run():
            return m(i["sample"], t, encoder_hidden_states=i["context"], added_cond_kwargs=i["added"], **extra).sample
        assert not getattr(m, "residual_fp32", False)
        before = _deterministic(run)
        m.residual_fp32 = True
        try:
            name = f"{fam} UNet fp32 stream {_name(dtype)}, {case}"
            judge(ops, name, run, lambda: S.unet_forward(gpu_sd, cfg, i["sample"], t, i["context"], i["added"], *sx), ref[case],
                  expect=expect, forbid=("ed_layernorm", "ed_add_layernorm"), whole=True, library_conv=True)
            with torch.no_grad():
                got = run()
            assert got.dtype == dtype
        finally:
            m.residual_fp32 = False
        after = _deterministic(run)
        assert torch.equal(before, after), (name, "the plain mode computes something else after a stream32 forward")
        e32, e16 = S.rel_l2([got], [ref[case]]), S.rel_l2([before], [ref[case]])
        print(f"{name}: stream32 {e32:.3e} plain {e16:.3e} stream32/plain {e32 / max(e16, 1e-300):.2f}")
