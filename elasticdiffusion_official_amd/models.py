"""Torch-ROCm model modules behind the hot path's model boundary (``unet_step``, elastic_diffusion.py:393-432;
``decode_latents`` :267-272; ``make_denoised_background`` :350; ControlNet elastic_diffusion_w_controlnet.py:476-518).

The reference takes these from ``diffusers==0.21.4`` (``UNet2DConditionModel``, ``AutoencoderKL``,
``ControlNetModel``), which is neither vendored nor installable here, and no pretrained weights exist offline.  These
are from-scratch pure-torch modules with the SD-1.x / SD-2.x-base / SDXL-base architecture hyper-parameters and
HF-layout parameter names (so a ``diffusion_pytorch_model.safetensors`` state dict loads with ``load_weights``).  For
benchmarks they are randomly initialised from a fixed seed ("synthetic" in bench.py).

This is plumbing, not the product: dense contractions (conv / linear / attention) go to MIOpen / hipBLASLt / SDPA,
i.e. the MFMA pipes, through PyTorch-ROCm; the memory-bound glue between them (GroupNorm+SiLU, GroupNorm->token
layout, GEGLU) is fused into hand-written HIP kernels (csrc/unet_kernels.hip) for 16-bit activations.
"""
import math
import os
import threading
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from .geometry import plan_constant_axis
from . import ops      # (imports without the shared library: it is loaded at the first launch)


# Fused HIP kernels inside the UNet (csrc/unet_kernels.hip): used for 16-bit CUDA activations; anything else (the fp32
# VAE, the CPU-baseline copy of the UNet, odd shapes) takes the plain torch ops.  Toggle for A/B measurements.
FUSED_KERNELS = True


# Channels-last activations end to end: MIOpen's CK convolutions are NHWC kernels, and an NCHW problem costs a layout
# transpose on either side of every convolution (batched_transpose_*: 5.9 ms of a 178 ms batch-20 forward,
# profiles/r2_s5_unet_fwd_b20_nchw_kernel_stats.csv).  With channels-last activations those launches disappear, GroupNorm's
# token-layout output and the transformer's closing residual add become plain views / contiguous adds, and the 1x1
# shortcut convolutions are plain GEMMs.  Measured (hipGraph replay, profiles/r2_s5_probe_channels_last.jsonl):
# 168.6 vs 174.9 ms at batch 20, 60.0 vs 61.4 ms at batch 6.  The in-tree MIOpen db carries NHWC entries derived from the
# tuned NCHW ones (tools/miopen_nhwc_from_nchw.py).  ED_CHANNELS_LAST=0 switches back (A/B).
CHANNELS_LAST = os.environ.get("ED_CHANNELS_LAST", "1") == "1"


_HALF = (torch.bfloat16, torch.float16)


def _fusable(x):
    return FUSED_KERNELS and x.is_cuda and x.dtype in _HALF and x.is_contiguous()


def _fusable_nhwc(x):
    return FUSED_KERNELS and x.is_cuda and x.dtype in _HALF and ops.is_nhwc(x)


# ---- fp32 residual stream under a 16-bit model (round 6, ``UNet2DConditionModel.residual_fp32``) ---------------------------------------
# The tolerance mode for configurations whose fp16 latent ends outside north_star's 1e-3 (cfg2, SD 1.5 512 x 1024: 1.09e-3 against the
# fp32 loop, profiles/bench_r6_s1_cfg2_fp32leg.json): the tensor that persists from block to block -- x in `x = x + branch(norm(x))` -- is
# kept in fp32, every branch still computes in the 16-bit model dtype (same MFMA kernels, same weights), i.e. the adds no longer round
# (a third of the 16-bit loop's drift by profiles/r5_precision_attribution.json).  Everything that READS the stream takes fp32 in and
# hands the model dtype on: the normalisation layers through torch ops in this mode (their HIP kernels are 16-bit in / out), the
# up / down-sampling and shortcut convolutions after a cast; everything that WRITES it adds a 16-bit branch result to the fp32 stream.
def _stream32(x, module_dtype):
    """is ``x`` an fp32 residual stream feeding a module whose parameters are 16-bit?"""
    return x.dtype == torch.float32 and module_dtype in _HALF


def _derived(module, slot, params, build):
    """``build()``, cached on ``module`` under ``slot`` and rebuilt when one of the source ``params`` is replaced (id: a fresh Parameter
    the caching allocator placed at the freed address has the same data_ptr and version 0), moved, written in place or cast"""
    key = tuple((id(p), p.data_ptr(), p._version, p.dtype, str(p.device)) for p in params)
    cache = module.__dict__.setdefault("_derived", {})
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        hit = cache[slot] = (key, build())
    return hit[1]


def _f32_params(norm):
    """fp32 copies of a normalisation layer's (weight, bias)"""
    w, b = norm.weight, norm.bias
    return _derived(norm, "f32", (w, b), lambda: (w.detach().float(), b.detach().float()))


def _f32_bias(mod):
    """fp32 copy of a module's bias (None without one)"""
    b = mod.bias
    return None if b is None else _derived(mod, "bias32", (b,), lambda: b.detach().float())


# The narrowed constant-image encode (AutoencoderKL.encode_constant): {(H, W) of an activation: (wx [W] | None, wy [H] | None, key_bias
# [H * W] | None)} -- the multiplicity of every column / row of the encoder's activations at that size, and its logarithm per token for
# the mid-block attention.  Set (per thread) only while such an encode runs: every GroupNorm and the attention are otherwise what
# they always were.
_CONSTANT_ENCODE = threading.local()


def _narrowed_encode_active():
    return getattr(_CONSTANT_ENCODE, "planes", None) is not None


def _plane_weights(x):
    planes = getattr(_CONSTANT_ENCODE, "planes", None)
    return (None, None, None) if planes is None else planes.get((x.shape[2], x.shape[3]), (None, None, None))


def _weighted_group_norm(norm, x, wx, wy, silu):
    """GroupNorm [+ SiLU] whose statistics count pixel (y, x) wy[y] * wx[x] times: the HIP kernels for the fp32 layouts the product runs
    (ed_groupnorm_nhwc_f32_weighted / ed_groupnorm_f32_weighted), plain torch for everything else (CPU, fp64, 16-bit)."""
    N, C, H, W = x.shape
    G = norm.num_groups
    if FUSED_KERNELS and x.is_cuda and x.dtype == torch.float32 and norm.weight.dtype == torch.float32:
        w32 = [None if w is None else w.float() for w in (wx, wy)]
        if VAE_SPLIT_CONV and ops.is_nhwc(x) and ops.groupnorm_nhwc_f32_ok(C, G):
            return ops.groupnorm_nhwc_f32(x, norm.weight, norm.bias, G, norm.eps, silu=silu, wx=w32[0], wy=w32[1])
        if VAE_HIP_GROUPNORM and x.is_contiguous() and (H * W) % 4 == 0 and N * G <= 65535:
            return ops.groupnorm_f32(x, norm.weight, norm.bias, G, norm.eps, silu=silu, wx=w32[0], wy=w32[1])
    dt = torch.float32 if x.dtype in _HALF else x.dtype
    xf = x.to(dt).reshape(N, G, C // G, H, W)
    w = (torch.ones(H, dtype=dt, device=x.device) if wy is None else wy.to(dt))[:, None] \
        * (torch.ones(W, dtype=dt, device=x.device) if wx is None else wx.to(dt))[None, :]
    count = w.sum() * (C // G)
    mean = (xf * w).sum((2, 3, 4), keepdim=True) / count
    d = xf - mean
    var = (d * d * w).sum((2, 3, 4), keepdim=True) / count
    y = (d * torch.rsqrt(var + norm.eps)).reshape(N, C, H, W) * norm.weight.to(dt)[None, :, None, None] + norm.bias.to(dt)[None, :, None, None]
    return (F.silu(y) if silu else y).to(x.dtype)


def group_norm_act(norm, x, silu=False, tokens=False, chan_bias=None, conv_bias=None):
    """GroupNorm [+ SiLU] [-> (N, H*W, C) token layout] of ``x``, or of ``(x + conv_bias[c]) + chan_bias[n, c]``: the
    bias of the (bias-free) convolution that produced x and the time-embedding add of ResnetBlock2D, folded into the
    kernel.  HIP: ed_groupnorm / ed_groupnorm_nhwc; torch otherwise."""
    N, C, H, W = x.shape
    G = norm.num_groups
    cpg = C // G
    wx, wy, _ = _plane_weights(x)
    if wx is not None or wy is not None:
        if tokens or chan_bias is not None or conv_bias is not None:
            # the narrowed encode runs its ResnetBlocks without folded biases (ResnetBlock2D.forward) and never asks for tokens
            raise RuntimeError("group_norm_act: weighted statistics take no folded bias and no token layout")
        return _weighted_group_norm(norm, x, wx, wy, silu)
    s32 = _stream32(x, norm.weight.dtype)
    nhwc = not s32 and _fusable_nhwc(x) and C % 8 == 0 and cpg >= 8
    if (chan_bias is not None or conv_bias is not None) and (
            s32 or not (FUSED_TEMB_ADD and (nhwc or (_fusable(x) and (H * W) % 8 == 0 and not tokens)))):
        # no kernel on this path folds the biases in
        if conv_bias is not None:
            x = x + conv_bias[None, :, None, None]
        if chan_bias is not None:
            x = x + chan_bias[:, :, None, None]
        chan_bias = conv_bias = None
        nhwc = not s32 and _fusable_nhwc(x) and C % 8 == 0 and cpg >= 8
    if s32 or nhwc:
        if nhwc:
            y = ops.groupnorm_nhwc(x, norm.weight, norm.bias, G, norm.eps, silu=silu,
                                   chan_bias=None if chan_bias is None else chan_bias.contiguous(), conv_bias=conv_bias)
        elif FUSED_KERNELS and x.is_cuda and C % 8 == 0 and cpg >= 8 and C <= 4096 and G <= 256 and ops.is_nhwc(x):
            # HIP: ed_groupnorm_nhwc_s32 (fp32 stream in, model dtype out; the 16-bit kernel's three launches)
            y = ops.groupnorm_nhwc_s32(x, norm.weight, norm.bias, G, norm.eps, silu=silu)
        else:   # fp32 residual stream: statistics and affine in fp32, the result in the model dtype
            y = F.group_norm(x, G, *_f32_params(norm), norm.eps)
            if silu:
                y = F.silu(y)
            y = y.to(norm.weight.dtype)
            if CHANNELS_LAST and y.is_cuda:
                y = y.contiguous(memory_format=torch.channels_last)
        return y.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else y  # a view: NHWC memory is the token layout
    if chan_bias is not None or conv_bias is not None:
        return ops.groupnorm(x, norm.weight, norm.bias, G, norm.eps, silu=silu,
                             chan_bias=None if chan_bias is None else chan_bias.contiguous(), conv_bias=conv_bias)
    if _fusable(x) and (H * W) % 8 == 0 and (not tokens or cpg % 4 == 0):
        return ops.groupnorm(x, norm.weight, norm.bias, G, norm.eps, silu=silu, tokens=tokens)
    if FUSED_KERNELS and x.is_cuda and x.dtype == torch.float32 and not tokens and norm.weight.dtype == torch.float32:
        # the channels-last fp32 VAE (VAE_SPLIT_CONV): the normalisation layers that do not feed a split convolution
        if VAE_SPLIT_CONV and ops.is_nhwc(x) and ops.groupnorm_nhwc_f32_ok(C, G):
            return ops.groupnorm_nhwc_f32(x, norm.weight, norm.bias, G, norm.eps, silu=silu)
        # the fp32 VAE: split statistics + apply (+SiLU) instead of torch's one-block-per-group moments
        if VAE_HIP_GROUPNORM and x.is_contiguous() and (H * W) % 4 == 0 and N * G <= 65535:
            return ops.groupnorm_f32(x, norm.weight, norm.bias, G, norm.eps, silu=silu)
    y = F.group_norm(x, G, norm.weight, norm.bias, norm.eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else y


FUSED_LAYERNORM = True
FUSED_TEMB_ADD = True      # ResnetBlock2D: h + temb folded into norm2 (ed_groupnorm chan_bias)
FUSED_CONV_BIAS = True     # ResnetBlock2D: bias-free convolutions, biases folded into norm2 / the closing residual add
FUSED_ADD_LAYERNORM = True  # BasicTransformerBlock: residual add + next LayerNorm in one kernel (ed_add_layernorm)
FUSED_TOKENS_ADD = True     # Transformer2DModel: tokens -> NCHW + residual in one kernel (ed_tokens_add_nchw)
FLASH_ATTENTION = True      # Attention: ed_flash_attention (head_dim 64, 16-bit) instead of SDPA / AOTriton
FUSED_QKV = True            # Attention: one projection GEMM for q,k,v (self) / k,v (cross)
HIP_GEGLU_GEMM = True       # GEGLU: projection GEMM with the gated product in its epilogue (ed_geglu_gemm) instead of hipBLASLt + ed_geglu
HIP_LINEAR = True           # the projections where ed_linear measured faster than hipBLASLt (ops.linear_wins)
FUSED_SKIP_CAT = True        # up blocks: ResnetBlock2D(cat([hidden, skip])) without the concatenated tensor (ed_groupnorm_nhwc_cat + a K-split shortcut)
FUSED_PROJ_OUT_ADD = True    # Transformer2DModel (channels-last): the closing x + proj_out(h) in ed_linear's residual epilogue
# Downsample2D (stride 2, padding 1), channels-last, as ed_conv3x3_nhwc_s2 instead of MIOpen's CK kernel: correct (tests) and a TIE in the forward
# (profiles/r6_s10_switch_ab_downsample.jsonl: +0.3 % at 40 rows, +0.2 % at 12, -0.1 % at 20, -0.2 % at 6 -- N = 320 fills 62 % of its two
# 256-column tiles), so the library call stays; the entry point and this switch are kept for A/B
HIP_DOWNSAMPLE_CONV = False
# BasicTransformerBlock: x + to_out(...) / x + ff(...) inside ed_linear's epilogue where that kernel runs the projection (the 640-channel level),
# the following LayerNorm then a plain one.  Measured NO gain in the forward (profiles/r6_s11_switch_ab_residual_linear.jsonl: -0.4 % at 40 rows,
# -0.3 % at 12, +0.1 % at 20, 0 at 6): the epilogue's residual read costs the projection what ed_add_layernorm -> ed_layernorm saves
# (profiles/r6_s11_addmm_probe.jsonl: [20480, 1280 -> 1280] projection + add-LayerNorm 94.8 us, own projection with residual + LayerNorm 96.7,
# library beta = 1 + LayerNorm 103.7).  Off; kept as an A/B switch.
FUSED_RESIDUAL_LINEAR = False
FUSED_UPSAMPLE_CONV = True   # Upsample2D: nearest 2x + conv 3x3 as one ed_conv3x3_nhwc_up2x launch (the A operand is gathered from the source)
HIP_CONV3X3 = True          # ResnetBlock2D / Upsample2D 3x3 convolutions, channels-last: ed_conv3x3_nhwc (+bias, +temb, +residual) instead of MIOpen
VAE_HIP_GROUPNORM = True    # VAE GroupNorm(+SiLU), fp32 NCHW: ed_groupnorm_f32 instead of torch's moments + affine + SiLU kernels
VAE_HIP_ATTENTION = True    # VAE mid-block attention: fp32 GEMM + ed_softmax_rows + fp32 GEMM instead of SDPA (AOTriton)
# _VaeAttention's residual: `x + attn` (True: the VAE stays NCHW -- ed_groupnorm_f32 everywhere, MIOpen's NCHW solvers) or
# `attn + x` (False, rounds 1-3: the permuted first operand makes the sum, and so the rest of the encoder / decoder,
# channels-last -- MIOpen's NHWC fp32 igemm convolutions, torch GroupNorm through strided copies).  Same values bit for
# bit.  Measured on the MI355X, each layout with its own MIOpen find (profiles/r4_s1_vae_layout_ab.jsonl): 8 decode tiles of
# 128 x 128 latents 979 -> 760 ms, the 128 x 256 decode 202 -> 198 ms, 5 pad-strip encodes 54.9 -> 54.7 ms.
VAE_NCHW_RESIDUAL = True
# Round 5: the VAE's ResnetBlock convolutions (94 % of the encoder's and 71 % of the decoder's convolution FLOPs) on the 16-bit MFMA
# pipe at fp32 accuracy: the activation after GroupNorm + SiLU and the weights are each carried as an fp16 (hi, lo) pair and
# x.w = xh.wh + xl.wh + xh.wl is ONE ed_conv3x3_nhwc main loop over 3 Cin channels with an fp32 epilogue (csrc/vae_kernels.hip).  The
# ResnetBlocks then pass channels-last fp32 activations to each other (the kernel's layout); the stream-fed up / down-sampling
# convolutions, conv_in / conv_out and the mid-block attention stay with the fp32 libraries in NCHW (_to_nchw: one layout copy per block
# boundary).  As accurate against fp64 as the library's fp32 convolution (tests/test_vae_split.py).
VAE_SPLIT_CONV = True
VAE_SPLIT_DOWNSAMPLE = True   # round 6: the encoder's stride-2 downsamplers on the split-operand path as well (ed_conv3x3_nhwc_f32out_s2)
# AutoencoderKL.encode_constant (the pad strips: constant-colour images) runs the encoder on an image narrowed to the non-constant border
# plus one weighted row / column per level (geometry.plan_constant_axis) -- 4x fewer pixels for a 256 x 1024 px strip.
# False: the full image through ``encode``.
VAE_NARROW_CONSTANT = True
# A/B switch from the environment: ED_DISABLE=FLASH_ATTENTION,FUSED_QKV,... turns the named module switches off
for _name in filter(None, os.environ.get("ED_DISABLE", "").split(",")):
    if _name not in globals() or not isinstance(globals()[_name], bool):
        raise RuntimeError(f"ED_DISABLE: unknown switch {_name!r}")
    globals()[_name] = False


def fused_unet_entry_points():
    """C-ABI entry points a 16-bit UNet forward reaches with the current switches (the real-architecture parity test
    checks that they were actually launched, i.e. that no torch fallback silently took over).  ed_linear / ed_conv3x3_nhwc
    take only the shapes they win on (ops.linear_wins / conv3x3_ok), so they are not REQUIRED of every model; where the
    convolution kernel runs, its epilogue has replaced ed_bias_residual_add."""
    hip_conv = FUSED_KERNELS and HIP_CONV3X3 and CHANNELS_LAST
    on = [("ed_groupnorm_nhwc" if CHANNELS_LAST else "ed_groupnorm", FUSED_KERNELS),
          ("ed_geglu_gemm" if HIP_GEGLU_GEMM else "ed_geglu", FUSED_KERNELS),
          ("ed_layernorm", FUSED_KERNELS and FUSED_LAYERNORM),
          ("ed_flash_attention", FUSED_KERNELS and FLASH_ATTENTION),
          ("ed_add_layernorm", FUSED_KERNELS and FUSED_ADD_LAYERNORM),
          ("ed_tokens_add_nchw", FUSED_KERNELS and FUSED_TOKENS_ADD and not CHANNELS_LAST),
          ("ed_bias_residual_add", FUSED_KERNELS and FUSED_CONV_BIAS and FUSED_TEMB_ADD and not hip_conv)]
    return {n for n, flag in on if flag}


def linear_(x, weight, bias=None):
    """F.linear, through ed_linear for the 16-bit shapes it measured faster on (ops.linear_wins), hipBLASLt otherwise."""
    if (HIP_LINEAR and FUSED_KERNELS and _fusable(x) and weight.dtype == x.dtype and weight.is_contiguous()
            and ops.linear_wins(x.numel() // x.shape[-1], x.shape[-1], weight.shape[0])):
        return ops.linear(x, weight, bias)
    return F.linear(x, weight, bias)


def linear_res_(x, weight, bias, residual):
    """(F.linear(x, weight, bias) + residual, True) in ONE launch where ed_linear takes the projection (its residual epilogue: bias + product +
    residual rounded once), else (F.linear(x, weight, bias), False) and the caller adds -- the transformer blocks' `x = x + branch(...)`: with
    the add inside the projection, the LayerNorm that follows reads and writes 2 units of traffic instead of ed_add_layernorm's 4."""
    if (FUSED_RESIDUAL_LINEAR and residual is not None and HIP_LINEAR and FUSED_KERNELS and _fusable(x) and _fusable(residual)
            and weight.dtype == x.dtype == residual.dtype and weight.is_contiguous()
            and residual.shape == x.shape[:-1] + (weight.shape[0],)
            and ops.linear_wins(x.numel() // x.shape[-1], x.shape[-1], weight.shape[0])):
        return ops.linear(x, weight, bias, residual=residual), True
    return linear_(x, weight, bias), False


def _hip_conv3x3(conv, like, cin):
    """Can ``conv`` (3x3, stride 1, padding 1) run as ed_conv3x3_nhwc on a channels-last activation of ``cin`` channels with the batch,
    size and dtype of ``like`` (which may be the activation itself, or stand for one that does not exist yet)?"""
    w = conv.weight
    if not (HIP_CONV3X3 and w.dtype == like.dtype and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    B, _, H, W = like.shape
    return ops.conv3x3_wins(B, H, W, cin, w.shape[0])


def _hip_conv_pair(blk, like, cin):
    """Do BOTH 3x3 convolutions of the ResnetBlock2D ``blk`` run as ed_conv3x3_nhwc, with norm2 through the channels-last HIP kernel
    between them (its torch fallback hands back an NCHW tensor the convolution wrapper rejects)?  ``like``: a 16-bit channels-last
    tensor with the batch, size and dtype of conv1's input, ``cin`` that input's channels; conv2's Cin is cout.  How
    norm1 runs is the caller's own condition."""
    cout = blk.conv1.out_channels
    return (_fusable_nhwc(like) and cout % 8 == 0 and cout // blk.norm2.num_groups >= 8
            and _hip_conv3x3(blk.conv1, like, cin) and _hip_conv3x3(blk.conv2, like, cout))


def _shortcut_nhwc(sc, x):
    """the 1x1 shortcut convolution of a channels-last ``x`` as a plain GEMM over its token view: no layout change"""
    return linear_(x.permute(0, 2, 3, 1), sc.weight.reshape(sc.out_channels, -1), sc.bias).permute(0, 3, 1, 2)


def _sliced(x, nb, fn):
    """``fn`` on slices of at most ``nb`` samples of the channels-last batch ``x`` (one launch must stay inside the kernels' 32-bit
    offsets), concatenated channels-last"""
    outs = [fn(x[i:i + nb]) for i in range(0, x.shape[0], nb)]
    return outs[0] if len(outs) == 1 else torch.cat(outs).contiguous(memory_format=torch.channels_last)


def _to_nchw(x):
    """The split VAE blocks (VAE_SPLIT_CONV) hand on channels-last fp32 activations; everything around them -- the stream-fed up / down-
    sampling convolutions, the mid-block attention, conv_norm_out / conv_out -- runs NCHW, the layout the in-tree MIOpen find-db has
    fp32 records for (a shape without a record costs a minutes-long find on first use).  One layout copy per block boundary."""
    return x if x.is_contiguous() else x.contiguous()


def _vae_split_ok(x, blk):
    """Can this fp32 VAE ResnetBlock2D (no time embedding) run its two convolutions as split-fp16 MFMA convolutions on ``x``?"""
    if not (VAE_SPLIT_CONV and FUSED_KERNELS and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and blk.time_emb_proj is None and blk.conv1.weight.dtype == torch.float32):
        return False
    B, cin, H, W = x.shape
    cout = blk.conv1.out_channels
    return (ops.groupnorm_nhwc_f32_ok(cin, blk.norm1.num_groups) and ops.groupnorm_nhwc_f32_ok(cout, blk.norm2.num_groups)
            and cin % 64 == 0 and cout % 64 == 0 and H * W * 3 * max(cin, cout) * 2 < 2 ** 31 - 16)


def _split_weight(conv):
    """(split fp16 weight, 2^-k) of a Conv2d for ops.conv3x3_f32out"""
    return _derived(conv, "split", (conv.weight,), lambda: ops.split_conv_weight(conv.weight))


def _split_shortcut(sc, C1):
    """the 1x1 shortcut's weight [cout, C1 + C2, 1, 1] as two contiguous matrices [cout, C1], [cout, C2]"""
    def build():
        w2d = sc.weight.detach().reshape(sc.weight.shape[0], -1)
        return w2d[:, :C1].contiguous(), w2d[:, C1:].contiguous()
    return _derived(sc, ("ksplit", C1), (sc.weight,), build)


def prepare_vae_split(vae):
    """Build the split fp16 weights of every convolution of an fp32 VAE that can take the split-operand path NOW (model load), so that
    the one host synchronisation of ``ops.split_conv_weight`` (the weight's absolute maximum) never falls into a forward -- or a stream
    capture -- later.  A no-op for a CPU / 16-bit VAE or with the switch off; a weight that changes afterwards is re-split
    on its next use (``_derived``'s key)."""
    if not (VAE_SPLIT_CONV and FUSED_KERNELS):
        return 0
    n = 0
    for m in vae.modules():
        convs = ()
        if isinstance(m, ResnetBlock2D) and m.time_emb_proj is None:
            convs = (m.conv1, m.conv2)
        elif isinstance(m, Upsample2D) and m.vae:
            convs = (m.conv,)
        elif isinstance(m, Downsample2D) and m.padding == 0:     # the VAE encoder's downsamplers (VAE_SPLIT_DOWNSAMPLE)
            convs = (m.conv,)
        for c in convs:
            w = c.weight
            if w.is_cuda and w.dtype == torch.float32 and w.shape[1] % 64 == 0 and w.shape[0] % 8 == 0 and tuple(w.shape[2:]) == (3, 3):
                _split_weight(c)
                n += 1
    return n


def layer_norm(norm, x):
    """LayerNorm over the last dim.  HIP: ed_layernorm (one wave per row); torch otherwise."""
    D = x.shape[-1]
    if norm.elementwise_affine and _stream32(x, norm.weight.dtype):   # fp32 residual stream -> model dtype
        if FUSED_LAYERNORM and FUSED_KERNELS and x.is_cuda and x.is_contiguous() and D % 8 == 0 and D <= 2048:
            return ops.layernorm_s32(x, norm.weight, norm.bias, norm.eps)
        return F.layer_norm(x, (D,), *_f32_params(norm), norm.eps).to(norm.weight.dtype)
    if FUSED_LAYERNORM and _fusable(x) and D % 8 == 0 and D <= 2048 and norm.elementwise_affine:
        return ops.layernorm(x, norm.weight, norm.bias, norm.eps)
    return norm(x)


def add_layer_norm(norm, a, b):
    """(a + b, LayerNorm(a + b)).  HIP: ed_add_layernorm; torch otherwise."""
    D = a.shape[-1]
    if (FUSED_ADD_LAYERNORM and _fusable(a) and _fusable(b) and a.shape == b.shape and D % 8 == 0 and D <= 2048
            and norm.elementwise_affine):
        return ops.add_layernorm(a, b, norm.weight, norm.bias, norm.eps)
    if (FUSED_ADD_LAYERNORM and FUSED_KERNELS and norm.elementwise_affine and _fusable(a) and _stream32(b, a.dtype) and b.is_cuda
            and b.is_contiguous() and a.shape == b.shape and D % 8 == 0 and D <= 2048 and norm.weight.dtype == a.dtype):
        # fp32 residual stream: 16-bit branch result + fp32 stream -> (fp32 stream, 16-bit LayerNorm)
        return ops.add_layernorm_s32(a, b, norm.weight, norm.bias, norm.eps)
    s = a + b          # (fp32 residual stream: a 16-bit branch result + the fp32 stream -> fp32)
    return s, layer_norm(norm, s)


class ModelOutput(dict):
    """``out['sample']`` and ``out.sample`` (the reference indexes the former, ED:422)."""

    __getattr__ = dict.__getitem__


# ---------------------------------------------------------------------------------------------------
# shared blocks
# ---------------------------------------------------------------------------------------------------
def timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=0.0, max_period=10000.0):
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device) / (half - freq_shift)
    emb = t[:, None].float() * torch.exp(exponent)[None, :]
    sin, cos = torch.sin(emb), torch.cos(emb)
    return torch.cat([cos, sin], dim=-1) if flip_sin_to_cos else torch.cat([sin, cos], dim=-1)


class TimestepEmbedding(nn.Module):
    def __init__(self, in_dim, dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_dim, dim)
        self.linear_2 = nn.Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(F.silu(self.linear_1(x)))


# 1x1 shortcut convolutions as one strided-batched GEMM with the residual folded in (beta = 1): replaces MIOpen's
# im2col + GEMM + bias kernels and the separate residual add.  Toggle for A/B measurements.
SHORTCUT_AS_GEMM = False  # measured on MI355X: 233.1 vs 231.1 ms at B=20 -- no gain over MIOpen + add, kept for A/B


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb_dim=None, eps=1e-5, groups=32):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = nn.Linear(temb_dim, cout) if temb_dim else None
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x, temb=None):
        if _vae_split_ok(x, self):
            return self._forward_split(x)
        tb = self.time_emb_proj(F.silu(temb)) if self.time_emb_proj is not None else None
        sc, c1, c2 = self.conv_shortcut, self.conv1, self.conv2
        cout = c1.out_channels
        if _narrowed_encode_active():
            # AutoencoderKL.encode_constant off the split path (CPU, fp64, a 16-bit VAE, VAE_SPLIT_CONV off): the plain block -- the
            # weighted GroupNorm folds no bias in and returns NCHW, which the fused branches below do not take
            h = c1(group_norm_act(self.norm1, x, silu=True))
            return (x if sc is None else sc(x)) + c2(group_norm_act(self.norm2, h, silu=True))
        if _stream32(x, c1.weight.dtype):
            # fp32 residual stream (UNet2DConditionModel.residual_fp32): both branches in the model dtype -- the same GroupNorm -> convolution
            # kernels from norm1's output on -- and ONE fp32 add onto the stream
            def add_to_stream(h):
                if sc is None:
                    return x + h
                xs = x.to(h.dtype)
                return (_shortcut_nhwc(sc, xs) if ops.is_nhwc(xs) else sc(xs)).float() + h

            def close(a2):
                B, _, H, W = a2.shape
                if a2.dtype == torch.float16 and ops.conv3x3_f32out_ok(B, H, W, cout, cout):
                    # conv2 through the fp32-output epilogue (ed_conv3x3_nhwc_f32out: fp16 operands, fp32 bias / residual / result): the
                    # branch result is never rounded to 16 bits and the add onto the stream costs no pass of its own
                    res = x if sc is None else _shortcut_nhwc(sc, x.to(a2.dtype)).float()
                    res = res.contiguous(memory_format=torch.channels_last)
                    return ops.conv3x3_f32out(a2, c2.weight, _f32_bias(c2), res, 1.0)
                return add_to_stream(ops.conv3x3_nhwc(a2, c2.weight, c2.bias))

            a = group_norm_act(self.norm1, x, silu=True)
            if _hip_conv_pair(self, a, a.shape[1]):
                return self._hip_convs(a, tb, close)
            return add_to_stream(c2(group_norm_act(self.norm2, c1(a), silu=True, chan_bias=tb)))
        cl = _fusable_nhwc(x) and cout % 8 == 0 and cout // self.norm2.num_groups >= 8
        # norm1 must take the channels-last HIP kernel as well
        if x.shape[1] // self.norm1.num_groups >= 8 and _hip_conv_pair(self, x, x.shape[1]):
            return self._hip_convs(group_norm_act(self.norm1, x, silu=True), tb, lambda a2: ops.conv3x3_nhwc(
                a2, c2.weight, c2.bias, residual=x if sc is None else _shortcut_nhwc(sc, x)))
        if FUSED_CONV_BIAS and FUSED_TEMB_ADD and (cl or (_fusable(x) and (x.shape[2] * x.shape[3]) % 8 == 0)):
            # MIOpen adds a convolution's bias with a separate broadcast kernel: run the convolutions bias-free and fold
            # conv1's bias (+ temb) into norm2's passes, conv2's and the shortcut's into the closing residual add
            h = F.conv2d(group_norm_act(self.norm1, x, silu=True), c1.weight, None, padding=1)
            a = group_norm_act(self.norm2, h, silu=True, chan_bias=tb, conv_bias=c1.bias)
            h = F.conv2d(a, c2.weight, None, padding=1)
            if sc is None:
                return ops.bias_residual_add(h, c2.bias, x)
            if cl:  # channels-last: the 1x1 shortcut is a plain GEMM over the token view, no layout change
                res = F.linear(x.permute(0, 2, 3, 1), sc.weight.reshape(cout, -1)).permute(0, 3, 1, 2)
            else:
                res = F.conv2d(x, sc.weight, None)
            return ops.bias_residual_add(h, c2.bias, res, sc.bias)
        h = c1(group_norm_act(self.norm1, x, silu=True))
        a = group_norm_act(self.norm2, h, silu=True, chan_bias=tb)  # GroupNorm(h + temb) (+SiLU)
        if sc is not None and SHORTCUT_AS_GEMM and _fusable(x):
            # out = W_sc x + (conv2(a) + b_conv2 + b_sc): the shortcut bias rides on conv2's bias, the residual sum is
            # the GEMM's C operand
            N, C, H, W = x.shape
            h = F.conv2d(a, c2.weight, c2.bias + sc.bias, padding=1)
            w = sc.weight.view(1, cout, C).expand(N, -1, -1)
            return torch.baddbmm(h.view(N, cout, H * W), w, x.view(N, C, H * W)).view(N, cout, H, W)
        return (x if sc is None else sc(x)) + c2(a)

    def _hip_convs(self, a, tb, close):
        """Both convolutions as ed_conv3x3_nhwc from ``a`` = SiLU(norm1(.)) on (``_hip_conv_pair``): conv1's epilogue adds its bias and the
        time embedding, norm2 is the channels-last kernel, and ``close(SiLU(norm2(.)))`` is the caller's conv2, whose epilogue adds its
        bias and the block's residual -- the two broadcast adds and the closing add never exist as separate passes"""
        h = ops.conv3x3_nhwc(a, self.conv1.weight, self.conv1.bias, sample_bias=None if tb is None else tb.contiguous())
        return close(group_norm_act(self.norm2, h, silu=True))

    def forward_cat(self, x, skip, temb=None):
        """``self(torch.cat([x, skip], 1), temb)`` -- the up blocks' call -- without writing the concatenation (round 6): norm1 reads the two
        channels-last sources in place (ed_groupnorm_nhwc_cat, bit-identical to the kernel on the materialised cat) and the 1x1 shortcut is
        split along K, W_sc [x | skip] = W_1 x + W_2 skip: the second product accumulates onto the first (ed_linear's residual epilogue or
        the library's beta = 1), which rounds the first partial sum to 16 bits once -- the only arithmetic difference from the cat path.
        Everything else is ``forward``'s channels-last HIP path; any shape / layout it does not take falls back to the concatenation."""
        sc, c2 = self.conv_shortcut, self.conv2
        C1, C = x.shape[1], x.shape[1] + skip.shape[1]
        if (FUSED_SKIP_CAT and FUSED_KERNELS and sc is not None and _fusable_nhwc(skip) and x.dtype == skip.dtype
                and _hip_conv_pair(self, x, C) and ops.groupnorm_nhwc_cat_ok(x, skip, self.norm1.num_groups)
                and self.conv1.weight.shape[1] == C and sc.weight.dtype == x.dtype):
            def close(a2):
                w1, w2 = _split_shortcut(sc, C1)
                xt, st = x.permute(0, 2, 3, 1), skip.permute(0, 2, 3, 1)          # contiguous [N, H, W, C] views of channels-last memory
                y = linear_(xt, w1, sc.bias)
                M, cout = st.numel() // st.shape[-1], w2.shape[0]
                if HIP_LINEAR and ops.linear_wins(M, st.shape[-1], cout):
                    y = ops.linear(st, w2, None, residual=y)
                else:
                    y = torch.addmm(y.reshape(M, cout), st.reshape(M, -1), w2.t()).view(y.shape)
                return ops.conv3x3_nhwc(a2, c2.weight, c2.bias, residual=y.permute(0, 3, 1, 2))

            tb = self.time_emb_proj(F.silu(temb)) if self.time_emb_proj is not None else None
            n1 = self.norm1
            return self._hip_convs(ops.groupnorm_nhwc_cat(x, skip, n1.weight, n1.bias, n1.num_groups, n1.eps, silu=True), tb, close)
        return self(torch.cat([x, skip], dim=1), temb)

    def _forward_split(self, x):
        """The fp32 VAE block with both 3x3 convolutions on the MFMA pipe (VAE_SPLIT_CONV): GroupNorm + SiLU write the split fp16 operand,
        the convolution's fp32 epilogue adds the bias and (conv2) the block's residual.  Batches whose operand would exceed the kernel's
        32-bit offsets are processed in slices (GroupNorm is per sample)."""
        n1, n2, sc = self.norm1, self.norm2, self.conv_shortcut
        _, cin, H, W = x.shape

        wx, wy, _ = _plane_weights(x)    # the narrowed constant-image encode: weighted statistics (None, None otherwise)

        def block(xs):
            w1, s1 = _split_weight(self.conv1)
            w2, s2 = _split_weight(self.conv2)
            a = ops.groupnorm_nhwc_f32(xs, n1.weight, n1.bias, n1.num_groups, n1.eps, silu=True, split=True, wx=wx, wy=wy)
            h = ops.conv3x3_f32out(a, w1, self.conv1.bias, None, s1)
            a = ops.groupnorm_nhwc_f32(h, n2.weight, n2.bias, n2.num_groups, n2.eps, silu=True, split=True, wx=wx, wy=wy)
            res = xs if sc is None else _shortcut_nhwc(sc, xs)    # 1x1 convolution = an fp32 GEMM over the NHWC view
            return ops.conv3x3_f32out(a, w2, self.conv2.bias, res, s2)

        per = H * W * 3 * max(cin, self.conv1.out_channels) * 2
        return _sliced(x.contiguous(memory_format=torch.channels_last), max(1, (2 ** 31 - 16) // per), block)


class Attention(nn.Module):
    def __init__(self, dim, heads, head_dim, cross_dim=None, bias=False):
        super().__init__()
        inner = heads * head_dim
        self.heads = heads
        self.to_q = nn.Linear(dim, inner, bias=bias)
        self.to_k = nn.Linear(cross_dim or dim, inner, bias=bias)
        self.to_v = nn.Linear(cross_dim or dim, inner, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(inner, dim), nn.Dropout(0.0)])
        # IP-Adapter (UNet2DConditionModel.install_ip_adapter): the last ``ip_tokens`` context rows are
        # image tokens with projections and a softmax of their own.  0 / None: the attention is what it always was.
        self.to_k_ip = self.to_v_ip = None
        self.ip_tokens = 0
        self.ip_scale = 1.0
        # Several adapters: ``ip_segments`` = every adapter's token count in context order (``ip_tokens`` is
        # their sum); adapter a >= 1 lives in ``to_k_ip_{a}`` / ``to_v_ip_{a}``; ``ip_weights`` is the UNet's one fp32 device tensor
        # [A] that replaces the by-value ``ip_scale`` from two adapters on.
        self.ip_segments = ()
        self.ip_weights = None
        # Attention masks: (m f32 [B, A, S], PH, PW, w f32 [A]) for the duration of one
        # ``UNet2DConditionModel.forward(ip_masks=)``, None otherwise -- and then every branch below is what it was.
        self.ip_mask = None

    def _ip_mask_level(self, B, N):
        """the level of the mask pyramid a cross attention of ``N`` query rows reads: a view [B, A, N] of the rows' buffer"""
        m, PH, PW, _ = self.ip_mask
        if m.shape[0] != B:
            raise ValueError(f"ip_masks holds {m.shape[0]} rows, the batch {B}")
        for off, n in ops.ip_mask_layout(PH, PW)[0]:
            if n == N:
                return m[:, :, off:off + n]
        raise ValueError(f"a cross attention with {N} query rows matches no level of the {PH} x {PW} mask pyramid "
                         f"({[n for _, n in ops.ip_mask_layout(PH, PW)[0]]})")

    @staticmethod
    def ip_names(a):
        return ("to_k_ip", "to_v_ip") if a == 0 else (f"to_k_ip_{a}", f"to_v_ip_{a}")

    def set_ip_adapter(self, to_k_ip=None, to_v_ip=None, tokens=0):
        """install (two bias-free Linear(cross_dim, inner) and the image-token count) as the ONLY adapter or, without arguments,
        remove every adapter"""
        for a in range(1, len(self.ip_segments)):
            for name in self.ip_names(a):
                delattr(self, name)
        for name, mod in (("to_k_ip", to_k_ip), ("to_v_ip", to_v_ip)):
            if isinstance(getattr(self, name), nn.Module):
                delattr(self, name)     # out of _modules, so the key leaves state_dict()
            setattr(self, name, mod)
        self.ip_tokens = int(tokens) if to_k_ip is not None else 0
        self.ip_segments = (self.ip_tokens,) if self.ip_tokens else ()
        self.ip_weights = None
        self.__dict__.pop("_derived", None)

    def add_ip_adapter(self, to_k_ip, to_v_ip, tokens, weights):
        """append one more adapter behind the installed one(s); ``weights``: the fp32 tensor [A] all layers of the model share"""
        a = len(self.ip_segments)
        if a == 0:
            raise ValueError("add_ip_adapter appends to an installed adapter: use set_ip_adapter for the first")
        for name, mod in zip(self.ip_names(a), (to_k_ip, to_v_ip)):
            setattr(self, name, mod)
        self.ip_segments = self.ip_segments + (int(tokens),)
        self.ip_tokens = sum(self.ip_segments)
        self.ip_weights = weights
        self.__dict__.pop("_derived", None)

    def _ip_rows(self, n):
        """[(first row, one past the last)] of every adapter's rows in a context / k|v of ``n`` rows"""
        out, off = [], n - self.ip_tokens
        for ni in self.ip_segments:
            out.append((off, off + ni))
            off += ni
        return out

    def _fused_weight(self, names, q_scale=None):
        """cat of the projection weights (bias-free in every SD / SDXL attention).
        ``q_scale``: factor folded into the first (query) weight -- softmax scale * log2 e for the exponent-domain attention
        kernel (ops.flash_prescale): the product is formed in fp32 and rounded once, so the scaled 16-bit weight is as close
        to c * W as the stored one is to W."""
        ws = [getattr(self, n).weight for n in names]

        def build():
            parts = [w.detach() for w in ws]
            if q_scale is not None:
                parts[0] = (parts[0].float() * q_scale).to(parts[0].dtype)
            return torch.cat(parts, dim=0).contiguous()
        return _derived(self, (names, q_scale), ws, build)

    def project_kv(self, context, out=None):
        """k, v of a cross-attention as ONE [B, Nk, 2 inner] tensor (fused weight).  They depend on the text rows only -- not on
        the latent, not on the timestep -- so a caller may compute them once per image and hand them to ``forward`` (``kv``)
        instead of re-projecting the same text tokens in every one of the ~100 forwards of an image (UNet.cross_attention_kv)."""
        w = self._fused_weight(("to_k", "to_v"))
        if out is None:   # the same library call for the first projection and every refresh: one hipBLASLt solution, same bits
            out = torch.empty(context.shape[:-1] + (w.shape[0],), dtype=context.dtype, device=context.device)
        if self.ip_tokens:
            # [text rows | image rows]: the text rows through to_k|to_v, the image rows through to_k_ip|to_v_ip, into one tensor
            # (rows in the order ed_flash_attention_ip reads them).  Same calls for the first projection and every refresh.
            nt = context.shape[-2] - self.ip_tokens
            out[..., :nt, :] = torch.matmul(context[..., :nt, :], w.t())
            if len(self.ip_segments) < 2:
                out[..., nt:, :] = torch.matmul(context[..., nt:, :], self._fused_weight(("to_k_ip", "to_v_ip")).t())
                return out
            for a, (lo, hi) in enumerate(self._ip_rows(context.shape[-2])):   # each adapter's rows through its own fused weight
                out[..., lo:hi, :] = torch.matmul(context[..., lo:hi, :], self._fused_weight(self.ip_names(a)).t())
            return out
        torch.matmul(context, w.t(), out=out)
        return out

    def forward(self, x, context=None, kv=None, residual=None):
        """``residual`` given: -> (out, fused) -- out = residual + attention(...) when the output projection took the add (fused), else the
        plain attention output and the caller adds."""
        out, fused = self._attend(x, context, kv, residual)
        return out if residual is None else (out, fused)

    def _attend(self, x, context, kv, residual):
        """-> (attention output, did to_out[0] add ``residual`` in its epilogue?)"""
        B, N, _ = x.shape
        inner = self.to_q.out_features
        if (FLASH_ATTENTION and _fusable(x) and inner % self.heads == 0 and inner // self.heads in (40, 64, 80, 160)
                and self.to_q.bias is None
                and (context is None or (_fusable(context) and context.dtype == x.dtype))):
            if context is None:
                # exponent-domain kernel: softmax scale * log2 e lives in the query weights (None: natural-domain q)
                c = ops.flash_prescale(N, N, 3 * inner if FUSED_QKV else inner) if inner == self.heads * 64 else None
                if FUSED_QKV:
                    qkv = linear_(x, self._fused_weight(("to_q", "to_k", "to_v"), c))
                    q, k, v = qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
                else:
                    q = linear_(x, self.to_q.weight if c is None else self._fused_weight(("to_q",), c))
                    k, v = self.to_k(x), self.to_v(x)
                o = ops.flash_attention(q, k, v, self.heads, prescaled=c is not None)
            elif self.ip_tokens:
                # decoupled cross attention: one launch where ed_flash_attention_ip takes the shape (head dim 64, <= 160 text keys),
                # else the two attentions through the existing kernels and a torch axpy (correct, not fused)
                q = linear_(x, self.to_q.weight)
                if kv is None:
                    kv = self.project_kv(context)
                k, v = kv[..., :inner], kv[..., inner:]
                nt = kv.shape[1] - self.ip_tokens
                if self.ip_mask is not None:
                    # masked image prompts (section 33), any adapter count: one ed_flash_attention_ipm launch where it takes the shape,
                    # else A + 1 attentions combined with DEVICE tensors only -- a replayed graph follows new masks and scales
                    mv, w = self._ip_mask_level(B, N), self.ip_mask[3]
                    if ops.flash_attention_ipm_ok(inner // self.heads, nt, self.ip_segments):
                        o = ops.flash_attention_ipm(q, k, v, self.heads, nt, self.ip_segments, w, mv)
                    else:
                        o = ops.flash_attention(q, k[:, :nt], v[:, :nt], self.heads)
                        wd = w.to(o.dtype)
                        for a, (lo, hi) in enumerate(self._ip_rows(kv.shape[1])):
                            o_a = ops.flash_attention(q, k[:, lo:hi], v[:, lo:hi], self.heads)
                            # o + (w[a] m_a) o_a as section 32's addcmul: at m == 1 the bits of the unmasked fallback
                            o = o.addcmul_(o_a, (wd[a] * mv[:, a].to(o.dtype))[..., None])
                elif len(self.ip_segments) >= 2:
                    # several adapters: one ed_flash_attention_ipn launch where it takes the shape, else A + 1 attentions combined
                    # with the DEVICE weights by a tensor multiply -- never a Python float, so a replayed graph follows a new scale
                    if ops.flash_attention_ipn_ok(inner // self.heads, nt, self.ip_segments):
                        o = ops.flash_attention_ipn(q, k, v, self.heads, nt, self.ip_segments, self.ip_weights)
                    else:
                        o = ops.flash_attention(q, k[:, :nt], v[:, :nt], self.heads)
                        wd = self.ip_weights.to(o.dtype)
                        for a, (lo, hi) in enumerate(self._ip_rows(kv.shape[1])):
                            o = o.addcmul_(ops.flash_attention(q, k[:, lo:hi], v[:, lo:hi], self.heads), wd[a])
                elif ops.flash_attention_ip_ok(inner // self.heads, nt, self.ip_tokens):
                    o = ops.flash_attention_ip(q, k, v, self.heads, nt, self.ip_scale)
                else:
                    o = ops.flash_attention(q, k[:, :nt], v[:, :nt], self.heads)
                    o = o.add_(ops.flash_attention(q, k[:, nt:], v[:, nt:], self.heads), alpha=self.ip_scale)
            else:
                q = linear_(x, self.to_q.weight)
                if kv is not None or FUSED_QKV:
                    if kv is None:
                        kv = self.project_kv(context)
                    k, v = kv[..., :inner], kv[..., inner:]
                else:
                    k, v = self.to_k(context), self.to_v(context)
                o = ops.flash_attention(q, k, v, self.heads)
            # the block's residual in to_out[0]'s epilogue when one is given and ed_linear runs this shape
            return linear_res_(o, self.to_out[0].weight, self.to_out[0].bias, residual)
        ctx = x if context is None else context
        q = self.to_q(x).view(B, N, self.heads, -1).transpose(1, 2)
        if context is not None and self.ip_tokens:
            if kv is None:
                kv = self.project_kv(ctx)
            nt = kv.shape[1] - self.ip_tokens
            k, v = (t.reshape(B, kv.shape[1], self.heads, -1).transpose(1, 2) for t in (kv[..., :inner], kv[..., inner:]))
            o = F.scaled_dot_product_attention(q, k[:, :, :nt], v[:, :, :nt])
            if self.ip_mask is not None:
                mv, wd = self._ip_mask_level(B, N), self.ip_mask[3].to(o.dtype)
                for a, (lo, hi) in enumerate(self._ip_rows(kv.shape[1])):
                    o_a = F.scaled_dot_product_attention(q, k[:, :, lo:hi], v[:, :, lo:hi])
                    o = o + (wd[a] * mv[:, a].to(o.dtype))[:, None, :, None] * o_a
            elif len(self.ip_segments) >= 2:
                wd = self.ip_weights.to(o.dtype)
                for a, (lo, hi) in enumerate(self._ip_rows(kv.shape[1])):
                    o = o + wd[a] * F.scaled_dot_product_attention(q, k[:, :, lo:hi], v[:, :, lo:hi])
            else:
                o = o + self.ip_scale * F.scaled_dot_product_attention(q, k[:, :, nt:], v[:, :, nt:])
            return self.to_out[0](o.transpose(1, 2).reshape(B, N, -1)), False
        if kv is not None:
            k, v = (t.reshape(B, ctx.shape[1], self.heads, -1).transpose(1, 2) for t in (kv[..., :inner], kv[..., inner:]))
        else:
            k = self.to_k(ctx).view(B, ctx.shape[1], self.heads, -1).transpose(1, 2)
            v = self.to_v(ctx).view(B, ctx.shape[1], self.heads, -1).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)
        return self.to_out[0](o.transpose(1, 2).reshape(B, N, -1)), False


class GEGLU(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.proj = nn.Linear(dim, inner * 2)

    def forward(self, x):
        if (HIP_GEGLU_GEMM and FUSED_KERNELS and _fusable(x) and self.proj.weight.dtype == x.dtype
                and ops.geglu_gemm_wins(x.numel() // x.shape[-1], x.shape[-1], self.proj.out_features // 2)):
            return ops.geglu_gemm(x, self.proj.weight, self.proj.bias)
        y = self.proj(x)
        if _fusable(y) and (y.shape[-1] // 2) % 8 == 0:
            return ops.geglu(y, y.shape[-1] // 2)
        h, gate = y.chunk(2, dim=-1)
        return h * F.gelu(gate)


class FeedForward(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * 4), nn.Dropout(0.0), nn.Linear(dim * 4, dim)])

    def forward(self, x, residual=None):
        if residual is not None:     # -> (out, fused): out = residual + ff(x) when the second projection took the add
            return linear_res_(self.net[0](x), self.net[2].weight, self.net[2].bias, residual)
        return linear_(self.net[0](x), self.net[2].weight, self.net[2].bias)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, heads, head_dim, cross_dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, heads, head_dim)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = Attention(dim, heads, head_dim, cross_dim)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)

    def forward(self, x, context, pending=None, kv=None):
        """-> (ff_out, x): the block's output is ``ff_out + x``; the caller either hands the pair to the next block
        (whose norm1 then runs fused with that add) or sums it -- or (None, x) when the feed-forward's second projection already
        added (FUSED_RESIDUAL_LINEAR: wherever ed_linear runs a residual-producing projection the add rides in its epilogue and the
        next LayerNorm is a plain one).  ``pending``: the previous block's ff_out.  ``kv``: dict
        {id(attention module): precomputed k|v} (UNet.cross_attention_kv) or None."""
        if pending is not None:
            x, h = add_layer_norm(self.norm1, pending, x)                 # x = prev_ff + x ; norm1(x)
        else:
            h = layer_norm(self.norm1, x)
        a, fused = self.attn1(h, residual=x)                              # x = attn1(norm1(x)) + x ; norm2(x)
        x, h = (a, layer_norm(self.norm2, a)) if fused else add_layer_norm(self.norm2, a, x)
        a, fused = self.attn2(h, context, None if kv is None else kv.get(id(self.attn2)), residual=x)   # x = attn2(norm2(x)) + x ; norm3(x)
        x, h = (a, layer_norm(self.norm3, a)) if fused else add_layer_norm(self.norm3, a, x)
        a, fused = self.ff(h, residual=x)
        return (None, a) if fused else (a, x)                              # (None, x): the add already happened in ff's projection


class Transformer2DModel(nn.Module):
    def __init__(self, ch, heads, depth, cross_dim, linear_proj):
        super().__init__()
        self.linear_proj = linear_proj
        self.norm = nn.GroupNorm(32, ch, eps=1e-6)
        self.proj_in = nn.Linear(ch, ch) if linear_proj else nn.Conv2d(ch, ch, 1)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(ch, heads, ch // heads, cross_dim) for _ in range(depth)])
        self.proj_out = nn.Linear(ch, ch) if linear_proj else nn.Conv2d(ch, ch, 1)

    def forward(self, x, context, kv=None):
        B, C, H, W = x.shape
        if self.linear_proj:
            h = linear_(group_norm_act(self.norm, x, tokens=True), self.proj_in.weight, self.proj_in.bias)
        else:
            # the blocks' LayerNorm kernels need a contiguous token tensor (.contiguous() is a no-op on a channels-last activation)
            h = self.proj_in(group_norm_act(self.norm, x)).permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
        s32 = _stream32(x, self.proj_out.weight.dtype)
        if s32:
            h = h.float()      # the blocks' own residual stream in fp32 as well (their LayerNorms hand the model dtype to the branches)
        pend = None
        for blk in self.transformer_blocks:
            pend, h = blk(h, context, pend, kv)
        if pend is not None:
            h = pend + h
        if s32:
            h = h.to(self.proj_out.weight.dtype)
        if self.linear_proj:
            if (FUSED_PROJ_OUT_ADD and HIP_LINEAR and FUSED_KERNELS and _fusable_nhwc(x) and _fusable(h) and self.proj_out.weight.dtype == x.dtype == h.dtype
                    and self.proj_out.weight.is_contiguous() and ops.linear_wins(B * H * W, C, C)):
                # channels-last: x's memory IS the token layout, so the block's closing `x + proj_out(h)` rides in ed_linear's residual
                # epilogue (one rounding of bias + product + residual instead of two) -- no separate add pass
                y = ops.linear(h, self.proj_out.weight, self.proj_out.bias, residual=x.permute(0, 2, 3, 1).reshape(B, H * W, C))
                return y.view(B, H, W, C).permute(0, 3, 1, 2)
            h = linear_(h, self.proj_out.weight, self.proj_out.bias)
            if (FUSED_TOKENS_ADD and _fusable(x) and _fusable(h) and C % 64 == 0 and (H * W) % 64 == 0):
                return ops.tokens_add_nchw(x, h)  # x + h^T in one pass through an LDS tile
            h = h.view(B, H, W, C).permute(0, 3, 1, 2)
        else:
            h = self.proj_out(h.view(B, H, W, C).permute(0, 3, 1, 2))
        return x + h  # x first: the sum keeps x's NCHW layout (a permuted first operand would make it channels-last)


class Downsample2D(nn.Module):
    def __init__(self, ch, padding=1):
        super().__init__()
        self.padding = padding
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=padding)

    def forward(self, x):
        if _stream32(x, self.conv.weight.dtype):   # fp32 residual stream: the convolution in the model dtype, its result widened (exact)
            return self.forward(x.to(self.conv.weight.dtype)).float()
        if self.padding == 0 and VAE_SPLIT_CONV and VAE_SPLIT_DOWNSAMPLE and FUSED_KERNELS and x.is_cuda and x.dtype == torch.float32 \
                and x.dim() == 4 and self.conv.weight.dtype == torch.float32:
            # the VAE encoder's downsampler on the MFMA pipe (round 6): the raw stream is split like the decoder's upsampler input (per-tensor
            # power-of-two scale from its absolute maximum), the pad-(0, 1, 0, 1) stride-2 convolution is template value CONV = 4 of the
            # split-operand main loop; channels-last in and out -- no NCHW copies around the library call
            B, C, H, W = x.shape
            if C % 64 == 0 and ops.conv3x3_f32out_s2_ok(1, H, W, 3 * C, self.conv.weight.shape[0]):
                w, sc = _split_weight(self.conv)

                def conv(xs):
                    am = ops.absmax_f32(xs)
                    return ops.conv3x3_f32out_s2(ops.split_f32(xs, absmax=am), w, self.conv.bias, sc, act_absmax=am)
                return _sliced(x.contiguous(memory_format=torch.channels_last), max(1, (2 ** 31 - 16) // (H * W * 3 * C * 2)), conv)
        if self.padding == 0:  # VAE encoder: asymmetric pad (diffusers Downsample2D)
            x = F.pad(_to_nchw(x), (0, 1, 0, 1))
        if HIP_DOWNSAMPLE_CONV and HIP_CONV3X3 and self.padding == 1 and _fusable_nhwc(x) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
            w = self.conv.weight
            B, C, H, W = x.shape
            if w.dtype == x.dtype and w.is_contiguous(memory_format=torch.channels_last) and ops.conv3x3_s2_wins(B, H // 2, W // 2, C, w.shape[0]):
                return ops.conv3x3_nhwc_s2(x, w, self.conv.bias)       # the stride-2 convolution on the MFMA main loop
        return self.conv(x)


class Upsample2D(nn.Module):
    def __init__(self, ch, vae=False):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)
        self.vae = vae   # the VAE decoder's upsampler (the split-operand path is the VAE's; an fp32 UNet stays plain torch: it is the
                         # tolerance reference of bench.py's fp32 leg and of the parity tests)

    def _split_ok(self, x):
        """fp32 VAE, channels % 64 == 0, and ONE sample's upsampled split operand within the kernel's 32-bit offsets (the 1024 x 2048
        decode's last upsampler -- [1, 768, 1024, 2048] fp16 = 3.2 GB -- is not: it stays with the library)"""
        if not (self.vae and VAE_SPLIT_CONV and FUSED_KERNELS and x.is_cuda and x.dim() == 4 and self.conv.weight.dtype == torch.float32):
            return False
        B, C, H, W = x.shape
        return C % 64 == 0 and 4 * H * W * 3 * C * 2 < 2 ** 31 - 16     # per sample; larger batches are processed in slices

    def forward(self, x):
        if _stream32(x, self.conv.weight.dtype):   # fp32 residual stream of a 16-bit UNet
            return self.forward(x.to(self.conv.weight.dtype)).float()
        if x.dtype == torch.float32:
            if self._split_ok(x):
                # the VAE decoder's upsampler on the MFMA pipe (VAE_SPLIT_CONV): the raw stream is split (scaled by a per-tensor power of
                # two taken from its absolute maximum on the device: the real decoder stream leaves fp16's range) and upsampled in one pass, the convolution is the same split-operand main loop as the ResnetBlocks'; channels-last in and out
                w, sc = _split_weight(self.conv)
                B, C, H, W = x.shape

                def conv(xs):
                    am = ops.absmax_f32(xs)     # per-slice power-of-two scale: the split is exact over the whole fp32 range
                    return ops.conv3x3_f32out(ops.split_f32(xs, upsample2x=True, absmax=am), w, self.conv.bias, None, sc, act_absmax=am)
                return _sliced(x.contiguous(memory_format=torch.channels_last), max(1, (2 ** 31 - 16) // (4 * H * W * 3 * C * 2)), conv)
            x = _to_nchw(x)  # NCHW for MIOpen's fp32 solvers (the UNet's 16-bit activations stay channels-last)
        if FUSED_UPSAMPLE_CONV and HIP_CONV3X3 and _fusable_nhwc(x):
            w = self.conv.weight
            B, C, H, W = x.shape
            if w.dtype == x.dtype and w.is_contiguous(memory_format=torch.channels_last) and ops.conv3x3_up2x_wins(B, 2 * H, 2 * W, C, w.shape[0]):
                return ops.conv3x3_nhwc_up2x(x, w, self.conv.bias)   # the upsampled tensor (4x the source) is never written
        up = F.interpolate(x, scale_factor=2.0, mode="nearest")
        if _fusable_nhwc(up) and _hip_conv3x3(self.conv, up, up.shape[1]):
            return ops.conv3x3_nhwc(up, self.conv.weight, self.conv.bias)
        return self.conv(up)


# ---------------------------------------------------------------------------------------------------
# UNet2DConditionModel
# ---------------------------------------------------------------------------------------------------
UNET_CONFIGS = {
    "sd15": dict(sample_size=64, in_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                 attn=(True, True, True, False), transformer_depth=(1, 1, 1, 1), heads=(8, 8, 8, 8),
                 cross_attention_dim=768, use_linear_projection=False, addition_time_embed_dim=None,
                 pooled_projection_dim=None),
    "sd2": dict(sample_size=64, in_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                attn=(True, True, True, False), transformer_depth=(1, 1, 1, 1), heads=(5, 10, 20, 20),
                cross_attention_dim=1024, use_linear_projection=True, addition_time_embed_dim=None,
                pooled_projection_dim=None),
    "sdxl": dict(sample_size=128, in_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
                 attn=(False, True, True), transformer_depth=(1, 2, 10), heads=(5, 10, 20),
                 cross_attention_dim=2048, use_linear_projection=True, addition_time_embed_dim=256,
                 pooled_projection_dim=1280),
}


# Reduced-width variants of the same architectures (same block structure, attention placement, projection kind, head
# dim 64, added-condition path): small enough that the fp32 CPU oracle runs them in seconds, so the parity tests and
# bench.py's parity leg can put the REAL module code (not a stand-in) inside an oracle-checked denoising loop.
SMALL_UNET_CONFIGS = {
    "sd15": dict(sample_size=64, in_channels=4, block_out_channels=(64, 128, 256, 256), layers_per_block=2,
                 attn=(True, True, True, False), transformer_depth=(1, 1, 1, 1), heads=(1, 2, 4, 4),
                 cross_attention_dim=64, use_linear_projection=False, addition_time_embed_dim=None,
                 pooled_projection_dim=None),
    "sdxl": dict(sample_size=128, in_channels=4, block_out_channels=(64, 128, 256), layers_per_block=2,
                 attn=(False, True, True), transformer_depth=(1, 1, 2), heads=(1, 2, 4),
                 cross_attention_dim=64, use_linear_projection=True, addition_time_embed_dim=16,
                 pooled_projection_dim=32),
}
SMALL_VAE_CHANNELS = (32, 64, 64, 64)

# Inpainting checkpoints (stable-diffusion-inpainting, stable-diffusion-2-inpainting, stable-diffusion-xl-1.0-inpainting-0.1): the
# same architectures with a 9-channel ``conv_in`` -- noisy latent (4) | latent mask (1) | masked-image latent (4), DESIGN.md section
# 22.  Only conv_in's input width differs, so every dispatch rule above applies unchanged (conv_in is library work at either width).
INPAINT_IN_CHANNELS = 9
INPAINT_SUFFIX = "-inpaint"


def unet_config(fam, small=False, in_channels=4):
    """The UNet configuration of a family at full or reduced width, with 4 (text-to-image) or 9 (inpainting) input channels."""
    if in_channels not in (4, INPAINT_IN_CHANNELS):
        raise ValueError(f"in_channels must be 4 or {INPAINT_IN_CHANNELS} (an inpainting checkpoint), got {in_channels}")
    table = SMALL_UNET_CONFIGS if small else UNET_CONFIGS
    if fam not in table:
        raise ValueError(f"no {'reduced-width ' if small else ''}architecture for family {fam!r}")
    return dict(table[fam], in_channels=in_channels)


class _DownBlock(nn.Module):
    def __init__(self, cin, cout, temb, layers, attn, heads, depth, cross, linear, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, temb) for i in range(layers)])
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, depth, cross, linear) for _ in range(layers)]) if attn else None
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if downsample else None

    def forward(self, x, temb, ctx, kv=None):
        outs = []
        for i, r in enumerate(self.resnets):
            x = r(x, temb)
            if self.attentions is not None:
                x = self.attentions[i](x, ctx, kv)
            outs.append(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
            outs.append(x)
        return x, outs


class _MidBlock(nn.Module):
    def __init__(self, ch, temb, heads, depth, cross, linear):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb), ResnetBlock2D(ch, ch, temb)])
        self.attentions = nn.ModuleList([Transformer2DModel(ch, heads, depth, cross, linear)])

    def forward(self, x, temb, ctx, kv=None):
        return self.resnets[1](self.attentions[0](self.resnets[0](x, temb), ctx, kv), temb)


class _UpBlock(nn.Module):
    def __init__(self, cin, cout, cprev, temb, layers, attn, heads, depth, cross, linear, upsample):
        super().__init__()
        rs = []
        for i in range(layers):
            skip = cin if i == layers - 1 else cout
            rs.append(ResnetBlock2D((cprev if i == 0 else cout) + skip, cout, temb))
        self.resnets = nn.ModuleList(rs)
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, depth, cross, linear) for _ in range(layers)]) if attn else None
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if upsample else None

    def forward(self, x, skips, temb, ctx, kv=None):
        for i, r in enumerate(self.resnets):
            x = r.forward_cat(x, skips.pop(), temb)
            if self.attentions is not None:
                x = self.attentions[i](x, ctx, kv)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class ImageProjection(nn.Module):
    """The base IP-Adapters' image projection (diffusers' ``ImageProjection``): CLIP image embedding [B, clip_dim] ->
    LayerNorm(Linear(e).reshape(B, Ni, cross_dim)), the Ni image tokens appended to the text tokens."""

    def __init__(self, clip_dim, cross_dim, tokens):
        super().__init__()
        self.tokens, self.cross_dim = tokens, cross_dim
        self.proj = nn.Linear(clip_dim, tokens * cross_dim)
        self.norm = nn.LayerNorm(cross_dim)

    def forward(self, embeds):
        return self.norm(self.proj(embeds).reshape(-1, self.tokens, self.cross_dim))


class PerceiverAttention(nn.Module):
    """One attention of the Resampler: the latents attend over [x | latents]; heads of 64, all projections bias-free."""
    DIM_HEAD = 64

    def __init__(self, dim, heads):
        super().__init__()
        inner = heads * self.DIM_HEAD
        self.heads = heads
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, 2 * inner, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)

    def forward(self, x, latents):
        x, latents = self.norm1(x), self.norm2(latents)
        B, N, _ = latents.shape
        q = self.to_q(latents)
        k, v = self.to_kv(torch.cat([x, latents], dim=-2)).chunk(2, dim=-1)
        q, k, v = (t.reshape(B, t.shape[1], self.heads, self.DIM_HEAD).transpose(1, 2) for t in (q, k, v))
        c = self.DIM_HEAD ** -0.25            # dh^-1/4 on q and on k, as published (the product is the usual dh^-1/2)
        w = torch.softmax((q * c) @ (k * c).transpose(-1, -2), dim=-1)
        return self.to_out((w @ v).transpose(1, 2).reshape(B, N, -1))


class Resampler(nn.Module):
    """The IP-Adapter Plus image projection (the published ``resampler.py``): the CLIP vision model's penultimate hidden states
    [B, S, embed_dim] -> Ni learned latents that attend over them through ``depth`` Perceiver layers -> [B, Ni, cross_dim] image
    tokens.  Attribute names are the file's keys (``image_proj.<name>``).  Runs once per image in torch: not on the hot path."""

    def __init__(self, dim, depth, heads, tokens, embed_dim, cross_dim, ff_inner):
        super().__init__()
        self.tokens, self.cross_dim = tokens, cross_dim
        self.latents = nn.Parameter(torch.zeros(1, tokens, dim))
        self.proj_in = nn.Linear(embed_dim, dim)
        self.proj_out = nn.Linear(dim, cross_dim)
        self.norm_out = nn.LayerNorm(cross_dim)
        self.layers = nn.ModuleList(
            nn.ModuleList([PerceiverAttention(dim, heads),
                           nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, ff_inner, bias=False), nn.GELU(),
                                         nn.Linear(ff_inner, dim, bias=False))])
            for _ in range(depth))

    def forward(self, x):
        latents = self.latents.repeat(x.shape[0], 1, 1)
        x = self.proj_in(x)
        for attn, ff in self.layers:
            latents = attn(x, latents) + latents
            latents = ff(latents) + latents
        return self.norm_out(self.proj_out(latents))

    @staticmethod
    def expected_keys(flat, cross):
        """{``image_proj.*`` key: shape} a Plus file must hold, every size read from the shapes of ``flat``; ValueError where the
        anchor tensors are missing or do not fit (naming Plus and Resampler) -> (expected, constructor arguments)"""
        def need(key, dims):
            t = flat.get(key)
            if t is None or t.dim() != dims:
                raise ValueError(f"IP-Adapter Plus: the Resampler's {key} is missing or not {dims}-dimensional; nothing installed")
            return t
        lat = need("image_proj.latents", 3)
        ni, dim = int(lat.shape[1]), int(lat.shape[2])
        if lat.shape[0] != 1 or not 1 <= ni <= ops.IP_MAX_IMAGE_KEYS:
            raise ValueError(f"IP-Adapter Plus: the Resampler's image_proj.latents is {tuple(lat.shape)}: not [1, 1..{ops.IP_MAX_IMAGE_KEYS}, "
                             "dim]; nothing installed")
        embed_dim = int(need("image_proj.proj_in.weight", 2).shape[1])
        out_w = need("image_proj.proj_out.weight", 2)
        if out_w.shape[0] != cross:
            raise ValueError(f"IP-Adapter Plus: the Resampler's proj_out has {out_w.shape[0]} output features, this UNet's cross-attention "
                             f"width is {cross}; nothing installed")
        layer_ids = sorted({int(k.split(".")[2]) for k in flat if k.startswith("image_proj.layers.") and k.split(".")[2].isdigit()})
        depth = len(layer_ids)
        if depth == 0 or layer_ids != list(range(depth)):
            raise ValueError(f"IP-Adapter Plus: the Resampler's layers are numbered {layer_ids[:8]}: not 0 .. depth - 1; nothing installed")
        inner = int(need("image_proj.layers.0.0.to_q.weight", 2).shape[0])
        ffi = int(need("image_proj.layers.0.1.1.weight", 2).shape[0])
        if inner % PerceiverAttention.DIM_HEAD or inner == 0:
            raise ValueError(f"IP-Adapter Plus: the Resampler's to_q has {inner} output features: not heads of {PerceiverAttention.DIM_HEAD}")
        exp = {"image_proj.latents": (1, ni, dim), "image_proj.proj_in.weight": (dim, embed_dim), "image_proj.proj_in.bias": (dim,),
               "image_proj.proj_out.weight": (cross, dim), "image_proj.proj_out.bias": (cross,),
               "image_proj.norm_out.weight": (cross,), "image_proj.norm_out.bias": (cross,)}
        for i in range(depth):
            p = f"image_proj.layers.{i}"
            for n in ("norm1", "norm2"):
                exp[f"{p}.0.{n}.weight"] = exp[f"{p}.0.{n}.bias"] = (dim,)
            exp[f"{p}.0.to_q.weight"], exp[f"{p}.0.to_kv.weight"], exp[f"{p}.0.to_out.weight"] = (inner, dim), (2 * inner, dim), (dim, inner)
            exp[f"{p}.1.0.weight"] = exp[f"{p}.1.0.bias"] = (dim,)
            exp[f"{p}.1.1.weight"], exp[f"{p}.1.3.weight"] = (ffi, dim), (dim, ffi)
        return exp, dict(dim=dim, depth=depth, heads=inner // PerceiverAttention.DIM_HEAD, tokens=ni, embed_dim=embed_dim,
                         cross_dim=cross, ff_inner=ffi)


IP_MAX_ADAPTERS = 4


def flatten_ip_adapter_state(state):
    """An IP-Adapter state dict with flat keys, from either form a file holds: already flat (``image_proj.proj.weight``,
    ``ip_adapter.1.to_k_ip.weight``: safetensors) or nested ``{"image_proj": {...}, "ip_adapter": {...}}`` (the pickled files)."""
    if not isinstance(state, dict):
        raise ValueError(f"IP-Adapter state must be a dict of tensors, got {type(state).__name__}")
    flat = {}
    for key, val in state.items():
        if isinstance(val, dict):
            for sub, t in val.items():
                flat[f"{key}.{sub}"] = t
        else:
            flat[key] = val
    bad = [k for k, t in flat.items() if not isinstance(t, torch.Tensor)]
    if bad:
        raise ValueError(f"IP-Adapter state holds non-tensor entries: {bad[:4]}")
    return flat


class UNet2DConditionModel(nn.Module):
    def __init__(self, sample_size, in_channels, block_out_channels, layers_per_block, attn, transformer_depth, heads,
                 cross_attention_dim, use_linear_projection, addition_time_embed_dim, pooled_projection_dim,
                 out_channels=4):
        super().__init__()
        boc = tuple(block_out_channels)
        temb = boc[0] * 4
        self.config = SimpleNamespace(sample_size=sample_size, in_channels=in_channels, out_channels=out_channels, block_out_channels=boc,
                                      cross_attention_dim=cross_attention_dim,
                                      addition_time_embed_dim=addition_time_embed_dim,
                                      pooled_projection_dim=pooled_projection_dim)
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        if addition_time_embed_dim:
            self.add_embedding = TimestepEmbedding(addition_time_embed_dim * 6 + pooled_projection_dim, temb)
        n = len(boc)
        self.down_blocks = nn.ModuleList()
        ch = boc[0]
        for i in range(n):
            self.down_blocks.append(_DownBlock(ch, boc[i], temb, layers_per_block, attn[i], heads[i], transformer_depth[i],
                                               cross_attention_dim, use_linear_projection, downsample=(i < n - 1)))
            ch = boc[i]
        self.mid_block = _MidBlock(boc[-1], temb, heads[-1], transformer_depth[-1], cross_attention_dim, use_linear_projection)
        self.up_blocks = nn.ModuleList()
        rev, rattn, rheads, rdepth = boc[::-1], attn[::-1], heads[::-1], transformer_depth[::-1]
        prev = rev[0]
        for i in range(n):
            cout, cin = rev[i], rev[min(i + 1, n - 1)]
            self.up_blocks.append(_UpBlock(cin, cout, prev, temb, layers_per_block + 1, rattn[i], rheads[i], rdepth[i],
                                           cross_attention_dim, use_linear_projection, upsample=(i < n - 1)))
            prev = cout
        self.conv_norm_out = nn.GroupNorm(32, boc[0], eps=1e-5)
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)
        self.ip_tokens = 0          # IP-Adapter image tokens at the end of the context; 0: no adapter installed
        self.ip_image_proj = None   # the (first) installed adapter's ImageProjection / Resampler
        self.ip_weights = None      # two or more adapters: fp32 [IP_MAX_ADAPTERS] on the device, one weight per adapter (section 32)
        self._ip_entries = []

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    def embed(self, sample, timestep, added_cond_kwargs):
        B = sample.shape[0]
        t = torch.as_tensor(timestep, device=sample.device).reshape(-1).expand(B)
        emb = self.time_embedding(timestep_embedding(t, self.config.block_out_channels[0]).to(sample.dtype))
        if self.config.addition_time_embed_dim:
            ids = added_cond_kwargs["time_ids"]
            tid = timestep_embedding(ids.reshape(-1).float(), self.config.addition_time_embed_dim).reshape(B, -1)
            add = torch.cat([added_cond_kwargs["text_embeds"].to(sample.dtype), tid.to(sample.dtype)], dim=-1)
            emb = emb + self.add_embedding(add)
        return emb

    def cross_attention_kv(self, encoder_hidden_states, into=None):
        """{id(attention module): k|v [B, Nk, 2 inner]} for every cross-attention of the model: functions of the text rows only,
        so the pipeline computes them once per image (per hipGraph batch shape) instead of once per forward -- 70 projections
        of the text tokens (77 per prompt chunk) per SDXL forward, ~100 forwards per image.  ``into``: a dict from an earlier call whose tensors are
        overwritten in place (a captured hipGraph reads them at fixed addresses)."""
        ctx = encoder_hidden_states.to(self.dtype)
        out = {} if into is None else into
        for m in self.modules():
            if isinstance(m, BasicTransformerBlock):
                out[id(m.attn2)] = m.attn2.project_kv(ctx, None if into is None else into[id(m.attn2)])
        return out

    # ---- IP-Adapter ---------------------------------------------------------------------------------
    def ip_attentions(self):
        """The cross attentions in the order an IP-Adapter file numbers them: ``down_blocks`` by index, then ``up_blocks``, then
        ``mid_block``; within each ``attentions[i].transformer_blocks[j].attn2``.  The n-th takes ``ip_adapter.{2n+1}.*`` --
        diffusers' ``attn_processors`` enumeration, whose even indices are the parameter-free self attentions."""
        out = []
        for blk in list(self.down_blocks) + list(self.up_blocks) + [self.mid_block]:
            for tr in (blk.attentions or ()):
                out.extend(tb.attn2 for tb in tr.transformer_blocks)
        return out

    @torch.no_grad()
    def install_ip_adapter(self, state, add=False):
        """Install an IP-Adapter from its state dict (flat ``image_proj.*`` / ``ip_adapter.*`` keys or the nested
        ``{"image_proj": {...}, "ip_adapter": {...}}`` form): a base adapter (``image_proj.proj`` / ``image_proj.norm``:
        ``ImageProjection``) or a Plus adapter (``image_proj.latents`` / ``layers`` / ``proj_in`` / ``proj_out`` / ``norm_out``:
        ``Resampler``).  Every expected key must be present with a fitting shape and no other key may be: otherwise ValueError, and
        nothing is installed.  ``add``: append behind the installed adapters (up to ``IP_MAX_ADAPTERS``) instead of replacing them.
        Returns the image-token count of this adapter."""
        flat = flatten_ip_adapter_state(state)
        if any(k.startswith("image_proj.proj.0.") or k.startswith("image_proj.proj.2.") or "lora" in k for k in flat):
            raise ValueError("this is an IP-Adapter FaceID file (image_proj.proj.0.* / LoRA keys): FaceID / ID-embedding adapters are not "
                             "supported; nothing installed")
        resampler_keys = [k for k in flat if k.startswith(("image_proj.latents", "image_proj.layers.", "image_proj.proj_in",
                                                            "image_proj.proj_out", "image_proj.norm_out"))]
        base_keys = [k for k in flat if k.startswith(("image_proj.proj.", "image_proj.norm."))]
        if resampler_keys and base_keys:
            raise ValueError(f"this file mixes an IP-Adapter 'Plus' Resampler's keys ({resampler_keys[0]}) with a base adapter's "
                             f"ImageProjection keys ({base_keys[0]}): it is neither; nothing installed")
        if add and len(self.__dict__.get("_ip_entries", ())) >= IP_MAX_ADAPTERS:
            raise ValueError(f"{IP_MAX_ADAPTERS} IP-Adapters are installed already: a fifth does not fit; nothing installed")
        attns = self.ip_attentions()
        cross = self.config.cross_attention_dim
        if resampler_keys:
            expected, rs_args = Resampler.expected_keys(flat, cross)
            ni = rs_args["tokens"]
        else:
            proj_w = flat.get("image_proj.proj.weight")
            if proj_w is None or proj_w.dim() != 2:
                raise ValueError("IP-Adapter: image_proj.proj.weight is missing or not a matrix")
            if proj_w.shape[0] % cross or not 1 <= proj_w.shape[0] // cross <= ops.IP_MAX_IMAGE_KEYS:
                raise ValueError(f"IP-Adapter: image_proj.proj has {proj_w.shape[0]} output features: not 1..{ops.IP_MAX_IMAGE_KEYS} "
                                 f"image tokens of cross-attention width {cross}")
            ni, clip_dim = proj_w.shape[0] // cross, proj_w.shape[1]
            expected = {"image_proj.proj.weight": (ni * cross, clip_dim), "image_proj.proj.bias": (ni * cross,),
                        "image_proj.norm.weight": (cross,), "image_proj.norm.bias": (cross,)}
        for n, a in enumerate(attns):
            for name in ("to_k_ip", "to_v_ip"):
                expected[f"ip_adapter.{2 * n + 1}.{name}.weight"] = (a.to_k.out_features, cross)
        missing = sorted(set(expected) - set(flat))
        surplus = sorted(set(flat) - set(expected))
        wrong = sorted(k for k in expected if k in flat and tuple(flat[k].shape) != expected[k])
        if missing or surplus or wrong:
            raise ValueError(f"IP-Adapter does not fit this UNet ({len(attns)} cross attentions, width {cross}): "
                             f"missing {missing[:4]}, unexpected {surplus[:4]}, "
                             f"wrong shape {[(k, tuple(flat[k].shape), expected[k]) for k in wrong[:4]]}; nothing installed")
        like = self.conv_in.weight

        def linear(w, b=None):
            m = nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device=like.device, dtype=like.dtype)
            m.weight.copy_(w)
            if b is not None:
                m.bias.copy_(b)
            return m.requires_grad_(False)
        if resampler_keys:    # (first to the model's dtype, then the copy: the file's values are rounded once)
            proj = Resampler(**rs_args).to(device=like.device, dtype=like.dtype).requires_grad_(False)
            proj.load_state_dict({k[len("image_proj."):]: flat[k] for k in expected if k.startswith("image_proj.")})
        else:
            proj = ImageProjection(clip_dim, cross, ni).to(device=like.device, dtype=like.dtype).requires_grad_(False)
            proj.proj.weight.copy_(flat["image_proj.proj.weight"]), proj.proj.bias.copy_(flat["image_proj.proj.bias"])
            proj.norm.weight.copy_(flat["image_proj.norm.weight"]), proj.norm.bias.copy_(flat["image_proj.norm.bias"])
        # (a replacement keeps the scale in force, as it always did; an appended adapter starts at 1)
        entry = {"proj": proj, "kind": "plus" if resampler_keys else "base", "tokens": ni, "scale": 1.0 if add else float(self.ip_scale),
                 "kv": [(linear(flat[f"ip_adapter.{2 * n + 1}.to_k_ip.weight"]), linear(flat[f"ip_adapter.{2 * n + 1}.to_v_ip.weight"]))
                        for n in range(len(attns))]}
        held = list(self.__dict__.get("_ip_entries", ())) if add else []
        self._install_ip_entries(held + [entry])
        return ni

    @staticmethod
    def _ip_proj_name(a):
        return "ip_image_proj" if a == 0 else f"ip_image_proj_{a}"

    def _install_ip_entries(self, entries):
        """Make ``entries`` (image projection, kind, token count, scale, per-layer (to_k_ip, to_v_ip)) the installed adapters, in
        order.  One adapter: the attribute names, state_dict() keys and by-value scale the project always had.  Two or more: the
        further adapters under ``ip_image_proj_{a}`` / ``to_k_ip_{a}`` / ``to_v_ip_{a}`` and ONE fp32 device tensor of weights, at
        an address that stays for the life of this UNet, shared by all its attention layers."""
        attns = self.ip_attentions()
        for a in range(len(self.__dict__.get("_ip_entries", ()))):
            if isinstance(getattr(self, self._ip_proj_name(a), None), nn.Module):
                delattr(self, self._ip_proj_name(a))
        for at in attns:
            at.set_ip_adapter()
        self.ip_image_proj = None
        self._ip_entries = list(entries)
        self.ip_tokens = sum(e["tokens"] for e in entries)
        if not entries:
            return
        if len(entries) >= 2 and self.__dict__.get("ip_weights") is None:
            self.ip_weights = torch.zeros(IP_MAX_ADAPTERS, dtype=torch.float32, device=self.conv_in.weight.device)
        for a, e in enumerate(entries):
            setattr(self, self._ip_proj_name(a), e["proj"])
            for at, (to_k, to_v) in zip(attns, e["kv"]):
                if a == 0:
                    at.set_ip_adapter(to_k, to_v, e["tokens"])
                else:
                    at.add_ip_adapter(to_k, to_v, e["tokens"], self.ip_weights[:len(entries)])
        self.ip_scales = [e["scale"] for e in entries]
        if len(entries) == 1 and self.__dict__.get("ip_weights") is not None:
            self.ip_weights[:1].fill_(entries[0]["scale"])     # read by the masked path alone (ip_mask_weights)

    def ip_mask_weights(self):
        """The fp32 device weights [A] the masked cross attentions read (section 33): the tensor of section 32, allocated here for a
        single adapter as well -- the masked path reads its scale from the device at every adapter count.  Call it once outside a
        graph capture; afterwards ``ip_scale`` / ``ip_scales`` keep it current."""
        entries = self.__dict__.get("_ip_entries", ())
        if not entries:
            raise ValueError("no IP-Adapter is installed")
        if self.__dict__.get("ip_weights") is None:
            self.ip_weights = torch.zeros(IP_MAX_ADAPTERS, dtype=torch.float32, device=self.conv_in.weight.device)
            self.ip_weights[:1].fill_(entries[0]["scale"])
        return self.ip_weights[:len(entries)]

    def remove_ip_adapter(self, index=None):
        """remove every adapter, or the ``index``-th one (the others keep their order and scales)"""
        entries = list(self.__dict__.get("_ip_entries", ()))
        if index is not None:
            del entries[index]
        else:
            entries = []
        self._install_ip_entries(entries)

    @property
    def ip_adapters(self):
        """[(kind "base" | "plus", image tokens, scale)] of the installed adapters, in context order"""
        return [(e["kind"], e["tokens"], e["scale"]) for e in self.__dict__.get("_ip_entries", ())]

    @property
    def ip_segments(self):
        return tuple(e["tokens"] for e in self.__dict__.get("_ip_entries", ()))

    @property
    def ip_scale(self):
        entries = self.__dict__.get("_ip_entries", ())
        if len(entries) >= 2:
            return entries[0]["scale"]
        a = self.ip_attentions()
        return a[0].ip_scale if a else 1.0

    @ip_scale.setter
    def ip_scale(self, scale):
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"IP-Adapter scale must be finite, got {scale}")
        entries = self.__dict__.get("_ip_entries", ())
        if len(entries) >= 2:
            self.ip_scales = [scale] * len(entries)
            return
        for e in entries:
            e["scale"] = scale
        for a in self.ip_attentions():
            a.ip_scale = scale
        if entries and self.__dict__.get("ip_weights") is not None:
            with torch.no_grad():
                self.ip_weights[:1].fill_(scale)

    @property
    def ip_scales(self):
        return [e["scale"] for e in self.__dict__.get("_ip_entries", ())]

    @ip_scales.setter
    def ip_scales(self, scales):
        """one scale per installed adapter.  One adapter: the by-value kernel argument.  Several: a copy into the device weights the
        kernels read when they run -- no captured graph has to be dropped."""
        entries = self.__dict__.get("_ip_entries", ())
        scales = [float(s) for s in scales]
        if len(scales) != len(entries):
            raise ValueError(f"{len(entries)} IP-Adapter(s) installed, {len(scales)} scale(s) given")
        if not all(math.isfinite(s) for s in scales):
            raise ValueError(f"IP-Adapter scales must be finite, got {scales}")
        if len(entries) == 1:
            self.ip_scale = scales[0]
            return
        for e, s in zip(entries, scales):
            e["scale"] = s
        if entries:
            with torch.no_grad():
                self.ip_weights[:len(entries)].copy_(torch.tensor(scales, dtype=torch.float32))

    @torch.no_grad()
    def ip_image_tokens(self, embeds, index=0):
        """adapter ``index``: [B, clip_dim] CLIP image embeddings (base) or [B, S, embed_dim] penultimate hidden states (Plus) ->
        [B, Ni, cross_dim] image tokens (for a base adapter a zero embedding gives the unconditional ones)"""
        entries = self.__dict__.get("_ip_entries", ())
        if not entries:
            raise ValueError("no IP-Adapter is installed")
        proj = entries[index]["proj"]
        p = proj.norm.weight if entries[index]["kind"] == "base" else proj.norm_out.weight
        return proj(embeds.to(device=p.device, dtype=p.dtype))

    def ip_embed_shape(self, index=0):
        """(rank, last dimension) of the embeddings adapter ``index`` takes: (2, clip_dim) base, (3, embed_dim) Plus"""
        e = self.__dict__["_ip_entries"][index]
        return (2, e["proj"].proj.in_features) if e["kind"] == "base" else (3, e["proj"].proj_in.in_features)

    def forward(self, sample, timestep, encoder_hidden_states=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None, cross_kv=None, control_residuals=None, ip_masks=None, **_):
        """``control_residuals`` = (per-net lists of raw down residuals, per-net raw mid residuals, w f32 [B, N]): the hand-off of
        several ControlNets -- every skip and the mid-block output receive sum_n w[:, n] * r_n in ONE
        ``ops.control_residuals`` launch, in place.  Mutually exclusive with the two ``*_additional_residual(s)`` keywords.
        ``ip_masks`` = (m f32 [B, A, S], PH, PW): IP-Adapter attention masks -- per row and adapter the four
        levels of ``ops.ip_mask_rows``; every cross attention multiplies adapter a's term at query row i by its level's m[b, a, i]."""
        if ip_masks is not None:
            m, PH, PW = ip_masks
            A = len(self.ip_segments)
            S = ops.ip_mask_layout(PH, PW)[1]
            if not A:
                raise ValueError("ip_masks without an installed IP-Adapter")
            if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or tuple(m.shape) != (sample.shape[0], A, S):
                raise ValueError(f"ip_masks: m must be f32 [{sample.shape[0]}, {A}, {S}] for {PH} x {PW} rows, got "
                                 f"{tuple(getattr(m, 'shape', ()))} {getattr(m, 'dtype', None)}")
            w = self.ip_mask_weights()
            attns = self.ip_attentions()
            for at in attns:
                at.ip_mask = (m, int(PH), int(PW), w)
            try:
                return self.forward(sample, timestep, encoder_hidden_states, added_cond_kwargs, down_block_additional_residuals,
                                    mid_block_additional_residual, cross_kv, control_residuals)
            finally:
                for at in attns:
                    at.ip_mask = None
        if control_residuals is not None and (down_block_additional_residuals is not None or mid_block_additional_residual is not None):
            raise ValueError("control_residuals and down_block_additional_residuals / mid_block_additional_residual exclude each other")
        x = sample.to(self.dtype)
        if CHANNELS_LAST and x.is_cuda and x.dtype != torch.float32:
            x = x.contiguous(memory_format=torch.channels_last)
        ctx = encoder_hidden_states.to(self.dtype)
        if self.ip_tokens and ctx.shape[1] <= self.ip_tokens:
            raise ValueError(f"an IP-Adapter with {self.ip_tokens} image tokens is installed: the context must be [text tokens | image "
                             f"tokens], got {ctx.shape[1]} tokens in all")
        emb = self.embed(x, timestep, added_cond_kwargs)
        x = self.conv_in(x)
        if getattr(self, "residual_fp32", False) and x.dtype != torch.float32:
            x = x.float()      # from here to conv_norm_out the residual stream is fp32 (see _stream32)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, emb, ctx, cross_kv)
            skips.extend(outs)
        if down_block_additional_residuals is not None:
            skips = [s + r for s, r in zip(skips, down_block_additional_residuals)]
        x = self.mid_block(x, emb, ctx, cross_kv)
        if mid_block_additional_residual is not None:
            x = x + mid_block_additional_residual
        if control_residuals is not None:
            # every down block and the mid block have read their inputs: the skips and x are written in place (a skip that IS the
            # mid block's output cannot occur, the mid block ends in a ResnetBlock2D that allocates its result)
            downs, mids, w = control_residuals
            if any(len(d) != len(skips) for d in downs) or len(mids) != len(downs):
                raise ValueError(f"control_residuals: {len(skips)} skips, got residual lists of {[len(d) for d in downs]} and {len(mids)} mids")
            summed = ops.control_residuals(skips + [x], [list(d) + [m] for d, m in zip(downs, mids)], w)
            skips, x = summed[:-1], summed[-1]
        for blk in self.up_blocks:
            x = blk(x, skips, emb, ctx, cross_kv)
        x = self.conv_out(group_norm_act(self.conv_norm_out, x, silu=True))
        return ModelOutput(sample=x)


# ---------------------------------------------------------------------------------------------------
# ControlNet (diffusers ControlNetModel): the UNet encoder + zero-convs, conditioned on a pixel-space image
# ---------------------------------------------------------------------------------------------------
class _CondEmbedding(nn.Module):
    def __init__(self, out_ch, chans=(16, 32, 96, 256)):
        super().__init__()
        self.conv_in = nn.Conv2d(3, chans[0], 3, padding=1)
        blocks = []
        for a, b in zip(chans[:-1], chans[1:]):
            blocks += [nn.Conv2d(a, a, 3, padding=1), nn.Conv2d(a, b, 3, padding=1, stride=2)]
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(chans[-1], out_ch, 3, padding=1)

    def forward(self, c):
        h = F.silu(self.conv_in(c))
        for b in self.blocks:
            h = F.silu(b(h))
        return self.conv_out(h)


class ControlNetModel(nn.Module):
    def __init__(self, unet_cfg):
        super().__init__()
        c = dict(unet_cfg)
        boc = tuple(c["block_out_channels"])
        temb = boc[0] * 4
        self.config = SimpleNamespace(**{k: c[k] for k in ("sample_size", "in_channels", "cross_attention_dim",
                                                           "addition_time_embed_dim", "pooled_projection_dim")},
                                      block_out_channels=boc)
        self.conv_in = nn.Conv2d(c["in_channels"], boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        if c["addition_time_embed_dim"]:
            self.add_embedding = TimestepEmbedding(c["addition_time_embed_dim"] * 6 + c["pooled_projection_dim"], temb)
        self.controlnet_cond_embedding = _CondEmbedding(boc[0])
        n = len(boc)
        self.down_blocks = nn.ModuleList()
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(boc[0], boc[0], 1)])
        ch = boc[0]
        for i in range(n):
            self.down_blocks.append(_DownBlock(ch, boc[i], temb, c["layers_per_block"], c["attn"][i], c["heads"][i],
                                               c["transformer_depth"][i], c["cross_attention_dim"],
                                               c["use_linear_projection"], downsample=(i < n - 1)))
            ch = boc[i]
            for _ in range(c["layers_per_block"] + (1 if i < n - 1 else 0)):
                self.controlnet_down_blocks.append(nn.Conv2d(ch, ch, 1))
        self.mid_block = _MidBlock(boc[-1], temb, c["heads"][-1], c["transformer_depth"][-1], c["cross_attention_dim"],
                                   c["use_linear_projection"])
        self.controlnet_mid_block = nn.Conv2d(boc[-1], boc[-1], 1)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    embed = UNet2DConditionModel.embed
    cross_attention_kv = UNet2DConditionModel.cross_attention_kv

    def forward(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                guess_mode=False, return_dict=False, added_cond_kwargs=None, cross_kv=None, raw_residuals=False, **_):
        """``raw_residuals``: return the zero-convolution outputs as they are, without the ``* conditioning_scale`` launches (the
        weights of ``UNet2DConditionModel.forward(control_residuals=)`` take the scale's place)"""
        x = sample.to(self.dtype)
        cond = controlnet_cond.to(self.dtype)
        if CHANNELS_LAST and x.is_cuda and x.dtype != torch.float32:
            x = x.contiguous(memory_format=torch.channels_last)
            cond = cond.contiguous(memory_format=torch.channels_last)
        ctx = encoder_hidden_states.to(self.dtype)
        emb = self.embed(x, timestep, added_cond_kwargs)
        x = self.conv_in(x) + self.controlnet_cond_embedding(cond)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, emb, ctx, cross_kv)
            skips.extend(outs)
        x = self.mid_block(x, emb, ctx, cross_kv)
        if raw_residuals:
            return [conv(s) for conv, s in zip(self.controlnet_down_blocks, skips)], self.controlnet_mid_block(x)
        down = [conv(s) * conditioning_scale for conv, s in zip(self.controlnet_down_blocks, skips)]
        mid = self.controlnet_mid_block(x) * conditioning_scale
        return down, mid


# ---------------------------------------------------------------------------------------------------
# AutoencoderKL
# ---------------------------------------------------------------------------------------------------
class _VaeAttention(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.group_norm = nn.GroupNorm(32, ch, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(ch, ch), nn.Linear(ch, ch), nn.Linear(ch, ch)
        self.to_out = nn.ModuleList([nn.Linear(ch, ch), nn.Dropout(0.0)])

    def forward(self, x):
        B, C, H, W = x.shape
        h = group_norm_act(self.group_norm, x)
        key_bias = _plane_weights(x)[2]   # the narrowed constant-image encode: log multiplicity of every key (None otherwise)
        cl = ops.is_nhwc(h)   # channels-last VAE (VAE_SPLIT_CONV)
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C) if cl else h.view(B, C, H * W).transpose(1, 2)
        if VAE_HIP_ATTENTION and h.is_cuda and h.dtype == torch.float32 and (H * W) % 4 == 0:
            # two fp32 library GEMMs around ed_softmax_rows: no AOTriton (Triton) kernel on the path
            o = ops.vae_attention(self.to_q(h), self.to_k(h), self.to_v(h), None if key_bias is None else key_bias.float())
        elif key_bias is not None:
            # scores + log multiplicity, formed in fp32 for a 16-bit VAE (log 769 in fp16 would be 3e-3 off); a few thousand tokens
            dt = torch.float32 if h.dtype in _HALF else h.dtype
            q, k, v = (f(h).to(dt) for f in (self.to_q, self.to_k, self.to_v))
            scores = torch.baddbmm(key_bias.to(dt).view(1, 1, -1), q, k.transpose(1, 2), alpha=C ** -0.5)
            o = torch.bmm(scores.softmax(-1), v).to(h.dtype)
        else:
            q, k, v = (f(h).unsqueeze(1) for f in (self.to_q, self.to_k, self.to_v))
            o = F.scaled_dot_product_attention(q, k, v).squeeze(1)
        a = self.to_out[0](o)
        a = a.view(B, H, W, C).permute(0, 3, 1, 2) if cl else a.transpose(1, 2).reshape(B, C, H, W)   # (cl: a view, no copy)
        return x + a if VAE_NCHW_RESIDUAL else a + x


class _VaeMid(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, None, eps=1e-6), ResnetBlock2D(ch, ch, None, eps=1e-6)])
        self.attentions = nn.ModuleList([_VaeAttention(ch)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](_to_nchw(self.resnets[0](x))))


class _EncBlock(nn.Module):
    def __init__(self, cin, cout, layers, down):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, None, eps=1e-6) for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout, padding=0)]) if down else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.downsamplers[0](x) if self.downsamplers is not None else x


class _DecBlock(nn.Module):
    def __init__(self, cin, cout, layers, up):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, None, eps=1e-6) for i in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample2D(cout, vae=True)]) if up else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if self.upsamplers is not None else x


class _Encoder(nn.Module):
    def __init__(self, boc, latent_channels, layers=2):
        super().__init__()
        self.conv_in = nn.Conv2d(3, boc[0], 3, padding=1)
        self.down_blocks = nn.ModuleList()
        ch = boc[0]
        for i, c in enumerate(boc):
            self.down_blocks.append(_EncBlock(ch, c, layers, down=(i < len(boc) - 1)))
            ch = c
        self.mid_block = _VaeMid(ch)
        self.conv_norm_out = nn.GroupNorm(32, ch, eps=1e-6)
        self.conv_out = nn.Conv2d(ch, 2 * latent_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        return self.conv_out(group_norm_act(self.conv_norm_out, _to_nchw(self.mid_block(x)), silu=True))


class _Decoder(nn.Module):
    def __init__(self, boc, latent_channels, layers=2):
        super().__init__()
        rev = boc[::-1]
        self.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
        self.mid_block = _VaeMid(rev[0])
        self.up_blocks = nn.ModuleList()
        ch = rev[0]
        for i, c in enumerate(rev):
            self.up_blocks.append(_DecBlock(ch, c, layers + 1, up=(i < len(boc) - 1)))
            ch = c
        self.conv_norm_out = nn.GroupNorm(32, ch, eps=1e-6)
        self.conv_out = nn.Conv2d(ch, 3, 3, padding=1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(group_norm_act(self.conv_norm_out, _to_nchw(x), silu=True))


class DiagonalGaussian:
    def __init__(self, moments):
        self.mean, logvar = moments.chunk(2, dim=1)
        self.logvar = logvar.clamp(-30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise


class AutoencoderKL(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), latent_channels=4, scaling_factor=0.18215,
                 force_upcast=False):
        super().__init__()
        self.config = SimpleNamespace(block_out_channels=tuple(block_out_channels), scaling_factor=scaling_factor,
                                      force_upcast=force_upcast, latent_channels=latent_channels)
        self.encoder = _Encoder(tuple(block_out_channels), latent_channels)
        self.decoder = _Decoder(tuple(block_out_channels), latent_channels)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)

    @property
    def dtype(self):
        return self.quant_conv.weight.dtype

    @property
    def device(self):
        return self.quant_conv.weight.device

    def encode(self, x):
        return SimpleNamespace(latent_dist=DiagonalGaussian(self.quant_conv(self.encoder(x))))

    def constant_plan(self, Hpx, Wpx):
        """(rows, columns): geometry.plan_constant_axis of a constant ``Hpx`` x ``Wpx`` image for this encoder, None for an axis that
        is left alone (too short, not a whole number of latent units, or VAE_NARROW_CONSTANT off)"""
        levels = len(self.config.block_out_channels)
        S = 1 << (levels - 1)
        layers = len(self.encoder.down_blocks[0].resnets)
        if not VAE_NARROW_CONSTANT or Hpx % S or Wpx % S:
            return None, None
        return plan_constant_axis(Hpx // S, levels, layers), plan_constant_axis(Wpx // S, levels, layers)

    def _constant_tables(self, py, px, Hn, Wn, device):
        """({(H, W) of the narrowed level-l activation: (wx, wy, key_bias)}, expand index of the latent rows, of the latent columns) on
        ``device``, built once per plan.  fp32 (what the kernels read; the multiplicities are small integers), fp64 for an fp64 VAE;
        key_bias[y * W + x] = log wy[y] + log wx[x], the log multiplicity of a token."""
        key = (None if py is None else py.L, None if px is None else px.L, Hn, Wn, str(device), self.dtype)
        cache = self.__dict__.setdefault("_constant_cache", {})
        if key not in cache:
            dt = torch.float64 if self.dtype == torch.float64 else torch.float32
            planes = {}
            for lv in range(len(self.config.block_out_channels)):
                wy = torch.ones(Hn >> lv, dtype=dt) if py is None else torch.tensor(py.weights[lv], dtype=dt)
                wx = torch.ones(Wn >> lv, dtype=dt) if px is None else torch.tensor(px.weights[lv], dtype=dt)
                bias = (wy.double().log()[:, None] + wx.double().log()[None, :]).reshape(-1).to(dt)
                planes[(Hn >> lv, Wn >> lv)] = (None if px is None else wx.to(device), None if py is None else wy.to(device), bias.to(device))
            index = [None if p is None else torch.tensor(p.expand, dtype=torch.int64, device=device) for p in (py, px)]
            cache[key] = (planes, index)
        return cache[key]

    @torch.no_grad()
    def encode_constant(self, colour, Hpx, Wpx):
        """``encode`` of the constant-colour images ``colour`` [n, 3] expanded to [n, 3, Hpx, Wpx], without encoding what is constant
        (DESIGN.md section 27): the encoder's activations vary only in a border that zero padding makes (geometry.constant_border_trace),
        so it runs on an image with every long axis narrowed to that border plus a clean margin, in which ONE row / column per level
        stands for the removed run: GroupNorm's statistics and the attention's softmax count it with its multiplicity, everything else is
        local.  The moments are then expanded by repeating the representative latent row / column.  Exact in exact arithmetic; in fp32
        the sums are re-associated.  An image too small to narrow is ``encode`` of the expanded image, bit for bit."""
        n = colour.shape[0]
        py, px = self.constant_plan(Hpx, Wpx)
        if py is None and px is None:
            return self.encode(colour[:, :, None, None].expand(n, 3, Hpx, Wpx).contiguous())
        S = 1 << (len(self.config.block_out_channels) - 1)
        Hn, Wn = (Hpx if py is None else py.keep * S), (Wpx if px is None else px.keep * S)
        planes, (iy, ix) = self._constant_tables(py, px, Hn, Wn, colour.device)
        if _narrowed_encode_active():
            raise RuntimeError("encode_constant: a narrowed encode is already running on this thread")
        _CONSTANT_ENCODE.planes = planes
        try:
            moments = self.quant_conv(self.encoder(colour[:, :, None, None].expand(n, 3, Hn, Wn).contiguous()))
        finally:
            _CONSTANT_ENCODE.planes = None
        if iy is not None:
            moments = moments.index_select(2, iy)
        if ix is not None:
            moments = moments.index_select(3, ix)
        return SimpleNamespace(latent_dist=DiagonalGaussian(moments))

    def decode(self, z):
        return SimpleNamespace(sample=self.decoder(self.post_quant_conv(z)))


# ---------------------------------------------------------------------------------------------------
def is_inpaint_version(sd_version):
    """``"1.5-inpaint"`` / ``"2.0-inpaint"`` / ``"XL1.0-inpaint"``: the 9-channel variant of that ``sd_version``"""
    return sd_version.endswith(INPAINT_SUFFIX)


def family(sd_version):
    if is_inpaint_version(sd_version):
        sd_version = sd_version[:-len(INPAINT_SUFFIX)]
    if sd_version.startswith("XL"):
        return "sdxl"
    if sd_version in ("2.0", "2.1"):
        return "sd2"
    if sd_version in ("1.4", "1.5"):
        return "sd15"
    raise ValueError(f"no built-in architecture for sd_version={sd_version!r}; pass unet=/vae= explicitly")


def _seeded_init(module, seed):
    """Deterministic synthetic weights (no checkpoints exist offline): PyTorch's default ``reset_parameters`` init under
    a private seed (measured: the random-init SDXL loop stays finite over 50 steps in bf16 without any rescaling).
    ``torch.random.fork_rng`` restores the CPU generator and the generator of the device being initialised."""
    devs = sorted({p.device.index for p in module.parameters() if p.is_cuda and p.device.index is not None})
    with torch.random.fork_rng(devices=devs):
        torch.manual_seed(seed)
        for m in module.modules():
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()


def state_dict_in_channels(state_dict):
    """Input channels of the UNet a state dict belongs to, read off the SHAPE of ``conv_in.weight`` [C_out, C_in, 3, 3] (not off any
    ``config.json``); None when the tensor is absent."""
    w = state_dict.get("conv_in.weight")
    return None if w is None else int(w.shape[1])


def snapshot_in_channels(path):
    """``state_dict_in_channels`` of a ``diffusion_pytorch_model.safetensors`` without loading its tensors"""
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        return int(f.get_slice("conv_in.weight").get_shape()[1]) if "conv_in.weight" in f.keys() else None


def load_weights(module, path):
    """Load an HF-layout ``diffusion_pytorch_model.safetensors`` (same parameter names as diffusers)."""
    from safetensors.torch import load_file
    sd = load_file(path)
    missing, unexpected = module.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"{path}: {len(missing)} missing / {len(unexpected)} unexpected keys, e.g. {missing[:3]} {unexpected[:3]}")
    return module


# The 16-bit dtype of the UNet / ControlNet when the caller does not choose one.  fp16 is what the reference's own GPU path
# runs the UNet in (``torch.autocast('cuda')``, ED:1012), and measured on the MI355X (profiles/r3_precision.json) its loop
# drift against the fp32 reference path is 8x smaller than bf16's (5e-3 vs 4e-2 rel-L2 on the SDXL geometry: 10 vs 7
# mantissa bits at the same MFMA rate); it stays finite over 50 steps at full width with random-init weights.
DEFAULT_MODEL_DTYPE = torch.float16


def build_models(sd_version, device="cuda", dtype=None, weights=None, vae_dtype=torch.float32, controlnet=False, seed=0,
                 small=False):
    """(unet, vae[, controlnet]) for the reference's ``sd_version`` keys (ED:128-141).  UNet/ControlNet run in
    DEFAULT_MODEL_DTYPE (fp16) unless ``dtype`` says otherwise; the VAE stays fp32 like the reference (its decode runs
    outside autocast, ED:1080-1121, and the encoder is explicitly kept out of autocast, ED:328).  ``small=True`` builds the
    reduced-width variants (parity checks).  ``"1.5-inpaint"`` / ``"2.0-inpaint"`` / ``"XL1.0-inpaint"``, or a ``weights`` snapshot
    whose ``conv_in.weight`` has 9 input channels, build the 9-channel inpainting UNet of the family."""
    fam = family(sd_version)
    in_channels = INPAINT_IN_CHANNELS if is_inpaint_version(sd_version) else 4
    unet_file = os.path.join(weights, "unet", "diffusion_pytorch_model.safetensors") if weights else None
    if unet_file and os.path.isfile(unet_file):
        # an inpainting snapshot selects the 9-channel variant by itself: the width of its conv_in decides, whatever the name says
        in_channels = snapshot_in_channels(unet_file) or in_channels
    cfg = unet_config(fam, small, in_channels)
    # the ControlNet keeps the 4-channel configuration (a 9-channel UNet with a ControlNet is refused by the pipeline)
    cn_cfg = unet_config(fam, small, 4)
    dtype = dtype or DEFAULT_MODEL_DTYPE
    with torch.device("meta"):
        unet = UNet2DConditionModel(**cfg)
        vae_kw = dict(block_out_channels=SMALL_VAE_CHANNELS) if small else {}
        vae = AutoencoderKL(scaling_factor=0.13025 if fam == "sdxl" else 0.18215, force_upcast=(fam == "sdxl"), **vae_kw)
        cn = ControlNetModel(cn_cfg) if controlnet else None
    out = []
    for k, (m, dt, sub) in enumerate([(unet, dtype, "unet"), (vae, vae_dtype, "vae"), (cn, dtype, "controlnet")]):
        if m is None:
            continue
        m = m.to_empty(device=device)
        f = os.path.join(weights, sub, "diffusion_pytorch_model.safetensors") if weights else None
        if f and os.path.isfile(f):
            load_weights(m, f)
        else:
            _seeded_init(m, seed + k)
        m = m.to(dtype=dt).eval().requires_grad_(False)
        if CHANNELS_LAST and sub != "vae" and dt != torch.float32:  # 16-bit UNet / ControlNet; the fp32 VAE stays NCHW
            m = m.to(memory_format=torch.channels_last)
        out.append(m)
    return tuple(out)


def build_controlnet(sd_version, device="cuda", dtype=None, weights=None, index=0, seed=0, small=False):
    """ControlNet number ``index`` of a Multi-ControlNet, built as ``build_models`` builds the first: from the
    snapshot's subfolder ``controlnet`` (index 0), ``controlnet_1``, ``controlnet_2``, ... (diffusers' ``MultiControlNetModel`` layout)
    where it exists, seeded otherwise."""
    cn_cfg = unet_config(family(sd_version), small, 4)
    dtype = dtype or DEFAULT_MODEL_DTYPE
    with torch.device("meta"):
        cn = ControlNetModel(cn_cfg)
    cn = cn.to_empty(device=device)
    sub = "controlnet" if index == 0 else f"controlnet_{index}"
    f = os.path.join(weights, sub, "diffusion_pytorch_model.safetensors") if weights else None
    if f and os.path.isfile(f):
        load_weights(cn, f)
    else:
        _seeded_init(cn, seed + 2 + index)
    cn = cn.to(dtype=dtype).eval().requires_grad_(False)
    if CHANNELS_LAST and dtype != torch.float32:
        cn = cn.to(memory_format=torch.channels_last)
    return cn
