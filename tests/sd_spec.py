"""Test-side restatement of the Stable Diffusion model forwards (test infrastructure, never shipped).

A functional statement of what diffusers 0.21.4's ``UNet2DConditionModel``, ``ControlNetModel`` and ``AutoencoderKL`` compute for
the SD 1.x / SD 2.x / SDXL configurations, from diffusers' published definitions ("The model forward against an independent
statement").  Every function takes a state dict ``{HF parameter name: tensor}``, a name prefix and plain config scalars, calls only
``torch`` / ``torch.nn.functional``, builds no ``nn.Module`` and imports nothing from ``elasticdiffusion_official_amd``: it shares no
code with ``models.py``.  It is dtype- and device-agnostic: fp64 on the CPU is the reference, the same code in a 16-bit dtype (or fp32)
on the GPU is the yardstick of what the plain op sequence loses in that dtype.

Every semantic choice is a named entry of ``SEMANTICS`` so that a test can override one at a time (``override``) and check that its
inputs would notice.

PARITY NOTE: diffusers itself is neither installed nor installable here, so parity with it stays "unpinned"; this file and ``models.py``
share an author but no code.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

SEMANTICS = {
    "eps_unet": 1e-5,                 # GroupNorm of the UNet / ControlNet ResnetBlocks and of conv_norm_out
    "eps_transformer": 1e-6,          # GroupNorm in front of a Transformer2DModel
    "eps_vae": 1e-6,                  # every GroupNorm of the AutoencoderKL
    "eps_layernorm": 1e-5,            # LayerNorms of a BasicTransformerBlock
    "gelu": "none",                   # GEGLU's gelu: "none" = exact (erf); "tanh" = the approximation
    "flip_sin_to_cos": True,          # sinusoid = [cos | sin]
    "freq_shift": 0.0,
    "geglu_hidden_first": True,       # hidden, gate = proj(x).chunk(2, -1)
    "cat_x_first": True,              # up blocks: cat([x, skip], 1)
    "cat_text_first": True,           # SDXL: cat([text_embeds, time_embeds], -1)
    "asymmetric_pad": True,           # VAE downsampler: F.pad(x, (0, 1, 0, 1)), then stride 2 without padding
    "attention_scale_exponent": -0.5,  # scale = head_dim ** -0.5
    "vae_attention_bias": True,       # the VAE attention's to_q / to_k / to_v carry a bias
}
GROUPS = 32
MAX_PERIOD = 10000.0


@contextlib.contextmanager
def override(**entries):
    """``SEMANTICS`` with the given entries replaced, restored on exit"""
    unknown = set(entries) - set(SEMANTICS)
    if unknown:
        raise KeyError(f"no such SEMANTICS entry: {sorted(unknown)}")
    keep = dict(SEMANTICS)
    SEMANTICS.update(entries)
    try:
        yield
    finally:
        SEMANTICS.clear()
        SEMANTICS.update(keep)


# ---- parameters -----------------------------------------------------------------------------------------------------------------
def _is_norm(key):
    parts = key.split(".")
    return len(parts) >= 2 and "norm" in parts[-2]


def randomise(state_dict, seed):
    """A copy of ``state_dict`` in which no affine parameter sits at its trivial value: norm weights 1 + 0.2 randn, norm biases
    0.1 randn, every conv / linear bias 0.2 randn; weights left as they are.  Drawn in fp64 on the CPU in sorted key order, so the
    values do not depend on the dict's dtype, device or order."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key in sorted(state_dict):
        t = state_dict[key]
        r = None
        if _is_norm(key) and key.endswith(".weight"):
            r = 1.0 + 0.2 * torch.randn(t.shape, generator=g, dtype=torch.float64)
        elif key.endswith(".bias"):
            r = (0.1 if _is_norm(key) else 0.2) * torch.randn(t.shape, generator=g, dtype=torch.float64)
        out[key] = t.detach().clone() if r is None else r.to(device=t.device, dtype=t.dtype)
    return out


# ---- primitives -----------------------------------------------------------------------------------------------------------------
def _p(prefix, name):
    return f"{prefix}.{name}" if prefix else name


def _gn(sd, p, x, eps):
    return F.group_norm(x, GROUPS, sd[p + ".weight"], sd[p + ".bias"], eps)


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], SEMANTICS["eps_layernorm"])


def _conv(sd, p, x, stride=1, padding=1):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=stride, padding=padding)


def _lin(sd, p, x, bias=True):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"] if bias else None)


def _tokens(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _image(t, H, W):
    B, _, C = t.shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ---- embeddings -----------------------------------------------------------------------------------------------------------------
def sinusoid(t, dim):
    """[cos(t f) | sin(t f)], f_j = exp(-ln(10000) j / (half - freq_shift)), computed in fp32 as diffusers does (the caller casts)"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float32, device=t.device)
    freq = torch.exp(-math.log(MAX_PERIOD) * j / (half - SEMANTICS["freq_shift"]))
    arg = t.reshape(-1, 1).to(torch.float32) * freq[None, :]
    parts = [torch.cos(arg), torch.sin(arg)] if SEMANTICS["flip_sin_to_cos"] else [torch.sin(arg), torch.cos(arg)]
    return torch.cat(parts, dim=-1)


def _mlp(sd, p, x):
    return _lin(sd, p + ".linear_2", F.silu(_lin(sd, p + ".linear_1", x)))


def time_embedding(sd, prefix, cfg, t, batch, dtype, added=None):
    """emb [B, 4 boc[0]] of a scalar or per-row timestep ``t`` (+ SDXL's added condition ``added`` = dict(text_embeds, time_ids))"""
    dev = sd[_p(prefix, "time_embedding.linear_1.weight")].device
    t = torch.as_tensor(t, device=dev).reshape(-1).expand(batch)
    emb = _mlp(sd, _p(prefix, "time_embedding"), sinusoid(t, cfg["block_out_channels"][0]).to(dtype))
    if cfg["addition_time_embed_dim"]:
        ids = sinusoid(added["time_ids"].reshape(-1), cfg["addition_time_embed_dim"]).reshape(batch, -1).to(dtype)
        text = added["text_embeds"].to(dtype)
        add = torch.cat([text, ids] if SEMANTICS["cat_text_first"] else [ids, text], dim=-1)
        emb = emb + _mlp(sd, _p(prefix, "add_embedding"), add)
    return emb


# ---- blocks ---------------------------------------------------------------------------------------------------------------------
def resnet(sd, p, x, emb=None, eps=None):
    """ResnetBlock2D; ``emb`` None: no time embedding (the VAE's blocks).  ``eps`` defaults to the UNet's."""
    eps = SEMANTICS["eps_unet"] if eps is None else eps
    h = _conv(sd, p + ".conv1", F.silu(_gn(sd, p + ".norm1", x, eps)))
    if emb is not None:
        h = h + _lin(sd, p + ".time_emb_proj", F.silu(emb))[:, :, None, None]
    h = _conv(sd, p + ".conv2", F.silu(_gn(sd, p + ".norm2", h, eps)))
    cin, cout = x.shape[1], sd[p + ".conv1.weight"].shape[0]
    return (_conv(sd, p + ".conv_shortcut", x, padding=0) if cin != cout else x) + h


def resnet_cat(sd, p, x, skip, emb=None, eps=None):
    """the up blocks' call: the ResnetBlock on cat([x, skip], 1)"""
    return resnet(sd, p, torch.cat([x, skip] if SEMANTICS["cat_x_first"] else [skip, x], dim=1), emb, eps)


def attention(sd, p, x, context, heads):
    """UNet attention: bias-free to_q / to_k / to_v, heads split the last dimension contiguously, softmax over the keys"""
    ctx = x if context is None else context
    B, N, _ = x.shape
    q, k, v = _lin(sd, p + ".to_q", x, False), _lin(sd, p + ".to_k", ctx, False), _lin(sd, p + ".to_v", ctx, False)
    d = q.shape[-1] // heads
    q, k, v = (t.reshape(B, t.shape[1], heads, d).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax((q @ k.transpose(-1, -2)) * d ** SEMANTICS["attention_scale_exponent"], dim=-1)
    return _lin(sd, p + ".to_out.0", (w @ v).transpose(1, 2).reshape(B, N, heads * d))


def feed_forward(sd, p, x):
    a, b = _lin(sd, p + ".net.0.proj", x).chunk(2, dim=-1)
    hidden, gate = (a, b) if SEMANTICS["geglu_hidden_first"] else (b, a)
    return _lin(sd, p + ".net.2", hidden * F.gelu(gate, approximate=SEMANTICS["gelu"]))


def basic_transformer_block(sd, p, x, context, heads):
    x = x + attention(sd, p + ".attn1", _ln(sd, p + ".norm1", x), None, heads)
    x = x + attention(sd, p + ".attn2", _ln(sd, p + ".norm2", x), context, heads)
    return x + feed_forward(sd, p + ".ff", _ln(sd, p + ".norm3", x))


def transformer_2d(sd, p, x, context, heads, depth, linear_proj):
    _, _, H, W = x.shape
    h = _gn(sd, p + ".norm", x, SEMANTICS["eps_transformer"])
    h = _lin(sd, p + ".proj_in", _tokens(h)) if linear_proj else _tokens(_conv(sd, p + ".proj_in", h, padding=0))
    for i in range(depth):
        h = basic_transformer_block(sd, f"{p}.transformer_blocks.{i}", h, context, heads)
    h = _image(_lin(sd, p + ".proj_out", h), H, W) if linear_proj else _conv(sd, p + ".proj_out", _image(h, H, W), padding=0)
    return h + x


def downsample(sd, p, x):
    """UNet Downsample2D"""
    return _conv(sd, p + ".conv", x, stride=2, padding=1)


def upsample(sd, p, x):
    """Upsample2D (UNet and VAE decoder)"""
    return _conv(sd, p + ".conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))


def vae_downsample(sd, p, x):
    return _conv(sd, p + ".conv", F.pad(x, (0, 1, 0, 1) if SEMANTICS["asymmetric_pad"] else (1, 0, 1, 0)), stride=2, padding=0)


def vae_upsample(sd, p, x):
    return upsample(sd, p, x)


def vae_attention(sd, p, x):
    """one head of C channels over the H W pixels, to_q / to_k / to_v with bias, plus the input"""
    _, C, H, W = x.shape
    bias = SEMANTICS["vae_attention_bias"]
    h = _tokens(_gn(sd, p + ".group_norm", x, SEMANTICS["eps_vae"]))
    q, k, v = _lin(sd, p + ".to_q", h, bias), _lin(sd, p + ".to_k", h, bias), _lin(sd, p + ".to_v", h, bias)
    w = torch.softmax((q @ k.transpose(-1, -2)) * C ** SEMANTICS["attention_scale_exponent"], dim=-1)
    return _image(_lin(sd, p + ".to_out.0", w @ v), H, W) + x


def cond_embedding(sd, p, cond):
    """ControlNet condition embedding: conv_in, silu, three times (conv 3x3, silu, conv 3x3 stride 2, silu), conv_out"""
    h = F.silu(_conv(sd, p + ".conv_in", cond))
    for i in range(3):
        h = F.silu(_conv(sd, f"{p}.blocks.{2 * i}", h))
        h = F.silu(_conv(sd, f"{p}.blocks.{2 * i + 1}", h, stride=2))
    return _conv(sd, p + ".conv_out", h)


# ---- UNet / ControlNet ----------------------------------------------------------------------------------------------------------
def _unet_encoder(sd, prefix, cfg, x, emb, ctx):
    """down blocks + mid block from x = conv_in(.) on -> (mid output, skips)"""
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    skips = [x]
    for i in range(len(boc)):
        for j in range(L):
            x = resnet(sd, _p(prefix, f"down_blocks.{i}.resnets.{j}"), x, emb)
            if cfg["attn"][i]:
                x = transformer_2d(sd, _p(prefix, f"down_blocks.{i}.attentions.{j}"), x, ctx, cfg["heads"][i],
                                   cfg["transformer_depth"][i], cfg["use_linear_projection"])
            skips.append(x)
        if i < len(boc) - 1:
            x = downsample(sd, _p(prefix, f"down_blocks.{i}.downsamplers.0"), x)
            skips.append(x)
    m = _p(prefix, "mid_block")
    x = resnet(sd, m + ".resnets.0", x, emb)
    x = transformer_2d(sd, m + ".attentions.0", x, ctx, cfg["heads"][-1], cfg["transformer_depth"][-1], cfg["use_linear_projection"])
    return resnet(sd, m + ".resnets.1", x, emb), skips


def unet_forward(sd, cfg, sample, t, context, added=None, down_residuals=None, mid_residual=None, prefix=""):
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    n = len(boc)
    emb = time_embedding(sd, prefix, cfg, t, sample.shape[0], sample.dtype, added)
    x, skips = _unet_encoder(sd, prefix, cfg, _conv(sd, _p(prefix, "conv_in"), sample), emb, context)
    if down_residuals is not None:
        assert len(down_residuals) == len(skips)
        skips = [s + r for s, r in zip(skips, down_residuals)]
    if mid_residual is not None:
        x = x + mid_residual
    for i in range(n):
        lvl = n - 1 - i
        for j in range(L + 1):
            x = resnet_cat(sd, _p(prefix, f"up_blocks.{i}.resnets.{j}"), x, skips.pop(), emb)
            if cfg["attn"][lvl]:
                x = transformer_2d(sd, _p(prefix, f"up_blocks.{i}.attentions.{j}"), x, context, cfg["heads"][lvl],
                                   cfg["transformer_depth"][lvl], cfg["use_linear_projection"])
        if i < n - 1:
            x = upsample(sd, _p(prefix, f"up_blocks.{i}.upsamplers.0"), x)
    assert not skips
    return _conv(sd, _p(prefix, "conv_out"), F.silu(_gn(sd, _p(prefix, "conv_norm_out"), x, SEMANTICS["eps_unet"])))


def controlnet_forward(sd, cfg, sample, t, context, cond, conditioning_scale=1.0, added=None, prefix=""):
    """-> (down residuals, mid residual)"""
    emb = time_embedding(sd, prefix, cfg, t, sample.shape[0], sample.dtype, added)
    x = _conv(sd, _p(prefix, "conv_in"), sample) + cond_embedding(sd, _p(prefix, "controlnet_cond_embedding"), cond)
    x, skips = _unet_encoder(sd, prefix, cfg, x, emb, context)
    down = [_conv(sd, _p(prefix, f"controlnet_down_blocks.{i}"), s, padding=0) * conditioning_scale for i, s in enumerate(skips)]
    return down, _conv(sd, _p(prefix, "controlnet_mid_block"), x, padding=0) * conditioning_scale


# ---- AutoencoderKL --------------------------------------------------------------------------------------------------------------
def _vae_mid(sd, p, x):
    eps = SEMANTICS["eps_vae"]
    x = resnet(sd, p + ".resnets.0", x, None, eps)
    return resnet(sd, p + ".resnets.1", vae_attention(sd, p + ".attentions.0", x), None, eps)


def vae_encoder(sd, p, boc, x):
    eps = SEMANTICS["eps_vae"]
    x = _conv(sd, p + ".conv_in", x)
    for i in range(len(boc)):
        for j in range(2):
            x = resnet(sd, f"{p}.down_blocks.{i}.resnets.{j}", x, None, eps)
        if i < len(boc) - 1:
            x = vae_downsample(sd, f"{p}.down_blocks.{i}.downsamplers.0", x)
    x = _vae_mid(sd, p + ".mid_block", x)
    return _conv(sd, p + ".conv_out", F.silu(_gn(sd, p + ".conv_norm_out", x, eps)))


def vae_decoder(sd, p, boc, z):
    eps = SEMANTICS["eps_vae"]
    x = _vae_mid(sd, p + ".mid_block", _conv(sd, p + ".conv_in", z))
    for i in range(len(boc)):
        for j in range(3):
            x = resnet(sd, f"{p}.up_blocks.{i}.resnets.{j}", x, None, eps)
        if i < len(boc) - 1:
            x = vae_upsample(sd, f"{p}.up_blocks.{i}.upsamplers.0", x)
    return _conv(sd, p + ".conv_out", F.silu(_gn(sd, p + ".conv_norm_out", x, eps)))


def vae_encode(sd, boc, x, prefix=""):
    """-> (mean, std) of the diagonal Gaussian"""
    moments = _conv(sd, _p(prefix, "quant_conv"), vae_encoder(sd, _p(prefix, "encoder"), boc, x), padding=0)
    mean, logvar = moments.chunk(2, dim=1)
    return mean, torch.exp(0.5 * logvar.clamp(-30.0, 20.0))


def vae_decode(sd, boc, z, prefix=""):
    return vae_decoder(sd, _p(prefix, "decoder"), boc, _conv(sd, _p(prefix, "post_quant_conv"), z, padding=0))


# ---- test inputs ----------------------------------------------------------------------------------------------------------------
BATCH = 3
TIMESTEPS = (981, 500, 21)          # one per row; the scalar case uses the first
CONDITIONING_SCALE = 0.7
CONTEXT_TOKENS = 77
CONTEXT_SCALE = 4.0                 # default-initialised k projections of unit-variance text rows leave every cross-attention softmax
                                    # nearly uniform, and the query path (norm2, to_q) nearly invisible; CLIP's hidden states are not that tame
TIME_IDS = ((1024, 1024, 0, 0, 1024, 1024), (512, 768, 16, 32, 512, 768), (768, 512, 64, 8, 1024, 2048))


def unet_inputs(cfg, size=(16, 8), seed=0, dtype=torch.float64):
    """Non-trivial inputs of a UNet / ControlNet forward, batch 3 with every sample different and a latent of ``size`` = (height, width):
    dict(sample, t, context, added, cond)"""
    H, W = size
    g = torch.Generator().manual_seed(1000 + seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)

    added = None
    if cfg["addition_time_embed_dim"]:
        added = dict(text_embeds=rn(BATCH, cfg["pooled_projection_dim"]), time_ids=torch.tensor(TIME_IDS, dtype=torch.float32))
    return dict(sample=rn(BATCH, cfg["in_channels"], H, W), t=torch.tensor(TIMESTEPS),
                context=CONTEXT_SCALE * rn(BATCH, CONTEXT_TOKENS, cfg["cross_attention_dim"]), added=added,
                cond=torch.rand(BATCH, 3, 8 * H, 8 * W, generator=g, dtype=torch.float64).to(dtype))


def rel_l2(got, want):
    """relative L2 distance of two tensors, or of two equally long lists of tensors taken as one vector"""
    if isinstance(want, torch.Tensor):
        got, want = [got], [want]
    num = sum(float((a.double().cpu() - b.double().cpu()).pow(2).sum()) for a, b in zip(got, want))
    den = sum(float(b.double().cpu().pow(2).sum()) for b in want)
    return math.sqrt(num / den)
