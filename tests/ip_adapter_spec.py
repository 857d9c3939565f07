"""Test-side statement of the IP-Adapter semantics (test infrastructure, never shipped).

fp64-capable, functional, and -- like ``tests/sd_spec.py`` -- imports nothing from ``elasticdiffusion_official_amd``.  What it
states, from the published IP-Adapter / diffusers definitions (``IPAdapterAttnProcessor``, ``ImageProjection``):

* a cross attention whose state dict holds ``<p>.to_k_ip.weight`` reads its context as ``[text tokens | Ni image tokens]`` and
  computes ``to_out(softmax(q k_t^T s) v_t + scale * softmax(q k_i^T s) v_i)`` with ``k_t, v_t = to_k, to_v`` of the text part
  and ``k_i, v_i = to_k_ip, to_v_ip`` of the image part, both softmaxes at the attention's own scale ``s``;
* the image tokens are ``LayerNorm(Linear(clip_embeds).reshape(B, Ni, cross_dim))``; the unconditional rows take the projection
  of an all-zero embedding;
* file index -> layer: the n-th cross attention in the order down blocks, up blocks, mid block takes ``ip_adapter.{2n+1}``.

``decoupled(Ni, scale)`` swaps ``sd_spec.attention`` (looked up as a module global by ``basic_transformer_block`` at call time)
for the decoupled version, so ``sd_spec.unet_forward`` runs with an adapter; ``sd_spec.py`` itself is untouched.  ``DEFECTS`` names
deliberate mis-statements a test uses to show that its inputs would notice.
"""
import contextlib

import torch
import torch.nn.functional as F

from tests import sd_spec as S

DEFECTS = ("shared_softmax", "scale_on_text")


def image_tokens(state, clip_embeds, cross_dim, eps=1e-5):
    """[B, clip_dim] -> [B, Ni, cross_dim] with the adapter's flat ``image_proj.*`` tensors"""
    w, b = state["image_proj.proj.weight"], state["image_proj.proj.bias"]
    ni = w.shape[0] // cross_dim
    y = F.linear(clip_embeds.to(w.dtype), w, b).reshape(clip_embeds.shape[0], ni, cross_dim)
    return F.layer_norm(y, (cross_dim,), state["image_proj.norm.weight"], state["image_proj.norm.bias"], eps)


def uncond_image_tokens(state, batch, cross_dim):
    w = state["image_proj.proj.weight"]
    return image_tokens(state, torch.zeros(batch, w.shape[1], dtype=w.dtype), cross_dim)


def layer_prefixes(cfg):
    """UNet state-dict prefixes of the cross attentions in the file's order: down blocks by index, up blocks, mid block"""
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    n = len(boc)
    out = []
    for i in range(n):
        if cfg["attn"][i]:
            for j in range(L):
                out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.{d}.attn2" for d in range(cfg["transformer_depth"][i])]
    for i in range(n):
        lvl = n - 1 - i
        if cfg["attn"][lvl]:
            for j in range(L + 1):
                out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.{d}.attn2" for d in range(cfg["transformer_depth"][lvl])]
    out += [f"mid_block.attentions.0.transformer_blocks.{d}.attn2" for d in range(cfg["transformer_depth"][-1])]
    return out


def with_adapter(unet_state, adapter_state, cfg, order=None):
    """The UNet state dict plus ``<prefix>.to_k_ip.weight`` / ``.to_v_ip.weight`` from the flat adapter state.
    ``order``: a permutation of the layer list (a deliberate defect); None = the stated mapping."""
    prefixes = layer_prefixes(cfg)
    if order is not None:
        prefixes = [prefixes[i] for i in order]
    sd = dict(unet_state)
    for n, p in enumerate(prefixes):
        for name in ("to_k_ip", "to_v_ip"):
            sd[f"{p}.{name}.weight"] = adapter_state[f"ip_adapter.{2 * n + 1}.{name}.weight"]
    return sd


def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def attention(sd, p, x, context, heads, ni, scale, defect=None, plain=S.attention):
    """``sd_spec.attention`` where the state dict has no ``<p>.to_k_ip.weight`` (self attention, a UNet without adapter);
    decoupled cross attention on ``context = [text | ni image tokens]`` where it has"""
    if context is None or (p + ".to_k_ip.weight") not in sd:
        return plain(sd, p, x, context, heads)
    B, N, _ = x.shape
    text, image = context[:, :context.shape[1] - ni], context[:, context.shape[1] - ni:]
    lin = lambda name, t: F.linear(t, sd[f"{p}.{name}.weight"])   # noqa: E731 -- bias-free projections
    q = _heads(lin("to_q", x), heads)
    kt, vt = _heads(lin("to_k", text), heads), _heads(lin("to_v", text), heads)
    ki, vi = _heads(lin("to_k_ip", image), heads), _heads(lin("to_v_ip", image), heads)
    s = q.shape[-1] ** S.SEMANTICS["attention_scale_exponent"]
    if defect == "shared_softmax":
        w = torch.softmax((q @ torch.cat([kt, ki], 2).transpose(-1, -2)) * s, dim=-1)
        o = w[..., :kt.shape[2]] @ vt + scale * (w[..., kt.shape[2]:] @ vi)
    else:
        ot = torch.softmax((q @ kt.transpose(-1, -2)) * s, dim=-1) @ vt
        oi = torch.softmax((q @ ki.transpose(-1, -2)) * s, dim=-1) @ vi
        o = scale * ot + oi if defect == "scale_on_text" else ot + scale * oi
    o = o.transpose(1, 2).reshape(B, N, -1)
    return F.linear(o, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])


@contextlib.contextmanager
def decoupled(ni, scale, defect=None):
    """``sd_spec.attention`` replaced by the decoupled attention for the duration (restored on exit)"""
    if defect is not None and defect not in DEFECTS:
        raise KeyError(defect)
    plain = S.attention

    def swapped(sd, p, x, context, heads):
        return attention(sd, p, x, context, heads, ni, scale, defect, plain)
    S.attention = swapped
    try:
        yield
    finally:
        S.attention = plain


def unet_forward(unet_state, adapter_state, cfg, sample, t, context, scale, added=None, defect=None, order=None, **kw):
    """``sd_spec.unet_forward`` of a UNet carrying the adapter; ``context`` = [text | image tokens]"""
    ni = adapter_state["image_proj.proj.weight"].shape[0] // cfg["cross_attention_dim"]
    sd = with_adapter(unet_state, adapter_state, cfg, order)
    with decoupled(ni, scale, defect):
        return S.unet_forward(sd, cfg, sample, t, context, added, **kw)


def random_adapter(cfg, ni=4, clip_dim=48, seed=0, dtype=torch.float64, gain=1.0):
    """A flat adapter state for a UNet of ``cfg``: every tensor from its own seed, no affine parameter trivial.  to_k_ip / to_v_ip
    are drawn at ``gain`` / sqrt(cross_dim), so image keys have the spread of a default-initialised projection of unit rows."""
    cross = cfg["cross_attention_dim"]
    boc, n = cfg["block_out_channels"], len(cfg["block_out_channels"])

    def rn(s, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed * 100003 + s), dtype=torch.float64).to(dtype)
    state = {"image_proj.proj.weight": rn(1, ni * cross, clip_dim) / clip_dim ** 0.5, "image_proj.proj.bias": 0.2 * rn(2, ni * cross),
             "image_proj.norm.weight": 1.0 + 0.2 * rn(3, cross), "image_proj.norm.bias": 0.1 * rn(4, cross)}
    for i, p in enumerate(layer_prefixes(cfg)):
        where, idx = p.split(".")[0], int(p.split(".")[1]) if p.split(".")[1].isdigit() else 0
        lvl = idx if where == "down_blocks" else (n - 1 - idx if where == "up_blocks" else n - 1)
        inner = boc[lvl]
        state[f"ip_adapter.{2 * i + 1}.to_k_ip.weight"] = gain * rn(10 + 2 * i, inner, cross) / cross ** 0.5
        state[f"ip_adapter.{2 * i + 1}.to_v_ip.weight"] = gain * rn(11 + 2 * i, inner, cross) / cross ** 0.5
    return state
