"""Test-side statement of several IP-Adapters at once and of the Plus adapters' Resampler (test infrastructure, never shipped;
DESIGN.md section 32).

fp64-capable, functional, and -- like ``tests/sd_spec.py`` and ``tests/ip_adapter_spec.py`` -- imports nothing from
``elasticdiffusion_official_amd``.  What it states, from the published IP-Adapter definitions (``resampler.py``,
``IPAdapterAttnProcessor`` with several adapters):

* a cross attention carrying A adapters reads its context as ``[text | tokens of adapter 0 | adapter 1 | ...]`` and computes
  ``to_out(softmax(q k_t^T s) v_t + sum_a w[a] * softmax(q k_a^T s) v_a)``: every adapter has its own ``to_k_ip`` / ``to_v_ip``
  and its OWN softmax.  State-dict names: adapter 0 ``<p>.to_k_ip.weight``, adapter a >= 1 ``<p>.to_k_ip_{a}.weight`` (``to_v`` alike);
* the Resampler: ``latents`` [1, Ni, dim] attend over ``proj_in(x)`` and themselves through ``depth`` layers of
  (PerceiverAttention + residual, FeedForward + residual), then ``norm_out(proj_out(latents))``;
* PerceiverAttention: ``x = norm1(x)``, ``l = norm2(latents)``, ``q = to_q(l)``, ``k, v = to_kv(cat([x, l], -2)).chunk(2)``,
  ``softmax((q dh^-1/4)(k dh^-1/4)^T) v`` over heads of 64, ``to_out``; all three projections bias-free;
* FeedForward = LayerNorm, Linear (no bias), exact-erf GELU, Linear (no bias); every LayerNorm has eps 1e-5.

``DEFECTS`` / ``RESAMPLER_DEFECTS`` name deliberate mis-statements a test uses to show that its inputs would notice.
"""
import contextlib

import torch
import torch.nn.functional as F

from tests import ip_adapter_spec as IS
from tests import sd_spec as S

DEFECTS = ("shared_softmax", "weights_swapped")
RESAMPLER_DEFECTS = ("no_latents_in_keys", "norms_swapped", "no_residual", "no_norm_out")
DIM_HEAD = 64
EPS = 1e-5


# ---- the operation on q / k / v (what the kernel is judged against) ------------------------------------------------------------
def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def softmax_v(q, k, v, heads, dtype=torch.float64):
    """softmax(q k^T / sqrt(d)) v per head in ``dtype`` on the values as given -> [B, Nq, H d]"""
    B, Nq, HD = q.shape
    qf, kf, vf = (_heads(t.to(dtype), heads) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) * (HD // heads) ** -0.5
    return (torch.softmax(s, dim=-1) @ vf).transpose(1, 2).reshape(B, Nq, HD)


def segments(n_text, n_image):
    """[(start, stop)] of the text rows and of every adapter's rows in k / v"""
    out, off = [(0, n_text)], n_text
    for n in n_image:
        out.append((off, off + n))
        off += n
    return out


def multi_ref(q, k, v, heads, n_text, n_image, w, dtype=torch.float64):
    """text + sum_a w[a] * segment a, one softmax per segment; ``w`` a sequence of floats or a tensor [A]"""
    seg = segments(n_text, n_image)
    out = softmax_v(q, k[:, :n_text], v[:, :n_text], heads, dtype)
    for a, (lo, hi) in enumerate(seg[1:]):
        out = out + float(w[a]) * softmax_v(q, k[:, lo:hi], v[:, lo:hi], heads, dtype)
    return out


# ---- the attention layer with A adapters ----------------------------------------------------------------------------------------
def ip_names(a):
    return ("to_k_ip", "to_v_ip") if a == 0 else (f"to_k_ip_{a}", f"to_v_ip_{a}")


def attention(sd, p, x, context, heads, n_image, weights, defect=None, plain=S.attention):
    """``sd_spec.attention`` where the state dict has no ``<p>.to_k_ip.weight``; the A-term decoupled cross attention where it has"""
    if context is None or (p + ".to_k_ip.weight") not in sd:
        return plain(sd, p, x, context, heads)
    B, N, _ = x.shape
    nt = context.shape[1] - sum(n_image)
    lin = lambda name, t: F.linear(t, sd[f"{p}.{name}.weight"])   # noqa: E731 -- bias-free projections
    q = _heads(lin("to_q", x), heads)
    s = q.shape[-1] ** S.SEMANTICS["attention_scale_exponent"]
    text = context[:, :nt]
    o = torch.softmax((q @ _heads(lin("to_k", text), heads).transpose(-1, -2)) * s, dim=-1) @ _heads(lin("to_v", text), heads)
    ws = list(weights)
    if defect == "weights_swapped":
        ws[0], ws[1] = ws[1], ws[0]
    ks, vs = [], []
    for a, (lo, hi) in enumerate(segments(nt, n_image)[1:]):
        kn, vn = ip_names(a)
        ks.append(_heads(lin(kn, context[:, lo:hi]), heads)), vs.append(_heads(lin(vn, context[:, lo:hi]), heads))
    if defect == "shared_softmax":      # adapters 0 and 1 under one softmax
        pr = torch.softmax((q @ torch.cat(ks[:2], 2).transpose(-1, -2)) * s, dim=-1)
        n0 = ks[0].shape[2]
        o = o + ws[0] * (pr[..., :n0] @ vs[0]) + ws[1] * (pr[..., n0:] @ vs[1])
        rest = range(2, len(ks))
    else:
        rest = range(len(ks))
    for a in rest:
        o = o + ws[a] * (torch.softmax((q @ ks[a].transpose(-1, -2)) * s, dim=-1) @ vs[a])
    o = o.transpose(1, 2).reshape(B, N, -1)
    return F.linear(o, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])


@contextlib.contextmanager
def decoupled(n_image, weights, defect=None):
    if defect is not None and defect not in DEFECTS:
        raise KeyError(defect)
    plain = S.attention

    def swapped(sd, p, x, context, heads):
        return attention(sd, p, x, context, heads, n_image, weights, defect, plain)
    S.attention = swapped
    try:
        yield
    finally:
        S.attention = plain


def with_adapters(unet_state, adapters, cfg):
    """The UNet state dict plus every adapter's per-layer projections under ``ip_names(a)``"""
    sd = dict(unet_state)
    for a, ad in enumerate(adapters):
        for n, p in enumerate(IS.layer_prefixes(cfg)):
            for name, src in zip(ip_names(a), ("to_k_ip", "to_v_ip")):
                sd[f"{p}.{name}.weight"] = ad[f"ip_adapter.{2 * n + 1}.{src}.weight"]
    return sd


def unet_forward(unet_state, adapters, cfg, sample, t, context, n_image, weights, added=None, defect=None, **kw):
    """``sd_spec.unet_forward`` of a UNet carrying the adapters; ``context`` = [text | tokens 0 | tokens 1 | ...]"""
    sd = with_adapters(unet_state, adapters, cfg)
    with decoupled(tuple(n_image), tuple(weights), defect):
        return S.unet_forward(sd, cfg, sample, t, context, added, **kw)


# ---- the Resampler ----------------------------------------------------------------------------------------------------------------
def _ln(state, key, x):
    return F.layer_norm(x, (x.shape[-1],), state[key + ".weight"], state[key + ".bias"], EPS)


def perceiver_attention(state, p, x, latents, defect=None):
    n1, n2 = ("norm2", "norm1") if defect == "norms_swapped" else ("norm1", "norm2")
    x, lat = _ln(state, f"{p}.{n1}", x), _ln(state, f"{p}.{n2}", latents)
    inner = state[f"{p}.to_q.weight"].shape[0]
    heads = inner // DIM_HEAD
    q = F.linear(lat, state[f"{p}.to_q.weight"])
    kv_in = x if defect == "no_latents_in_keys" else torch.cat([x, lat], dim=-2)
    k, v = F.linear(kv_in, state[f"{p}.to_kv.weight"]).chunk(2, dim=-1)
    q, k, v = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    c = DIM_HEAD ** -0.25
    o = torch.softmax((q * c) @ (k * c).transpose(-1, -2), dim=-1) @ v
    B, _, N, _ = o.shape
    return F.linear(o.transpose(1, 2).reshape(B, N, inner), state[f"{p}.to_out.weight"])


def feed_forward(state, p, x):
    h = F.linear(_ln(state, f"{p}.0", x), state[f"{p}.1.weight"])
    return F.linear(F.gelu(h), state[f"{p}.3.weight"])       # F.gelu's default is the exact erf form


def resampler(state, x, defect=None):
    """[B, S, embed_dim] (the CLIP vision model's penultimate hidden states) -> [B, Ni, cross_dim] image tokens, with the flat
    ``image_proj.*`` tensors of a Plus adapter"""
    if defect is not None and defect not in RESAMPLER_DEFECTS:
        raise KeyError(defect)
    pre = "image_proj"
    lat = state[f"{pre}.latents"].to(x.dtype).repeat(x.shape[0], 1, 1)
    x = F.linear(x, state[f"{pre}.proj_in.weight"], state[f"{pre}.proj_in.bias"])
    depth = 1 + max(int(k.split(".")[2]) for k in state if k.startswith(f"{pre}.layers."))
    for i in range(depth):
        a = perceiver_attention(state, f"{pre}.layers.{i}.0", x, lat, defect)
        lat = a if (defect == "no_residual" and i == 0) else a + lat
        lat = feed_forward(state, f"{pre}.layers.{i}.1", lat) + lat
    lat = F.linear(lat, state[f"{pre}.proj_out.weight"], state[f"{pre}.proj_out.bias"])
    return lat if defect == "no_norm_out" else _ln(state, f"{pre}.norm_out", lat)


def random_resampler(cross, ni=16, embed_dim=80, dim=128, depth=2, heads=2, ff_mult=2, seed=0, dtype=torch.float64):
    """flat ``image_proj.*`` tensors of a Resampler, every tensor from its own seed, no affine parameter trivial"""
    def rn(s, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed * 100003 + 7000 + s), dtype=torch.float64).to(dtype)
    inner, ffi = heads * DIM_HEAD, ff_mult * dim
    st = {"image_proj.latents": rn(1, 1, ni, dim) / dim ** 0.5 * 4.0,
          "image_proj.proj_in.weight": rn(2, dim, embed_dim) / embed_dim ** 0.5, "image_proj.proj_in.bias": 0.2 * rn(3, dim),
          "image_proj.proj_out.weight": rn(4, cross, dim) / dim ** 0.5, "image_proj.proj_out.bias": 0.2 * rn(5, cross),
          "image_proj.norm_out.weight": 1.0 + 0.2 * rn(6, cross), "image_proj.norm_out.bias": 0.1 * rn(7, cross)}
    for i in range(depth):
        p, s = f"image_proj.layers.{i}", 20 + 20 * i
        for j, n in enumerate(("norm1", "norm2")):
            st[f"{p}.0.{n}.weight"], st[f"{p}.0.{n}.bias"] = 1.0 + 0.3 * rn(s + 2 * j, dim), 0.3 * rn(s + 2 * j + 1, dim)
        st[f"{p}.0.to_q.weight"] = 2.0 * rn(s + 4, inner, dim) / dim ** 0.5
        st[f"{p}.0.to_kv.weight"] = 2.0 * rn(s + 5, 2 * inner, dim) / dim ** 0.5
        st[f"{p}.0.to_out.weight"] = rn(s + 6, dim, inner) / inner ** 0.5
        st[f"{p}.1.0.weight"], st[f"{p}.1.0.bias"] = 1.0 + 0.2 * rn(s + 7, dim), 0.1 * rn(s + 8, dim)
        st[f"{p}.1.1.weight"] = rn(s + 9, ffi, dim) / dim ** 0.5
        st[f"{p}.1.3.weight"] = rn(s + 10, dim, ffi) / ffi ** 0.5
    return st


def random_plus_adapter(cfg, ni=16, embed_dim=80, seed=0, dtype=torch.float64, gain=1.0, **kw):
    """A flat Plus adapter for a UNet of ``cfg``: ``random_resampler``'s image projection and ``ip_adapter_spec.random_adapter``'s
    per-layer projections"""
    base = IS.random_adapter(cfg, ni, 8, seed=seed, dtype=dtype, gain=gain)
    st = {k: v for k, v in base.items() if k.startswith("ip_adapter.")}
    st.update(random_resampler(cfg["cross_attention_dim"], ni, embed_dim, seed=seed, dtype=dtype, **kw))
    return st


def image_tokens(state, embeds, cross_dim):
    """either adapter type: the Resampler where the state has one, ``ip_adapter_spec.image_tokens`` otherwise"""
    if "image_proj.latents" in state:
        return resampler(state, embeds.to(state["image_proj.latents"].dtype))
    return IS.image_tokens(state, embeds, cross_dim)
