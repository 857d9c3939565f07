"""Test-side statement of IP-Adapter attention masks (test infrastructure, never shipped).

Functional, fp64-capable and -- like the other ``*_spec.py`` files -- imports nothing from ``elasticdiffusion_official_amd``.

* **Mask value.**  Adapter a's mask is ``fp32(u8) / 255`` (one rounding) at latent resolution [H/8, W/8]; no mask means all ones.
* **Row frames.**  A model row is not the picture: a global row of resampling step k holds, at (y, x) inside the picked frame
  (``g_off_y <= y < g_off_y + h`` ...), the latent of source pixel ``(src_row[2 i + (q >> 1)], src_col[2 j + (q & 1)])`` with
  ``q = idx[k, i w + j]``; a view row holds the window at (win_y0[v], win_x0[v]).  The row's level-0 mask frame is THAT gather
  applied to the mask, and 0 wherever the latent channels do not read the picture (pad strips, context outside the picture).
  The ``copies`` rows of a step (uncond, cond, regional conds) share their frame.  Rows: global rows step-major, then view rows.
* **Levels.**  Level L + 1 is the 2 x 2 mean of level L, ``0.25 * ((l[2y,2x] + l[2y,2x+1]) + (l[2y+1,2x] + l[2y+1,2x+1]))``,
  every operation rounded in the working dtype in that association.  A cross attention with (PH >> L)(PW >> L) query rows reads
  level L at query index ``i = y (PW >> L) + x``.
* **Attention.**  ``softmax(q k_t^T s) v_t + sum_a (w[a] m_a[row, i]) softmax(q k_a^T s) v_a``: the mask multiplies adapter a's
  whole term at query row i -- not the text term, not the scores inside a softmax.

``DEFECTS`` names deliberate mis-statements a test uses to show that its inputs would notice each of them.
"""
import contextlib

import torch
import torch.nn.functional as F

from tests import ip_adapter_multi_spec as MS
from tests import sd_spec as S

LEVELS = 4
DEFECTS = ("mask_on_text", "masks_swapped", "level_stride", "key_mask", "pad_one")


def layout(PH, PW):
    """([(offset, count)] of levels 0..3 inside one row's flat mask, S)"""
    sizes = [(PH >> L) * (PW >> L) for L in range(LEVELS)]
    return [(sum(sizes[:L]), sizes[L]) for L in range(LEVELS)], sum(sizes)


def mask_values(u8):
    """uint8 [..] -> fp32(u8) / 255, rounded once"""
    return u8.to(torch.float32) / 255.0


def row_frames(masks, idx, src_row, src_col, h, w, g_off_y, g_off_x, win_y0, win_x0, Sh, Sw, v_off_y, v_off_x, PH, PW, copies,
               pad=0.0):
    """masks [B,A,H,W]; idx u8 [K,h*w] (or None), src_row [2h], src_col [2w]; win_y0 / win_x0 [V] (or None) -> level 0 of every
    row, [(K*copies + V)*B, A, PH, PW] in masks' dtype.  ``pad``: the value where the row does not read the picture (the rule: 0)."""
    B, A, H, W = masks.shape
    out = []
    K = 0 if idx is None else idx.shape[0]
    for k in range(K):
        q = idx[k].reshape(h, w).long()
        sy = src_row.long().reshape(h, 2).gather(1, q >> 1)                        # [h,w]: src_row[2 i + (q >> 1)]
        sx = src_col.long().reshape(w, 2).t().gather(0, q & 1)                     # [h,w]: src_col[2 j + (q & 1)]
        frame = torch.full((B, A, PH, PW), pad, dtype=masks.dtype)
        frame[:, :, g_off_y:g_off_y + h, g_off_x:g_off_x + w] = masks[:, :, sy, sx]
        out.extend([frame] * copies)                                               # row (k * copies + c) * B + b
    V = 0 if win_y0 is None else len(win_y0)
    for v in range(V):
        frame = torch.full((B, A, PH, PW), pad, dtype=masks.dtype)
        for yy in range(Sh):
            sy = int(win_y0[v]) + yy
            for xx in range(Sw):
                sx = int(win_x0[v]) + xx
                inside = 0 <= sy < H and 0 <= sx < W
                frame[:, :, v_off_y + yy, v_off_x + xx] = masks[:, :, sy, sx] if inside else pad
        out.append(frame)
    return torch.cat(out, 0) if out else torch.zeros(0, A, PH, PW, dtype=masks.dtype)


def pyramid(l0):
    """[.., PH, PW] -> the four levels, each operation rounded in l0's dtype, in the stated association"""
    levels = [l0]
    for _ in range(LEVELS - 1):
        l = levels[-1]
        quarter = torch.tensor(0.25, dtype=l.dtype)
        levels.append(quarter * ((l[..., 0::2, 0::2] + l[..., 0::2, 1::2]) + (l[..., 1::2, 0::2] + l[..., 1::2, 1::2])))
    return levels


def flatten(levels):
    """the four levels -> [.., S], level L at ``layout``'s offset"""
    return torch.cat([l.reshape(*l.shape[:-2], -1) for l in levels], dim=-1)


def mask_rows(masks, *gather, pad=0.0):
    """``row_frames`` then ``pyramid``: [(K*copies + V)*B, A, S]"""
    return flatten(pyramid(row_frames(masks, *gather, pad=pad)))


def level_of(m, PH, PW, N, defect=None):
    """m [B,A,S] -> [B,A,N]: the level a cross attention of N query rows reads"""
    lay, S_ = layout(PH, PW)
    for L, (off, n) in enumerate(lay):
        if n == N:
            if defect == "level_stride":      # level L addressed with the row pitch of level L - 1 (twice its own)
                hh, ww = PH >> L, PW >> L
                y, x = torch.meshgrid(torch.arange(hh), torch.arange(ww), indexing="ij")
                return m[:, :, (off + y * (2 * ww) + x).reshape(-1) % S_]
            return m[:, :, off:off + n]
    raise ValueError(f"{N} query rows match no level of a {PH} x {PW} row")


# ---- the operation on q / k / v (what the kernel is judged against) ------------------------------------------------------------
def masked_ref(q, k, v, heads, n_text, n_image, w, m, dtype=torch.float64):
    """text + sum_a (w[a] m[:, a, :, None]) * segment a; m [B or 1, A, Nq]"""
    seg = MS.segments(n_text, n_image)
    out = MS.softmax_v(q, k[:, :n_text], v[:, :n_text], heads, dtype)
    for a, (lo, hi) in enumerate(seg[1:]):
        coef = (torch.as_tensor(w, dtype=torch.float32)[a] * m[:, a].to(torch.float32)).to(dtype)   # fl(w m), the kernel's one rounding
        out = out + coef[..., None] * MS.softmax_v(q, k[:, lo:hi], v[:, lo:hi], heads, dtype)
    return out


# ---- the attention layer ---------------------------------------------------------------------------------------------------------
def attention(sd, p, x, context, heads, n_image, weights, m, PH, PW, defect=None, plain=S.attention):
    """``sd_spec.attention`` where the state dict carries no adapter; the masked decoupled cross attention where it does"""
    if context is None or (p + ".to_k_ip.weight") not in sd:
        return plain(sd, p, x, context, heads)
    B, N, _ = x.shape
    nt = context.shape[1] - sum(n_image)
    lin = lambda name, t: F.linear(t, sd[f"{p}.{name}.weight"])   # noqa: E731 -- bias-free projections
    q = MS._heads(lin("to_q", x), heads)
    s = q.shape[-1] ** S.SEMANTICS["attention_scale_exponent"]
    mv = level_of(m, PH, PW, N, defect).to(x.dtype)                # [B,A,N]
    if defect == "masks_swapped":
        mv = mv[:, [1, 0] + list(range(2, mv.shape[1]))]
    text = context[:, :nt]
    o = torch.softmax((q @ MS._heads(lin("to_k", text), heads).transpose(-1, -2)) * s, dim=-1) @ MS._heads(lin("to_v", text), heads)
    if defect == "mask_on_text":
        o = o * mv[:, 0, None, :, None]
    for a, (lo, hi) in enumerate(MS.segments(nt, n_image)[1:]):
        kn, vn = MS.ip_names(a)
        ka, va = MS._heads(lin(kn, context[:, lo:hi]), heads), MS._heads(lin(vn, context[:, lo:hi]), heads)
        if defect == "key_mask":              # the mask inside the softmax, as a bias log(m) on the keys' scores: a no-op per row
            sc = (q @ ka.transpose(-1, -2)) * s + torch.log(mv[:, a].clamp_min(1e-30))[:, None, :, None]
            o = o + weights[a] * (torch.softmax(sc, dim=-1) @ va)
        else:
            o = o + (weights[a] * mv[:, a])[:, None, :, None] * (torch.softmax((q @ ka.transpose(-1, -2)) * s, dim=-1) @ va)
    o = o.transpose(1, 2).reshape(B, N, -1)
    return F.linear(o, sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])


@contextlib.contextmanager
def masked(n_image, weights, m, PH, PW, defect=None):
    if defect is not None and defect not in DEFECTS:
        raise KeyError(defect)
    plain = S.attention

    def swapped(sd, p, x, context, heads):
        return attention(sd, p, x, context, heads, n_image, weights, m, PH, PW, defect, plain)
    S.attention = swapped
    try:
        yield
    finally:
        S.attention = plain


def unet_forward(unet_state, adapters, cfg, sample, t, context, n_image, weights, m, PH, PW, added=None, defect=None, **kw):
    """``sd_spec.unet_forward`` of a UNet carrying the adapters, every cross attention masked; m [B,A,S] as ``mask_rows`` gives it"""
    sd = MS.with_adapters(unet_state, adapters, cfg)
    with masked(tuple(n_image), tuple(weights), m, PH, PW, defect):
        return S.unet_forward(sd, cfg, sample, t, context, added, **kw)
