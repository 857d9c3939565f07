"""torch-CPU restatement of ``ed_ip_mask_rows`` in fp32 (test infrastructure): the bits the kernel must give.

Index arithmetic on whole tensors, every fp32 operation of the pyramid a separate torch op (torch's CPU kernels neither contract
nor re-associate), so ``mask_rows`` is bit-comparable with the device buffer.  Not a conftest and not collected.
"""
import torch

LEVELS = 4


def layout(PH, PW):
    sizes = [(PH >> L) * (PW >> L) for L in range(LEVELS)]
    return [(sum(sizes[:L]), sizes[L]) for L in range(LEVELS)], sum(sizes)


def u8_masks(B, A, H, W, seed):
    """uint8 masks with exact 0, exact 255 and graded k / 255 pixels, as fp32 values in [0, 1]: [B,A,H,W]"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 256, (B, A, H, W), generator=g, dtype=torch.uint8)
    sel = torch.rand(B, A, H, W, generator=g)
    m[sel < 0.3] = 0
    m[sel > 0.7] = 255
    return m.to(torch.float32) / 255.0


def level0(masks, idx, src_row, src_col, h, w, g_off_y, g_off_x, win_y0, win_x0, Sh, Sw, v_off_y, v_off_x, PH, PW, copies):
    """-> f32 [(K*copies + V)*B, A, PH, PW]; all index tensors on the CPU, idx / win_y0 may be None"""
    B, A, H, W = masks.shape
    parts = []
    if idx is not None and idx.shape[0]:
        K = idx.shape[0]
        q = idx.reshape(K, h, w).long()
        i = torch.arange(h).view(1, h, 1).expand(K, h, w)
        j = torch.arange(w).view(1, 1, w).expand(K, h, w)
        sy = src_row.long()[2 * i + (q >> 1)]
        sx = src_col.long()[2 * j + (q & 1)]
        g = torch.zeros(K, B, A, PH, PW, dtype=torch.float32)
        g[:, :, :, g_off_y:g_off_y + h, g_off_x:g_off_x + w] = masks[:, :, sy, sx].permute(2, 0, 1, 3, 4)
        parts.append(g[:, None].expand(K, copies, B, A, PH, PW).reshape(K * copies * B, A, PH, PW))
    if win_y0 is not None and len(win_y0):
        V = len(win_y0)
        sy = win_y0.long().view(V, 1) + torch.arange(Sh).view(1, Sh)                 # [V,Sh]
        sx = win_x0.long().view(V, 1) + torch.arange(Sw).view(1, Sw)                 # [V,Sw]
        ok = ((sy >= 0) & (sy < H))[:, :, None] & ((sx >= 0) & (sx < W))[:, None, :]  # [V,Sh,Sw]
        val = masks[:, :, sy.clamp(0, H - 1)[:, :, None], sx.clamp(0, W - 1)[:, None, :]]   # [B,A,V,Sh,Sw]
        val = torch.where(ok, val, torch.zeros((), dtype=torch.float32)).permute(2, 0, 1, 3, 4)
        v = torch.zeros(V, B, A, PH, PW, dtype=torch.float32)
        v[:, :, :, v_off_y:v_off_y + Sh, v_off_x:v_off_x + Sw] = val
        parts.append(v.reshape(V * B, A, PH, PW))
    return torch.cat(parts, 0)


def pyramid(l0):
    out = [l0]
    for _ in range(LEVELS - 1):
        l = out[-1]
        top = l[..., 0::2, 0::2] + l[..., 0::2, 1::2]
        bot = l[..., 1::2, 0::2] + l[..., 1::2, 1::2]
        out.append(0.25 * (top + bot))
    return out


def mask_rows(masks, *gather):
    """-> f32 [(K*copies + V)*B, A, S]: what ``ops.ip_mask_rows`` must return, bit for bit"""
    return torch.cat([l.reshape(*l.shape[:-2], -1) for l in pyramid(level0(masks, *gather))], dim=-1).contiguous()
