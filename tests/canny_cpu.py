"""numpy restatement of the Canny specification in DESIGN.md ("Canny condition extraction"): OpenCV 4.x
``cv::Canny(src, edges, t1, t2, apertureSize=3, L2gradient=False)`` for 8-bit input.  A test helper, not product: the
product path is csrc/canny_kernels.hip.  Everything is integer arithmetic, so the HIP kernels must match it exactly.

    canny_map(img, low, high)  -> uint8 map, 1 = not an edge, 0 = candidate, 2 = strong
    hysteresis(map)            -> (map with connected candidates promoted to 2, number of one-pixel dilation passes)
    canny(img, low, high)      -> uint8 [H, W] edges, 255 / 0
"""
import math

import numpy as np


def _as_hwc(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return img[:, :, None] if img.ndim == 2 else img


def thresholds(low, high):
    low, high = int(math.floor(low)), int(math.floor(high))
    return (high, low) if low > high else (low, high)


def gradients(img):
    """-> dx, dy, m (int32 [H, W]) of the channel with the largest |dx| + |dy| (lowest index on ties)."""
    a = np.pad(_as_hwc(img).astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = a.shape[0] - 2, a.shape[1] - 2

    def s(dy, dx):
        return a[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    dx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    dy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    n = np.abs(dx) + np.abs(dy)
    k = np.argmax(n, axis=2)[:, :, None]        # first maximum = the strict '>' scan over k = 1..C-1
    pick = lambda v: np.take_along_axis(v, k, axis=2)[:, :, 0]  # noqa: E731
    return pick(dx), pick(dy), pick(n)


def canny_map(img, low=100, high=200):
    low, high = thresholds(low, high)
    dx, dy, m = gradients(img)
    H, W = m.shape
    mp = np.pad(m, 1)                            # magnitude outside the image is 0

    def nb(di, dj):
        return mp[1 + di:1 + di + H, 1 + dj:1 + dj + W]

    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    tg22x = x * 13573
    tg67x = tg22x + (x << 16)
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    neg = (dx ^ dy) < 0                          # s = -1
    keep_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    keep_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    keep_d = np.where(neg, (m > nb(-1, 1)) & (m > nb(1, -1)), (m > nb(-1, -1)) & (m > nb(1, 1)))
    keep = (m > low) & np.where(horiz, keep_h, np.where(vert, keep_v, keep_d))
    out = np.ones((H, W), np.uint8)
    out[keep & (m <= high)] = 0
    out[keep & (m > high)] = 2
    return out


def hysteresis(cmap):
    """Breadth-first flood from the strong pixels through the candidates (8-connectivity).  Wave k promotes exactly the
    candidates that a k-th one-pixel dilation of the strong set would reach, so the number of waves run (the last,
    empty one included) is the number of passes a one-pixel-per-pass dilation needs to see that nothing changes."""
    out = np.array(cmap, dtype=np.uint8, copy=True)
    H, W = out.shape
    pad = np.ones((H + 2, W + 2), np.uint8)
    pad[1:-1, 1:-1] = out
    fy, fx = np.nonzero(pad == 2)
    passes = 0
    while True:
        passes += 1
        ny = np.concatenate([fy + d for d in (-1, -1, -1, 0, 0, 1, 1, 1)])
        nx = np.concatenate([fx + d for d in (-1, 0, 1, -1, 1, -1, 0, 1)])
        hit = pad[ny, nx] == 0
        if not hit.any():
            break
        ny, nx = ny[hit], nx[hit]
        pad[ny, nx] = 2
        flat = np.unique(ny.astype(np.int64) * (W + 2) + nx)
        fy, fx = flat // (W + 2), flat % (W + 2)
    return pad[1:-1, 1:-1].copy(), passes


def hysteresis_by_labels(cmap):
    """The independent formulation: a connected component (8-connectivity) of ``map != 1`` is kept iff it holds a 2."""
    from scipy import ndimage
    lab, n = ndimage.label(cmap != 1, structure=np.ones((3, 3), int))
    has_strong = np.zeros(n + 1, bool)
    has_strong[lab[cmap == 2]] = True
    has_strong[0] = False
    out = np.array(cmap, dtype=np.uint8, copy=True)
    out[has_strong[lab]] = 2
    return out


def canny(img, low=100, high=200):
    promoted, _ = hysteresis(canny_map(img, low, high))
    return np.where(promoted == 2, 255, 0).astype(np.uint8)


def box_blur(img, k=5):
    """Box blur of a uint8 image with an edge-replicated border (long, smooth chains for the tests); integer mean."""
    a = _as_hwc(img).astype(np.int64)
    r = k // 2
    p = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    H, W = a.shape[:2]
    acc = sum(p[i:i + H, j:j + W] for i in range(k) for j in range(k))
    out = (acc // (k * k)).astype(np.uint8)
    return out[:, :, 0] if np.asarray(img).ndim == 2 else out


def spiral_path(n=1024, pitch=16, margin=8):
    """One-pixel-wide rectangular spiral from (margin, margin) inwards, arms ``pitch`` apart -> int array [N, 2] of (y, x) in
    path order: one long chain that re-enters every tile many times (hysteresis tests and timing)."""
    y = x = margin
    pts = [(y, x)]
    length, k = n - 1 - 2 * margin, 0
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    while length > 0:
        dy, dx = dirs[k % 4]
        for _ in range(length):
            y, x = y + dy, x + dx
            pts.append((y, x))
        k += 1
        if k >= 3 and k % 2 == 1:
            length -= pitch
    return np.array(pts)
