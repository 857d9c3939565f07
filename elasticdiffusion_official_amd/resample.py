"""Fixed-point coefficient tables of Pillow's 8-bit resampler (``Image.resize`` with an antialiased filter), on the host.

Pure Python: no torch, no GPU.  ``ops.resize_u8`` uploads these tables and the HIP kernels of csrc/resize_kernels.hip do the
integer accumulation; tests/resize_cpu.py does the same in numpy.  The arithmetic is written out in DESIGN.md §15.

Along one axis, ``in_size`` -> ``out_size`` with a filter of support ``s``:

    scale = in / out, fs = max(scale, 1), support = s * fs, ksize = 2 * ceil(support) + 1
    per output xx:  center = (xx + 0.5) * scale
                    xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - xmin
                    w[x] = f((x + xmin - center + 0.5) * (1 / fs)) for x < n, divided by their sum (taken in index order) unless it is 0
                    k[x] = int(w * 2^22 -+ 0.5)   (away from zero)

``(1 / fs)`` is a rounded double that multiplies, as in Pillow's C; a division by ``fs`` differs from it in the last place.
"""
import math
from functools import lru_cache

PRECISION_BITS = 22                  # 255 * sum |k| stays below 2^31: the accumulator is int32
MAX_DIM = 8192                       # bound of the kernels (ed_resize_rows_u8 / ed_resize_cols_u8)


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x           # the C library's sin: numpy's may differ in the last place


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0), "bilinear": (_bilinear, 1.0)}


def ksize(in_size, out_size, filter):
    """Width of the coefficient table: 2 * ceil(support * max(in / out, 1)) + 1."""
    support = FILTERS[filter][1] * max(in_size / out_size, 1.0)
    return int(math.ceil(support)) * 2 + 1


def coefficient_lists(in_size, out_size, filter):
    """-> (rows, bounds): ``rows[xx]`` the ``n`` int coefficients of output ``xx`` (not padded), ``bounds[xx] = (xmin, n)``."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    f, s = FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = s * fs
    ss = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    rows, bounds = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append([int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w])
        bounds.append((xmin, n))
    return rows, bounds


@lru_cache(maxsize=64)
def _table(in_size, out_size, filter):
    import numpy as np
    rows, bounds = coefficient_lists(in_size, out_size, filter)
    coeff = np.zeros((out_size, ksize(in_size, out_size, filter)), np.int32)
    for xx, r in enumerate(rows):
        coeff[xx, :len(r)] = r
    b = np.asarray(bounds, np.int32).reshape(out_size, 2)
    coeff.setflags(write=False)
    b.setflags(write=False)
    return coeff, b


def coefficients(in_size, out_size, filter="bicubic"):
    """-> (coeff int32 [out, ksize] zero-padded, bounds int32 [out, 2] = (xmin, n)); cached per (in, out, filter), read-only."""
    return _table(int(in_size), int(out_size), filter)


def plan(in_hw, out_hw, filter="bicubic"):
    """The passes of a two-dimensional resize (H, W) -> (H_out, W_out), in order.  A pass whose size does not change is absent.

    -> list of ("rows", coeff, bounds, y0, y1) / ("cols", coeff, bounds): the horizontal pass covers the source rows [y0, y1) the
    vertical pass reads, and the vertical bounds are already shifted by -y0."""
    (H, W), (Ho, Wo) = in_hw, out_hw
    passes = []
    y0, y1 = 0, H
    vert = None
    if Ho != H:
        kv, bv = coefficients(H, Ho, filter)
        if Wo != W:                                    # the intermediate holds only the rows the vertical pass needs
            y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
            bv = bv.copy()
            bv[:, 0] -= y0
        vert = ("cols", kv, bv)
    if Wo != W:
        kh, bh = coefficients(W, Wo, filter)
        passes.append(("rows", kh, bh, y0, y1))
    if vert:
        passes.append(vert)
    return passes
