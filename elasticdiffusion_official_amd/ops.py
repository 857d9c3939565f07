"""Torch-tensor wrappers over the C ABI (include/elastic_hip.h).  PyTorch is only plumbing here: it owns the device
buffers and the stream; every wrapper validates its arguments, passes raw device pointers and raises on a HIP
error.  No wrapper has a fallback path -- a tensor that is not on a ROCm device is an error.  (One stated exception:
``control_residuals`` runs the torch op sequence it replaces for a level whose tensors do not share dense strides, and for host tensors.)"""
import ctypes
import math

import torch

from . import _hip

ED_F32, ED_F16, ED_BF16 = 0, 1, 2
_DTYPE = {torch.float32: ED_F32, torch.float16: ED_F16, torch.bfloat16: ED_BF16}


# Device of the launch being assembled: every ``_dev`` of one wrapper call must name the same ROCm device; ``_stream``
# (always the last argument evaluated) and ``_call`` then use THAT device's current stream and make it the current
# device around the ctypes launch.  Nothing here depends on the process-wide current device (ADVICE r1:
# ``ElasticDiffusion('cuda:1')`` in a process whose current device is 0 must not launch on device 0).
_LAUNCH = {"device": None}


def _stream_of(t):
    """``_stream`` for wrappers whose tensor arguments are not all checked through ``_dev`` (non-default strides)."""
    if _LAUNCH["device"] is None:
        _LAUNCH["device"] = t.device
    return _stream()


def _stream():
    dev = _LAUNCH["device"]
    if dev is None:
        raise RuntimeError("internal: _stream() before any device tensor argument")
    return torch.cuda.current_stream(dev).cuda_stream


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the launch stream (bench.py's roofline leg).
    Disabled by default: zero overhead on the product path."""

    def __init__(self):
        self.enabled = False
        self.events = {}
        self.work = {}

    def start(self):
        self.events, self.work, self.enabled = {}, {}, True

    def stop(self):
        """-> {kernel: (launches, mean_us, total_ms)}; synchronises.  ``self.work[kernel]`` = [flops, bytes] summed over
        the timed launches (ALGORITHMIC work each wrapper declared via ``note_work``)."""
        self.enabled = False
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = (len(ms), 1e3 * sum(ms) / len(ms), sum(ms))
        return out

    def note_work(self, name, flops=0.0, nbytes=0.0):
        if self.enabled and not torch.cuda.is_current_stream_capturing():
            w = self.work.setdefault(name, [0.0, 0.0])
            w[0] += flops
            w[1] += nbytes


TIMER = KernelTimer()


def _call(name, *args):
    fn = getattr(_hip.lib(), name)
    dev, _LAUNCH["device"] = _LAUNCH["device"], None
    if dev is not None and dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):  # a HIP launch runs on the calling thread's current device
            _LAUNCH["device"] = dev
            return _call(name, *args)
    if TIMER.enabled and not torch.cuda.is_current_stream_capturing():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        err = fn(*args)
        b.record()
        TIMER.events.setdefault(name, []).append((a, b))
    else:
        err = fn(*args)
    _hip.check(err, name)


def _reject(msg):
    _LAUNCH["device"] = None  # an abandoned launch must not leak its device into the next one
    raise RuntimeError(msg)


def _dev(t, dtype=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        _reject(f"{name} must be a tensor on the MI355X (got {type(t).__name__}"
                f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}); no CPU fallback")
    if not t.is_contiguous():
        _reject(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        _reject(f"{name} must be {dtype}, got {t.dtype}")
    if _LAUNCH["device"] is None:
        _LAUNCH["device"] = t.device
    elif _LAUNCH["device"] != t.device:
        _reject(f"{name} lives on {t.device} but an earlier argument of this launch is on {_LAUNCH['device']}")
    return t.data_ptr()


def _opt(t, dtype=None, name="tensor"):
    return None if t is None else _dev(t, dtype, name)


def is_nhwc(x):
    """is ``x`` [N,C,H,W] in channels-last memory and NOT NCHW-contiguous as well (a tensor with C = 1 or H = W = 1 is both: every path
    treats it as NCHW)?  The one spelling of the layout test, for the wrappers here and the dispatch rules of models.py."""
    return x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)


def _code(t, name):
    try:
        return _DTYPE[t.dtype]
    except KeyError:
        _reject(f"{name}: unsupported dtype {t.dtype}")


def gather_views(latent, out, win_y0, win_x0, Sh, Sw, off_y=0, off_x=0, frame=None, divisor=1.0):
    """latent f32 [B,C,H,W] -> out [(V*B),C,PH,PW] (row = v*B+b).  See ed_gather_views."""
    B, C, H, W = latent.shape
    V = win_y0.numel()
    rows, C2, PH, PW = out.shape
    assert rows == V * B and C2 == C and win_x0.numel() == V
    assert off_y >= 0 and off_x >= 0 and off_y + Sh <= PH and off_x + Sw <= PW
    if frame is not None:
        assert tuple(frame.shape) == (C, PH, PW)
    _call("ed_gather_views", _dev(latent, torch.float32, "latent"), _dev(out, None, "out"), _code(out, "out"),
          B, C, H, W, _dev(win_y0, torch.int32, "win_y0"), _dev(win_x0, torch.int32, "win_x0"),
          V, Sh, Sw, PH, PW, off_y, off_x, _opt(frame, torch.float32, "frame"),
          float(divisor), _stream())
    return out


def scatter_centres(pred, local, n_col_blocks, row_blk, row_src, col_blk, col_src):
    """pred [(V*B),C,PH,PW] -> local f32 [B,C,H,W], first writer (by value) wins.  See ed_scatter_centres."""
    B, C, H, W = local.shape
    rows, C2, PH, PW = pred.shape
    assert C2 == C and rows % B == 0
    assert row_blk.numel() == H * 2 == row_src.numel() and col_blk.numel() == W * 2 == col_src.numel()
    _call("ed_scatter_centres", _dev(pred, None, "pred"), _code(pred, "pred"), _dev(local, torch.float32, "local"),
          B, C, H, W, PH, PW, n_col_blocks,
          _dev(row_blk, torch.int32), _dev(row_src, torch.int32),
          _dev(col_blk, torch.int32), _dev(col_src, torch.int32), _stream())
    return local


def pick_assemble(latent, idx, src_row, src_col, out, h, w, off_y=0, off_x=0, frame=None, low=None):
    """latent f32 [B,C,H,W], idx u8 [K,h*w] -> out [(K*2*B),C,PH,PW], low f32 [K,B,C,h,w].  See ed_pick_assemble."""
    B, C, H, W = latent.shape
    K = idx.shape[0]
    rows, C2, PH, PW = out.shape
    assert rows == K * 2 * B and C2 == C and idx.shape[1] == h * w
    assert src_row.numel() == 2 * h and src_col.numel() == 2 * w
    assert off_y + h <= PH and off_x + w <= PW
    if frame is not None:
        assert tuple(frame.shape) == (C, PH, PW)
    if low is not None:
        assert tuple(low.shape) == (K, B, C, h, w)
    _call("ed_pick_assemble", _dev(latent, torch.float32, "latent"), _dev(idx, torch.uint8, "idx"),
          _dev(src_row, torch.int32), _dev(src_col, torch.int32),
          _opt(frame, torch.float32, "frame"), _dev(out, None, "out"), _code(out, "out"),
          _opt(low, torch.float32, "low"), K, B, C, H, W, h, w, PH, PW, off_y, off_x,
          _stream())
    return out


def assemble_rows(latent, idx, src_row, src_col, g_rows, h, w, g_off_y, g_off_x, gframe, low, v_rows, win_y0, win_x0, Sh,
                  Sw, v_off_y, v_off_x, vframe):
    """pick_assemble + gather_views in one launch (see ed_assemble_rows): g_rows [(K*2*B),C,gPH,gPW] and v_rows
    [(V*B),C,vPH,vPW] are the two parts of one fused model batch (usually slices of one tensor)."""
    B, C, H, W = latent.shape
    K, V = idx.shape[0], win_y0.numel()
    gr, C2, gPH, gPW = g_rows.shape
    vr, C3, vPH, vPW = v_rows.shape
    assert gr == K * 2 * B and vr == V * B and C2 == C == C3 and idx.shape[1] == h * w and g_rows.dtype == v_rows.dtype
    assert src_row.numel() == 2 * h and src_col.numel() == 2 * w and win_x0.numel() == V
    assert g_off_y + h <= gPH and g_off_x + w <= gPW and v_off_y + Sh <= vPH and v_off_x + Sw <= vPW
    if gframe is not None:
        assert tuple(gframe.shape) == (C, gPH, gPW)
    if vframe is not None:
        assert tuple(vframe.shape) == (C, vPH, vPW)
    if low is not None:
        assert tuple(low.shape) == (K, B, C, h, w)
    _call("ed_assemble_rows", _dev(latent, torch.float32, "latent"), B, C, H, W, _dev(idx, torch.uint8, "idx"),
          _dev(src_row, torch.int32), _dev(src_col, torch.int32), _opt(gframe, torch.float32, "gframe"),
          _dev(g_rows, None, "g_rows"), _opt(low, torch.float32, "low"), K, h, w, gPH, gPW, g_off_y, g_off_x,
          _dev(win_y0, torch.int32), _dev(win_x0, torch.int32), _opt(vframe, torch.float32, "vframe"),
          _dev(v_rows, None, "v_rows"), V, Sh, Sw, vPH, vPW, v_off_y, v_off_x, _code(g_rows, "g_rows"), _stream())


def assemble_rows_x(latent, idx, src_row, src_col, g_rows, h, w, g_off_y, g_off_x, gframe, low, v_rows, win_y0, win_x0, Sh,
                    Sw, v_off_y, v_off_x, vframe, extra, pad_value):
    """``assemble_rows`` for model rows of C + E channels (see ed_assemble_rows_x): ``extra`` f32 [B,E,H,W] goes through the index
    map of each row's latent into channels C.., ``pad_value`` f32 [E] (device) fills them where the latent reads the frame.
    g_rows [(K*2*B),C+E,gPH,gPW], v_rows [(V*B),C+E,vPH,vPW]; ``low`` stays [K,B,C,h,w]."""
    if not isinstance(latent, torch.Tensor) or latent.dim() != 4:
        _reject(f"assemble_rows_x: latent must be an f32 [B,C,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(latent, 'shape', ()))})")
    B, C, H, W = latent.shape
    if not isinstance(extra, torch.Tensor) or extra.dim() != 4 or extra.shape[1] < 1 or \
            (extra.shape[0], extra.shape[2], extra.shape[3]) != (B, H, W):
        _reject(f"assemble_rows_x: extra must be f32 [{B},E,{H},{W}] with E >= 1, got {tuple(getattr(extra, 'shape', ()))}")
    E = int(extra.shape[1])
    if not isinstance(pad_value, torch.Tensor) or tuple(pad_value.shape) != (E,):
        _reject(f"assemble_rows_x: pad_value must be an f32 [{E}] device tensor, got {tuple(getattr(pad_value, 'shape', ()))}")
    K, V = idx.shape[0], win_y0.numel()
    gr, C2, gPH, gPW = g_rows.shape
    vr, C3, vPH, vPW = v_rows.shape
    if not (gr == K * 2 * B and vr == V * B and C2 == C + E == C3 and g_rows.dtype == v_rows.dtype):
        _reject(f"assemble_rows_x: rows must be [{K * 2 * B},{C + E},..] and [{V * B},{C + E},..] of one dtype, got "
                f"{tuple(g_rows.shape)} {g_rows.dtype} / {tuple(v_rows.shape)} {v_rows.dtype}")
    assert idx.shape[1] == h * w and src_row.numel() == 2 * h and src_col.numel() == 2 * w and win_x0.numel() == V
    assert g_off_y + h <= gPH and g_off_x + w <= gPW and v_off_y + Sh <= vPH and v_off_x + Sw <= vPW
    if gframe is not None:
        assert tuple(gframe.shape) == (C, gPH, gPW)
    if vframe is not None:
        assert tuple(vframe.shape) == (C, vPH, vPW)
    if low is not None:
        assert tuple(low.shape) == (K, B, C, h, w)
    _call("ed_assemble_rows_x", _dev(latent, torch.float32, "latent"), B, C, H, W, _dev(idx, torch.uint8, "idx"),
          _dev(src_row, torch.int32), _dev(src_col, torch.int32), _opt(gframe, torch.float32, "gframe"),
          _dev(g_rows, None, "g_rows"), _opt(low, torch.float32, "low"), K, h, w, gPH, gPW, g_off_y, g_off_x,
          _dev(win_y0, torch.int32), _dev(win_x0, torch.int32), _opt(vframe, torch.float32, "vframe"),
          _dev(v_rows, None, "v_rows"), V, Sh, Sw, vPH, vPW, v_off_y, v_off_x, _code(g_rows, "g_rows"),
          _dev(extra, torch.float32, "extra"), E, _dev(pad_value, torch.float32, "pad_value"), _stream())
    # algorithmic bytes: every row element written once, one fp32 read per element, the picks and `low`
    n_rows = (gr * gPH * gPW + vr * vPH * vPW) * (C + E)
    TIMER.note_work("ed_assemble_rows_x", nbytes=float(n_rows * g_rows.element_size() + 4 * (n_rows - gr * gPH * gPW * (C + E) // 2)
                                                       + K * h * w + (0 if low is None else 4 * low.numel())))


MAX_REGION_ROWS = 8  # ED_MAX_REGION_ROWS: the conditional rows of a step, base prompt + at most 7 regions


def assemble_rows_n(latent, idx, src_row, src_col, g_rows, h, w, g_off_y, g_off_x, gframe, low, v_rows, win_y0, win_x0, Sh,
                    Sw, v_off_y, v_off_x, vframe, copies, extra=None, pad_value=None):
    """``assemble_rows`` / ``assemble_rows_x`` with ``copies`` (2..9) rows per resampling step and sample in the place of 2 (see
    ed_assemble_rows_n): g_rows [(K*copies*B),C+E,gPH,gPW]; ``extra`` / ``pad_value`` as in ``assemble_rows_x`` or both None (E = 0)."""
    if not isinstance(latent, torch.Tensor) or latent.dim() != 4:
        _reject(f"assemble_rows_n: latent must be an f32 [B,C,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(latent, 'shape', ()))})")
    B, C, H, W = latent.shape
    if not isinstance(copies, int) or not 2 <= copies <= 1 + MAX_REGION_ROWS:
        _reject(f"assemble_rows_n: copies must be an int in [2, {1 + MAX_REGION_ROWS}], got {copies!r}")
    E = 0
    if (extra is None) != (pad_value is None):
        _reject("assemble_rows_n: extra and pad_value come together")
    if extra is not None:
        if not isinstance(extra, torch.Tensor) or extra.dim() != 4 or extra.shape[1] < 1 or \
                (extra.shape[0], extra.shape[2], extra.shape[3]) != (B, H, W):
            _reject(f"assemble_rows_n: extra must be f32 [{B},E,{H},{W}] with E >= 1, got {tuple(getattr(extra, 'shape', ()))}")
        E = int(extra.shape[1])
        if not isinstance(pad_value, torch.Tensor) or tuple(pad_value.shape) != (E,):
            _reject(f"assemble_rows_n: pad_value must be an f32 [{E}] device tensor, got {tuple(getattr(pad_value, 'shape', ()))}")
    K, V = idx.shape[0], win_y0.numel()
    gr, C2, gPH, gPW = g_rows.shape
    vr, C3, vPH, vPW = v_rows.shape
    if not (gr == K * copies * B and vr == V * B and C2 == C + E == C3 and g_rows.dtype == v_rows.dtype):
        _reject(f"assemble_rows_n: rows must be [{K * copies * B},{C + E},..] and [{V * B},{C + E},..] of one dtype, got "
                f"{tuple(g_rows.shape)} {g_rows.dtype} / {tuple(v_rows.shape)} {v_rows.dtype}")
    assert idx.shape[1] == h * w and src_row.numel() == 2 * h and src_col.numel() == 2 * w and win_x0.numel() == V
    assert g_off_y + h <= gPH and g_off_x + w <= gPW and v_off_y + Sh <= vPH and v_off_x + Sw <= vPW
    if gframe is not None:
        assert tuple(gframe.shape) == (C, gPH, gPW)
    if vframe is not None:
        assert tuple(vframe.shape) == (C, vPH, vPW)
    if low is not None:
        assert tuple(low.shape) == (K, B, C, h, w)
    _call("ed_assemble_rows_n", _dev(latent, torch.float32, "latent"), B, C, H, W, _dev(idx, torch.uint8, "idx"),
          _dev(src_row, torch.int32), _dev(src_col, torch.int32), _opt(gframe, torch.float32, "gframe"),
          _dev(g_rows, None, "g_rows"), _opt(low, torch.float32, "low"), K, h, w, gPH, gPW, g_off_y, g_off_x,
          _dev(win_y0, torch.int32), _dev(win_x0, torch.int32), _opt(vframe, torch.float32, "vframe"),
          _dev(v_rows, None, "v_rows"), V, Sh, Sw, vPH, vPW, v_off_y, v_off_x, _code(g_rows, "g_rows"),
          _opt(extra, torch.float32, "extra"), E, _opt(pad_value, torch.float32, "pad_value"), copies, _stream())
    # algorithmic bytes: every row element written once, one fp32 read per picked vector and view element, the picks and `low`
    n_g, n_v = gr * gPH * gPW * (C + E), vr * vPH * vPW * (C + E)
    TIMER.note_work("ed_assemble_rows_n", nbytes=float((n_g + n_v) * g_rows.element_size() + 4 * (n_g // copies + n_v)
                                                       + K * h * w + (0 if low is None else 4 * low.numel())))


IP_MASK_LEVELS = 4        # ed_ip_mask_rows: levels 0..3 of the 2 x 2-mean pyramid
IP_MASK_MAX_ADAPTERS = 4


def ip_mask_layout(PH, PW):
    """[(offset, (PH >> L) * (PW >> L)) for L in 0..3] inside one row's [S] floats of ``ip_mask_rows``' buffer, and S"""
    sizes = [(PH >> L) * (PW >> L) for L in range(IP_MASK_LEVELS)]
    return [(sum(sizes[:L]), sizes[L]) for L in range(IP_MASK_LEVELS)], sum(sizes)


def ip_mask_rows(masks, idx, src_row, src_col, h, w, g_off_y, g_off_x, win_y0, win_x0, Sh, Sw, v_off_y, v_off_x, PH, PW, copies,
                 out=None):
    """IP-Adapter attention masks of every row of one fused model batch (see ed_ip_mask_rows): ``masks`` f32
    [B,A,H,W] on the device, the gather arguments of ``assemble_rows_n`` (``idx`` [K,h*w] / ``win_y0`` [V] may be None for a batch
    without global / view rows) -> f32 [(K*copies+V)*B, A, S]: per row and adapter the level-0 frame [PH,PW] followed by its
    2 x 2-mean levels 1..3 (``ip_mask_layout``).  One launch."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 4 or not masks.is_cuda or masks.dtype != torch.float32:
        _reject(f"ip_mask_rows: masks must be an f32 [B,A,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(masks, 'shape', ()))} {getattr(masks, 'dtype', None)})")
    B, A, H, W = masks.shape
    if not 1 <= A <= IP_MASK_MAX_ADAPTERS:
        _reject(f"ip_mask_rows: 1 to {IP_MASK_MAX_ADAPTERS} adapters, got {A}")
    if not isinstance(copies, int) or not 2 <= copies <= 1 + MAX_REGION_ROWS:
        _reject(f"ip_mask_rows: copies must be an int in [2, {1 + MAX_REGION_ROWS}], got {copies!r}")
    PH, PW = int(PH), int(PW)
    if PH < 8 or PW < 8 or PH % 8 or PW % 8:
        _reject(f"ip_mask_rows: the padded row size must be a multiple of 8 on both axes, got {PH} x {PW}")
    K = 0 if idx is None else idx.shape[0]
    V = 0 if win_y0 is None else win_y0.numel()
    if K and (idx.shape[1] != h * w or src_row.numel() != 2 * h or src_col.numel() != 2 * w):
        _reject(f"ip_mask_rows: idx [K,{h * w}], src_row [{2 * h}] and src_col [{2 * w}] expected, got {tuple(idx.shape)}, "
                f"{src_row.numel()}, {src_col.numel()}")
    if V and win_x0.numel() != V:
        _reject(f"ip_mask_rows: win_y0 and win_x0 must hold one entry per view, got {V} and {win_x0.numel()}")
    if (K and (g_off_y < 0 or g_off_x < 0 or g_off_y + h > PH or g_off_x + w > PW)) or \
            (V and (v_off_y < 0 or v_off_x < 0 or v_off_y + Sh > PH or v_off_x + Sw > PW)):
        _reject(f"ip_mask_rows: the picked frame ({h} x {w} at {g_off_y}, {g_off_x}) / the window ({Sh} x {Sw} at {v_off_y}, "
                f"{v_off_x}) does not fit a {PH} x {PW} row")
    S = ip_mask_layout(PH, PW)[1]
    rows = (K * copies + V) * B
    if out is None:
        out = torch.empty(rows, A, S, device=masks.device, dtype=torch.float32)
    elif tuple(out.shape) != (rows, A, S) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != masks.device:
        _reject(f"ip_mask_rows: out must be a contiguous f32 [{rows},{A},{S}] tensor beside masks, got {tuple(out.shape)} {out.dtype}")
    if rows == 0:
        return out
    _call("ed_ip_mask_rows", _dev(masks, torch.float32, "masks"), B, A, H, W, _opt(idx if K else None, torch.uint8, "idx"),
          _opt(src_row if K else None, torch.int32, "src_row"), _opt(src_col if K else None, torch.int32, "src_col"), K,
          h if K else 0, w if K else 0, g_off_y if K else 0, g_off_x if K else 0, _opt(win_y0 if V else None, torch.int32, "win_y0"),
          _opt(win_x0 if V else None, torch.int32, "win_x0"), V, Sh if V else 0, Sw if V else 0, v_off_y if V else 0,
          v_off_x if V else 0, PH, PW, copies, _dev(out, torch.float32, "out"), _stream())
    # algorithmic bytes: every output float once, one fp32 read per gathered level-0 pixel, the picks
    TIMER.note_work("ed_ip_mask_rows", nbytes=float(4 * out.numel() + 4 * (K + V) * B * A * PH * PW + K * h * w))
    return out


def _region_w(region_w, H, W, what, outputs=()):
    """``region_w`` f32 [P,H,W] on the device, 1 <= P <= 8, sharing no memory with the launch's outputs -> (pointer, P)"""
    if not isinstance(region_w, torch.Tensor) or region_w.dim() != 3 or tuple(region_w.shape[1:]) != (H, W) or \
            not 1 <= region_w.shape[0] <= MAX_REGION_ROWS:
        _reject(f"{what}: region_w must be an f32 [P,{H},{W}] tensor with 1 <= P <= {MAX_REGION_ROWS}, got "
                f"{tuple(getattr(region_w, 'shape', ()))}")
    lo, hi = region_w.data_ptr(), region_w.data_ptr() + 4 * region_w.numel()
    for t_ in outputs:
        if isinstance(t_, torch.Tensor) and t_.data_ptr() < hi and lo < t_.data_ptr() + t_.element_size() * t_.numel():
            _reject(f"{what}: region_w overlaps an output of the launch")
    return _dev(region_w, torch.float32, "region_w"), int(region_w.shape[0])


def region_weights(masks, weights, out=None):
    """masks u8 [n,Hl,Wl] (255 = inside the region), ``weights`` n floats > 0 -> f32 [n + 1,Hl,Wl]: the per-pixel weights of the
    base prompt (plane 0) and the n regions, summing to 1 (see ed_region_weights).  1 <= n <= 7.  One launch."""
    import ctypes
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or not 1 <= masks.shape[0] <= MAX_REGION_ROWS - 1:
        _reject(f"region_weights: masks must be a u8 [n,Hl,Wl] tensor on the MI355X with 1 <= n <= {MAX_REGION_ROWS - 1}; no CPU "
                f"fallback (got {tuple(getattr(masks, 'shape', ()))})")
    n, Hl, Wl = masks.shape
    try:
        wts = [float(v) for v in weights]
    except (TypeError, ValueError):
        _reject(f"region_weights: weights must be {n} floats, got {weights!r}")
    if len(wts) != n or not all(0.0 < v < float("inf") for v in wts):
        _reject(f"region_weights: weights must be {n} finite floats > 0, got {weights!r}")
    if out is None:
        out = torch.empty(n + 1, Hl, Wl, dtype=torch.float32, device=masks.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n + 1, Hl, Wl):
        _reject(f"region_weights: out must be f32 [{n + 1},{Hl},{Wl}], got {tuple(getattr(out, 'shape', ()))}")
    _call("ed_region_weights", _dev(masks, torch.uint8, "masks"), (ctypes.c_float * n)(*wts), n, Hl * Wl,
          _dev(out, torch.float32, "out"), _stream())
    TIMER.note_work("ed_region_weights", nbytes=float(n * Hl * Wl + 4 * (n + 1) * Hl * Wl))
    return out


def region_blend(dirs, region_w, out=None):
    """dirs f32 [P,B,C,H,W] (the P per-region class directions), region_w f32 [P,H,W] -> f32 [B,C,H,W], the weighted sum over p with
    the skip rule and order of the fused regional epilogue (see ed_region_blend): the un-fused path's last step."""
    if not isinstance(dirs, torch.Tensor) or dirs.dim() != 5:
        _reject(f"region_blend: dirs must be an f32 [P,B,C,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(dirs, 'shape', ()))})")
    P, B, C, H, W = dirs.shape
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=dirs.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, C, H, W):
        _reject(f"region_blend: out must be f32 [{B},{C},{H},{W}], got {tuple(getattr(out, 'shape', ()))}")
    lo, hi = out.data_ptr(), out.data_ptr() + 4 * out.numel()
    if dirs.data_ptr() < hi and lo < dirs.data_ptr() + 4 * dirs.numel():
        _reject("region_blend: dirs overlaps out")
    wp, P2 = _region_w(region_w, H, W, "region_blend", (out,))
    if P2 != P:
        _reject(f"region_blend: dirs holds {P} directions, region_w {P2} planes")
    _call("ed_region_blend", _dev(dirs, torch.float32, "dirs"), wp, _dev(out, torch.float32, "out"), P, B * C, H * W, _stream())
    TIMER.note_work("ed_region_blend", nbytes=4.0 * (dirs.numel() + region_w.numel() + out.numel()))
    return out


PREDICTION_TYPES = {"epsilon": 0, "v_prediction": 1}  # ED_PRED_EPSILON / ED_PRED_V


def _pred_code(prediction_type):
    if prediction_type not in PREDICTION_TYPES:
        _reject(f"prediction_type must be one of {sorted(PREDICTION_TYPES)}, got {prediction_type!r}")
    return PREDICTION_TYPES[prediction_type]


def rescale_coefficients(guidance_rescale):
    """(gr, omgr) = (float32(guidance_rescale), float32(1 - guidance_rescale)), the two host-side scalars of the rescale
    m <- gr * (m * ratio) + omgr * m; ``guidance_rescale`` outside [0, 1] raises ValueError."""
    import numpy as np
    gr = float(guidance_rescale)
    if not 0.0 <= gr <= 1.0:          # also refuses NaN
        raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
    return float(np.float32(gr)), float(np.float32(1.0 - gr))


def _ratio_ptr(ratio, B, name):
    if not isinstance(ratio, torch.Tensor) or tuple(ratio.shape) != (B,):
        _reject(f"{name} must be an f32 [{B}] tensor (one ratio per sample), got {tuple(getattr(ratio, 'shape', ()))}")
    return _dev(ratio, torch.float32, name)


def _multistep(multistep, prev, x0, what):
    """``multistep`` = (c_x, b, half_b, r_inv, x0_hist): the four host scalars of DPMSolverSchedule.multistep_coefficients and the
    previous timestep's x0 (f32, the outputs' shape), or None in its place for the first-order form -> (floats, x0_hist).
    A history that shares memory with ``prev`` or ``x0`` is refused: they are written while it is being read."""
    try:
        c_x, b, half_b, r_inv, x0_hist = multistep
        scalars = tuple(float(v) for v in (c_x, b, half_b, r_inv))
    except (TypeError, ValueError):
        _reject(f"{what}: multistep must be (c_x, b, half_b, r_inv, x0_hist or None), got {multistep!r}")
    if x0_hist is not None:
        if not isinstance(x0_hist, torch.Tensor) or x0_hist.numel() != x0.numel():
            _reject(f"{what}: x0_hist must be an f32 tensor of {x0.numel()} elements")
        lo, hi = x0_hist.data_ptr(), x0_hist.data_ptr() + 4 * x0_hist.numel()
        for t_, name in ((prev, "prev"), (x0, "x0")):
            if isinstance(t_, torch.Tensor) and t_.data_ptr() < hi and lo < t_.data_ptr() + 4 * t_.numel():
                _reject(f"{what}: x0_hist overlaps {name} (the history is read while the outputs are written)")
    return scalars, x0_hist


def _noise(noise, like, outputs, what):
    """``noise`` = (c_n, tensor): the scalar of the stochastic samplers' noise term (``noise_coefficient`` of the schedule) and the
    host's draw (f32, ``like``'s shape) -> (c_n as a float, tensor).  A non-finite c_n, and a tensor that shares memory with an output
    of the launch (they are written while it is being read), are refused."""
    try:
        c_n, tensor = noise
        c_n = float(c_n)
    except (TypeError, ValueError):
        _reject(f"{what}: noise must be (c_n, tensor), got {noise!r}")
    if not math.isfinite(c_n):
        _reject(f"{what}: the noise coefficient must be finite, got {c_n!r}")
    if not isinstance(tensor, torch.Tensor) or tuple(tensor.shape) != tuple(like.shape):
        _reject(f"{what}: the noise must be an f32 tensor of shape {tuple(like.shape)}, got {tuple(getattr(tensor, 'shape', ()))}")
    lo, hi = tensor.data_ptr(), tensor.data_ptr() + 4 * tensor.numel()
    for t_ in outputs:
        if isinstance(t_, torch.Tensor) and t_.data_ptr() < hi and lo < t_.data_ptr() + 4 * t_.numel():
            _reject(f"{what}: the noise overlaps an output of the launch")
    return c_n, tensor


def guidance_moments_workspace(B, n_full, n_low=0, device=None):
    """The partials buffer of guidance_moments / phase_moments for B samples of ``n_full`` elements (+ the
    reduced-resolution pair of ``n_low`` elements): an f64 tensor, allocate once and reuse (launches on one stream)."""
    nbytes = _hip.lib().ed_guidance_moments_workspace(int(B), int(n_full), int(n_low))
    return torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)


def _workspace(ws, B, n_full, n_low):
    need = _hip.lib().ed_guidance_moments_workspace(int(B), int(n_full), int(n_low))
    if not isinstance(ws, torch.Tensor) or ws.numel() * ws.element_size() < need:
        _reject(f"workspace must hold {need} bytes (guidance_moments_workspace({B}, {n_full}, {n_low}))")
    return _dev(ws, None, "workspace")


def guidance_moments(local, direction, g, ratio, workspace, text=None):
    """ratio f32 [B] <- std(local + direction) / std(local + g * direction) per sample (unbiased, over everything but
    dim 0) of two f32 tensors [B, ...]: the guidance-rescale factor of the reference's rescale_noise_cfg, computed on the
    device (see ed_guidance_moments).  ``text`` (optional, same shape): the numerator's tensor given as is (plain CFG: the
    conditional prediction) instead of local + direction.  workspace = guidance_moments_workspace(B, n)."""
    B = ratio.numel()
    if B == 0 or local.numel() % B or local.shape[0] != B or local.shape != direction.shape:
        _reject(f"guidance_moments: local / direction must be equal-shaped [B={B}, ...] tensors, got "
                f"{tuple(local.shape)} / {tuple(direction.shape)}")
    if text is not None and text.shape != local.shape:
        _reject(f"guidance_moments: text must have local's shape {tuple(local.shape)}, got {tuple(text.shape)}")
    n = local.numel() // B
    _call("ed_guidance_moments", _dev(local, torch.float32, "local"), _dev(direction, torch.float32, "direction"),
          _opt(text, torch.float32, "text"), float(g), B, n, _dev(ratio, torch.float32, "ratio"), _workspace(workspace, B, n, 0), _stream())
    TIMER.note_work("ed_guidance_moments", nbytes=(8.0 if text is None else 12.0) * B * n)
    return ratio


def phase_moments(g_out, v_out, shape, stamp, pick_tables, view_tables, n_col_blocks, g_off, K, h, w, g, ratio, workspace,
                  ratio_low=None, region_w=None):
    """The ratios guidance_moments would give on the ``direction`` / ``local`` (and, with ``ratio_low``, the
    ``uncond_last`` / ``low_dir``) by-products of phase_epilogue, reduced straight from the model output rows (see
    ed_phase_moments): same arguments as phase_epilogue, ``shape`` = (B, C, H, W) of the latent.
    workspace = guidance_moments_workspace(B, C*H*W, C*h*w if ratio_low is given else 0).  ``region_w`` (f32 [P,H,W], regional
    prompts): g_out holds 1 + P rows per step and sample and the direction is their weighted sum (ed_phase_moments_rg)."""
    B, C, H, W = shape
    gr, C2, gPH, gPW = g_out.shape
    vr, C3, vPH, vPW = v_out.shape
    copies = 2 if region_w is None else 1 + int(getattr(region_w, "shape", (1,))[0])
    assert gr == K * copies * B and C2 == C == C3 and vr % B == 0 and g_out.dtype == v_out.dtype
    assert tuple(stamp.shape) == (h * w, 4)
    inv_row, inv_col, up_row, up_col, down_row, down_col = pick_tables
    assert inv_row.numel() == 2 * H and inv_col.numel() == 2 * W and up_row.numel() == H and up_col.numel() == W
    assert down_row.numel() == h and down_col.numel() == w
    row_blk, row_src, col_blk, col_src = view_tables
    assert row_blk.numel() == H * 2 == row_src.numel() and col_blk.numel() == W * 2 == col_src.numel()
    for t_, name in ((ratio, "ratio"), (ratio_low, "ratio_low")):
        if t_ is not None and tuple(t_.shape) != (B,):
            _reject(f"phase_moments: {name} must be f32 [{B}], got {tuple(t_.shape)}")
    n_low = C * h * w if ratio_low is not None else 0
    if region_w is not None:
        wp, P = _region_w(region_w, H, W, "phase_moments", (ratio, ratio_low, workspace))
        _call("ed_phase_moments_rg", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
              _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
              *(_dev(t_, torch.int32) for t_ in view_tables), _dev(ratio, torch.float32, "ratio"),
              _opt(ratio_low, torch.float32, "ratio_low"), _workspace(workspace, B, C * H * W, n_low),
              K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), wp, P, _stream())
        TIMER.note_work("ed_phase_moments_rg", nbytes=(2.0 + P) * g_out.element_size() * B * (C * H * W + n_low))
        return ratio, ratio_low
    _call("ed_phase_moments", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
          _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
          *(_dev(t_, torch.int32) for t_ in view_tables), _dev(ratio, torch.float32, "ratio"),
          _opt(ratio_low, torch.float32, "ratio_low"), _workspace(workspace, B, C * H * W, n_low),
          K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), _stream())
    # the rows behind every output element: cond + uncond of its step and (at most a few) view centres
    TIMER.note_work("ed_phase_moments", nbytes=3.0 * g_out.element_size() * B * (C * H * W + n_low))
    return ratio, ratio_low


def phase_epilogue(g_out, v_out, x, stamp, pick_tables, view_tables, n_col_blocks, g_off, K, h, w, g, coef, prev, x0,
                   low_dir=None, uncond_last=None, direction=None, local=None, x_next=None, low_latent=None,
                   rrg_norm=0.0, rrg_weight=0.0, prediction_type="epsilon", ratio=None, ratio_low=None,
                   guidance_rescale=0.0, multistep=None, region_w=None, noise=None):
    """unpad_direction + fill_directions + scatter_centres + cfg_ddim_step (+ rrg_update when ``x_next`` is given) in
    one launch (see ed_phase_epilogue / ed_phase_epilogue_pt).  pick_tables = (inv_row, inv_col, up_row, up_col,
    down_row, down_col); view_tables = (row_blk, row_src, col_blk, col_src); coef = DDIMSchedule.step_coefficients(t);
    prediction_type = the scheduler's ("epsilon" or "v_prediction").  ``ratio`` (f32 [B] from phase_moments, with
    ``ratio_low`` when ``x_next`` is given) applies the guidance rescale ``guidance_rescale`` (ed_phase_epilogue_gr);
    None is the plain launch.  ``multistep`` = (c_x, b, half_b, r_inv, x0_hist or None): the DPM-Solver++(2M) update in the
    DDIM one's place (ed_phase_epilogue_ms; only coef[:2] are then used); None launches what it always launched.
    ``region_w`` (f32 [P,H,W] from ``region_weights``; regional prompts): g_out holds 1 + P rows per step and
    sample, [(K*(1+P)*B),C,gPH,gPW], and the class direction of a pixel is the weighted sum of the P directions cond_p - uncond
    (ed_phase_epilogue_rg, one launch with every other keyword as above); None launches what it always launched.
    ``noise`` = (c_n, f32 [B,C,H,W]): the stochastic samplers' term, prev += c_n * noise, before the fused RRG output is formed
    (ed_phase_epilogue_sde; with ``multistep`` the multistep form, otherwise the DDIM form with coef[3] =
    sd_eta); at c_n == 0 the deterministic kernels run and the tensor is not read.  None launches what it always launched."""
    pt = _pred_code(prediction_type)
    B, C, H, W = x.shape
    gr, C2, gPH, gPW = g_out.shape
    vr, C3, vPH, vPW = v_out.shape
    copies = 2 if region_w is None else 1 + int(getattr(region_w, "shape", (1,))[0])
    assert gr == K * copies * B and C2 == C == C3 and vr % B == 0 and g_out.dtype == v_out.dtype
    assert tuple(stamp.shape) == (h * w, 4) and tuple(prev.shape) == tuple(x.shape) == tuple(x0.shape)
    inv_row, inv_col, up_row, up_col, down_row, down_col = pick_tables
    assert inv_row.numel() == 2 * H and inv_col.numel() == 2 * W and up_row.numel() == H and up_col.numel() == W
    assert down_row.numel() == h and down_col.numel() == w
    row_blk, row_src, col_blk, col_src = view_tables
    assert row_blk.numel() == H * 2 == row_src.numel() and col_blk.numel() == W * 2 == col_src.numel()
    for t_, shp in ((low_dir, (B, C, h, w)), (uncond_last, (B, C, h, w)), (low_latent, (B, C, h, w)),
                    (direction, (B, C, H, W)), (local, (B, C, H, W)), (x_next, (B, C, H, W))):
        assert t_ is None or tuple(t_.shape) == shp
    if x_next is not None and low_latent is None:
        _reject("phase_epilogue: x_next (fused RRG) needs low_latent")
    f32 = torch.float32
    if ratio is None and (ratio_low is not None or float(guidance_rescale) != 0.0):
        _reject("phase_epilogue: guidance_rescale / ratio_low need ratio (phase_moments)")
    if noise is not None:
        if region_w is not None:
            _reject("phase_epilogue: the regional epilogue has no noise variant (regions with a stochastic sampler)")
        c_n, nz = _noise(noise, x, (prev, x0, x_next, low_dir, uncond_last, direction, local), "phase_epilogue")
        ms, x0_hist = (tuple(float(c) for c in coef[2:4]) + (0.0, 0.0), None)
        if multistep is not None:
            ms, x0_hist = _multistep(multistep, prev, x0, "phase_epilogue")
            if x0_hist is not None and tuple(x0_hist.shape) != tuple(x0.shape):
                _reject(f"phase_epilogue: x0_hist must have x0's shape {tuple(x0.shape)}, got {tuple(x0_hist.shape)}")
        gr_f, omgr_f = 0.0, 0.0
        if ratio is not None:
            if x_next is not None and ratio_low is None:
                _reject("phase_epilogue: the fused RRG term with a rescale needs ratio_low")
            if ratio_low is not None and tuple(ratio_low.shape) != (B,):
                _reject(f"ratio_low must be f32 [{B}], got {tuple(ratio_low.shape)}")
            gr_f, omgr_f = rescale_coefficients(guidance_rescale)
        _call("ed_phase_epilogue_sde", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
              _dev(x, f32, "x"), _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
              *(_dev(t_, torch.int32) for t_ in view_tables), _opt(low_latent, f32, "low_latent"), _dev(prev, f32, "prev"),
              _dev(x0, f32, "x0"), _opt(x_next, f32, "x_next"), _opt(low_dir, f32, "low_dir"),
              _opt(uncond_last, f32, "uncond_last"), _opt(direction, f32, "direction"), _opt(local, f32, "local"),
              K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), float(coef[0]), float(coef[1]),
              *ms, float(rrg_norm), float(rrg_weight), pt, None if ratio is None else _ratio_ptr(ratio, B, "ratio"),
              _opt(ratio_low, f32, "ratio_low"), gr_f, omgr_f, _opt(x0_hist, f32, "x0_hist"), int(multistep is not None), c_n,
              _dev(nz, f32, "noise"), _stream())
        TIMER.note_work("ed_phase_epilogue_sde", nbytes=4.0 * x.numel())  # the read the variant adds to the epilogue's
        return prev, x0
    if region_w is not None:
        ms, x0_hist = (tuple(float(c) for c in coef[2:4]) + (0.0, 0.0), None)
        if multistep is not None:
            ms, x0_hist = _multistep(multistep, prev, x0, "phase_epilogue")
            if x0_hist is not None and tuple(x0_hist.shape) != tuple(x0.shape):
                _reject(f"phase_epilogue: x0_hist must have x0's shape {tuple(x0.shape)}, got {tuple(x0_hist.shape)}")
        gr_f, omgr_f = 0.0, 0.0
        if ratio is not None:
            if x_next is not None and ratio_low is None:
                _reject("phase_epilogue: the fused RRG term with a rescale needs ratio_low")
            if ratio_low is not None and tuple(ratio_low.shape) != (B,):
                _reject(f"ratio_low must be f32 [{B}], got {tuple(ratio_low.shape)}")
            gr_f, omgr_f = rescale_coefficients(guidance_rescale)
        wp, P = _region_w(region_w, H, W, "phase_epilogue", (prev, x0, x_next, low_dir, uncond_last, direction, local))
        _call("ed_phase_epilogue_rg", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
              _dev(x, f32, "x"), _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
              *(_dev(t_, torch.int32) for t_ in view_tables), _opt(low_latent, f32, "low_latent"), _dev(prev, f32, "prev"),
              _dev(x0, f32, "x0"), _opt(x_next, f32, "x_next"), _opt(low_dir, f32, "low_dir"),
              _opt(uncond_last, f32, "uncond_last"), _opt(direction, f32, "direction"), _opt(local, f32, "local"),
              K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), float(coef[0]), float(coef[1]),
              *ms, float(rrg_norm), float(rrg_weight), pt, None if ratio is None else _ratio_ptr(ratio, B, "ratio"),
              _opt(ratio_low, f32, "ratio_low"), gr_f, omgr_f, _opt(x0_hist, f32, "x0_hist"), int(multistep is not None), wp, P,
              _stream())
        TIMER.note_work("ed_phase_epilogue_rg", nbytes=float(g_out.element_size() * (2 + P) * x.numel() + 4 * 3 * x.numel()))
        return prev, x0
    if multistep is not None:
        ms, x0_hist = _multistep(multistep, prev, x0, "phase_epilogue")
        if x0_hist is not None and tuple(x0_hist.shape) != tuple(x0.shape):
            _reject(f"phase_epilogue: x0_hist must have x0's shape {tuple(x0.shape)}, got {tuple(x0_hist.shape)}")
        gr_f, omgr_f = 0.0, 0.0
        if ratio is not None:
            if x_next is not None and ratio_low is None:
                _reject("phase_epilogue: the fused RRG term with a rescale needs ratio_low")
            if ratio_low is not None and tuple(ratio_low.shape) != (B,):
                _reject(f"ratio_low must be f32 [{B}], got {tuple(ratio_low.shape)}")
            gr_f, omgr_f = rescale_coefficients(guidance_rescale)
        _call("ed_phase_epilogue_ms", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
              _dev(x, f32, "x"), _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
              *(_dev(t_, torch.int32) for t_ in view_tables), _opt(low_latent, f32, "low_latent"), _dev(prev, f32, "prev"),
              _dev(x0, f32, "x0"), _opt(x_next, f32, "x_next"), _opt(low_dir, f32, "low_dir"),
              _opt(uncond_last, f32, "uncond_last"), _opt(direction, f32, "direction"), _opt(local, f32, "local"),
              K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), float(coef[0]), float(coef[1]),
              *ms, float(rrg_norm), float(rrg_weight), pt, None if ratio is None else _ratio_ptr(ratio, B, "ratio"),
              _opt(ratio_low, f32, "ratio_low"), gr_f, omgr_f, _opt(x0_hist, f32, "x0_hist"), _stream())
        return prev, x0
    if ratio is not None:
        if x_next is not None and ratio_low is None:
            _reject("phase_epilogue: the fused RRG term with a rescale needs ratio_low")
        if ratio_low is not None and tuple(ratio_low.shape) != (B,):
            _reject(f"ratio_low must be f32 [{B}], got {tuple(ratio_low.shape)}")
        gr_f, omgr_f = rescale_coefficients(guidance_rescale)  # ValueError before any argument of the launch is taken
        _call("ed_phase_epilogue_gr", _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
              _dev(x, f32, "x"), _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
              *(_dev(t_, torch.int32) for t_ in view_tables), _opt(low_latent, f32, "low_latent"), _dev(prev, f32, "prev"),
              _dev(x0, f32, "x0"), _opt(x_next, f32, "x_next"), _opt(low_dir, f32, "low_dir"),
              _opt(uncond_last, f32, "uncond_last"), _opt(direction, f32, "direction"), _opt(local, f32, "local"),
              K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), *(float(c) for c in coef),
              float(rrg_norm), float(rrg_weight), pt, _ratio_ptr(ratio, B, "ratio"), _opt(ratio_low, f32, "ratio_low"), gr_f, omgr_f, _stream())
        return prev, x0
    _call("ed_phase_epilogue_pt" if pt else "ed_phase_epilogue",
          _dev(g_out, None, "g_out"), _dev(v_out, None, "v_out"), _code(g_out, "g_out"),
          _dev(x, f32, "x"), _dev(stamp, torch.int8, "stamp"), *(_dev(t_, torch.int32) for t_ in pick_tables),
          *(_dev(t_, torch.int32) for t_ in view_tables), _opt(low_latent, f32, "low_latent"), _dev(prev, f32, "prev"),
          _dev(x0, f32, "x0"), _opt(x_next, f32, "x_next"), _opt(low_dir, f32, "low_dir"),
          _opt(uncond_last, f32, "uncond_last"), _opt(direction, f32, "direction"), _opt(local, f32, "local"),
          K, B, C, H, W, h, w, gPH, gPW, g_off[0], g_off[1], vPH, vPW, n_col_blocks, float(g), *(float(c) for c in coef),
          float(rrg_norm), float(rrg_weight), *((pt,) if pt else ()), _stream())
    return prev, x0


def unpad_direction(unet_out, dirs, uncond_last, off_y=0, off_x=0):
    """unet_out [(K*2*B),C,PH,PW] -> dirs f32 [K,B,C,h,w] (= cond - uncond), uncond_last f32 [B,C,h,w]."""
    K, B, C, h, w = dirs.shape
    rows, C2, PH, PW = unet_out.shape
    assert rows == K * 2 * B and C2 == C
    if uncond_last is not None:
        assert tuple(uncond_last.shape) == (B, C, h, w)
    _call("ed_unpad_direction", _dev(unet_out, None, "unet_out"), _code(unet_out, "unet_out"),
          _dev(dirs, torch.float32, "dirs"), _opt(uncond_last, torch.float32, "uncond_last"),
          K, B, C, h, w, PH, PW, off_y, off_x, _stream())
    return dirs


def fill_directions(dirs, stamp, inv_row, inv_col, up_row, up_col, down_row, down_col, target, low_dir=None):
    """dirs f32 [K,B,C,h,w] + stamp i8 [h*w,4] -> target f32 [B,C,H,W] (+ low_dir f32 [B,C,h,w])."""
    K, B, C, h, w = dirs.shape
    B2, C2, H, W = target.shape
    assert (B2, C2) == (B, C) and tuple(stamp.shape) == (h * w, 4)
    assert inv_row.numel() == 2 * H and inv_col.numel() == 2 * W and up_row.numel() == H and up_col.numel() == W
    assert down_row.numel() == h and down_col.numel() == w
    _call("ed_fill_directions", _dev(dirs, torch.float32, "dirs"), _dev(stamp, torch.int8, "stamp"),
          _dev(inv_row, torch.int32), _dev(inv_col, torch.int32),
          _dev(up_row, torch.int32), _dev(up_col, torch.int32),
          _dev(down_row, torch.int32), _dev(down_col, torch.int32),
          _dev(target, torch.float32, "target"), _opt(low_dir, torch.float32, "low_dir"),
          K, B, C, H, W, h, w, _stream())
    return target


def cfg_ddim_step(local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_1m_alpha_prev,
                  prediction_type="epsilon", ratio=None, guidance_rescale=0.0, multistep=None, noise=None):
    """``ratio`` (f32 [B] from guidance_moments; the buffers are then B equal samples) applies the guidance rescale to
    local + g * direction before the update (ed_cfg_ddim_step_gr); None is the plain launch.  ``multistep`` = (c_x, b, half_b,
    r_inv, x0_hist or None): the DPM-Solver++(2M) update in the DDIM one's place (ed_cfg_ddim_step_ms; sqrt_alpha_prev and
    sqrt_1m_alpha_prev are then unused); None launches what it always launched.  ``noise`` = (c_n, f32 tensor of x's shape): the
    stochastic samplers' term prev += c_n * noise (ed_cfg_ddim_step_sde; the multistep form with
    ``multistep``, otherwise the DDIM form with sqrt_1m_alpha_prev = sd_eta); at c_n == 0 the deterministic kernels run and the
    tensor is not read.  None launches what it always launched."""
    pt = _pred_code(prediction_type)
    n = x.numel()
    for t in (local, direction, prev, x0):
        assert t.numel() == n
    if ratio is None and float(guidance_rescale) != 0.0:
        _reject("cfg_ddim_step: guidance_rescale needs ratio (guidance_moments)")
    if noise is not None:
        c_n, nz = _noise(noise, x, (prev, x0), "cfg_ddim_step")
        ms, x0_hist = (float(sqrt_alpha_prev), float(sqrt_1m_alpha_prev), 0.0, 0.0), None
        if multistep is not None:
            ms, x0_hist = _multistep(multistep, prev, x0, "cfg_ddim_step")
        B, gr_f, omgr_f = 0, 0.0, 0.0
        if ratio is not None:
            B = ratio.numel()
            if B == 0 or n % B:
                _reject(f"cfg_ddim_step: {n} elements are not {B} equal samples")
            gr_f, omgr_f = rescale_coefficients(guidance_rescale)
        _call("ed_cfg_ddim_step_sde",
              _dev(local, torch.float32), _dev(direction, torch.float32), _dev(x, torch.float32),
              _dev(prev, torch.float32), _dev(x0, torch.float32), float(g), float(sqrt_beta_t), float(sqrt_alpha_t), *ms, n, pt,
              None if ratio is None else _ratio_ptr(ratio, B, "ratio"), gr_f, omgr_f, B,
              _opt(x0_hist, torch.float32, "x0_hist"), int(multistep is not None), c_n, _dev(nz, torch.float32, "noise"), _stream())
        TIMER.note_work("ed_cfg_ddim_step_sde", nbytes=4.0 * n)  # the read the variant adds to the step's
        return prev, x0
    if multistep is not None:
        ms, x0_hist = _multistep(multistep, prev, x0, "cfg_ddim_step")
        B, gr_f, omgr_f = 0, 0.0, 0.0
        if ratio is not None:
            B = ratio.numel()
            if B == 0 or n % B:
                _reject(f"cfg_ddim_step: {n} elements are not {B} equal samples")
            gr_f, omgr_f = rescale_coefficients(guidance_rescale)
        _call("ed_cfg_ddim_step_ms",
              _dev(local, torch.float32), _dev(direction, torch.float32), _dev(x, torch.float32),
              _dev(prev, torch.float32), _dev(x0, torch.float32), float(g), float(sqrt_beta_t), float(sqrt_alpha_t), *ms, n, pt,
              None if ratio is None else _ratio_ptr(ratio, B, "ratio"), gr_f, omgr_f, B,
              _opt(x0_hist, torch.float32, "x0_hist"), _stream())
        return prev, x0
    if ratio is not None:
        B = ratio.numel()
        if B == 0 or n % B:
            _reject(f"cfg_ddim_step: {n} elements are not {B} equal samples")
        gr_f, omgr_f = rescale_coefficients(guidance_rescale)  # ValueError before any argument of the launch is taken
        _call("ed_cfg_ddim_step_gr",
              _dev(local, torch.float32), _dev(direction, torch.float32), _dev(x, torch.float32),
              _dev(prev, torch.float32), _dev(x0, torch.float32), float(g), float(sqrt_beta_t),
              float(sqrt_alpha_t), float(sqrt_alpha_prev), float(sqrt_1m_alpha_prev), n, pt,
              _ratio_ptr(ratio, B, "ratio"), gr_f, omgr_f, B, _stream())
        return prev, x0
    _call("ed_cfg_ddim_step_pt" if pt else "ed_cfg_ddim_step",
          _dev(local, torch.float32), _dev(direction, torch.float32), _dev(x, torch.float32),
          _dev(prev, torch.float32), _dev(x0, torch.float32), float(g), float(sqrt_beta_t),
          float(sqrt_alpha_t), float(sqrt_alpha_prev), float(sqrt_1m_alpha_prev), n, *((pt,) if pt else ()), _stream())
    return prev, x0


def cfg_ddim_step_width(local, direction, x, prev, x0, ratio=None):
    """Elements per thread of the kernels cfg_ddim_step launches for these buffers: 4 (16-byte accesses) or 1 (scalar), by the
    library's own launch predicate (ed_cfg_ddim_step_width; launches nothing).  Without ``ratio`` the choice depends on the
    element count and the alignment alone; a ratio also asks that a sample be a whole number of float4s."""
    n = x.numel()
    B = 0 if ratio is None else ratio.numel()
    ptrs = [_dev(t, torch.float32) for t in (local, direction, x, prev, x0)]
    rp = _opt(ratio, torch.float32, "ratio")
    _LAUNCH["device"] = None  # a query, not a launch
    return _hip.lib().ed_cfg_ddim_step_width(*ptrs, n, rp, B)


def undo_step(x_in, noise, coef, x_out):
    """noise f32 [n_sub, *x.shape], coef f32 [n_sub,2] on device."""
    n = x_in.numel()
    n_sub = noise.shape[0]
    assert noise.numel() == n_sub * n and coef.numel() == 2 * n_sub and x_out.numel() == n
    _call("ed_undo_step", _dev(x_in, torch.float32), _dev(noise, torch.float32), _dev(coef, torch.float32),
          _dev(x_out, torch.float32), n_sub, n, _stream())
    return x_out


def rrg_update(prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g, sqrt_beta_t, sqrt_alpha_t, norm, weight,
               prediction_type="epsilon", ratio_low=None, guidance_rescale=0.0):
    """``ratio_low`` (f32 [B] from guidance_moments on low_uncond / low_dir) applies the guidance rescale to the
    reduced-resolution prediction low_uncond + g * low_dir (ed_rrg_update_gr); None is the plain launch."""
    pt = _pred_code(prediction_type)
    B, C, H, W = prev.shape
    h, w = low_latent.shape[-2:]
    assert tuple(low_latent.shape) == (B, C, h, w) == tuple(low_uncond.shape) == tuple(low_dir.shape)
    assert up_row.numel() == H and up_col.numel() == W
    if ratio_low is None and float(guidance_rescale) != 0.0:
        _reject("rrg_update: guidance_rescale needs ratio_low (guidance_moments)")
    if ratio_low is not None:
        gr_f, omgr_f = rescale_coefficients(guidance_rescale)  # ValueError before any argument of the launch is taken
        _call("ed_rrg_update_gr",
              _dev(prev, torch.float32), _dev(x0, torch.float32), _dev(low_latent, torch.float32),
              _dev(low_uncond, torch.float32), _dev(low_dir, torch.float32),
              _dev(up_row, torch.int32), _dev(up_col, torch.int32), _dev(out, torch.float32),
              float(g), float(sqrt_beta_t), float(sqrt_alpha_t), float(norm), float(weight),
              B, C, H, W, h, w, pt, _ratio_ptr(ratio_low, B, "ratio_low"), gr_f, omgr_f, _stream())
        return out
    _call("ed_rrg_update_pt" if pt else "ed_rrg_update",
          _dev(prev, torch.float32), _dev(x0, torch.float32), _dev(low_latent, torch.float32),
          _dev(low_uncond, torch.float32), _dev(low_dir, torch.float32),
          _dev(up_row, torch.int32), _dev(up_col, torch.int32), _dev(out, torch.float32),
          float(g), float(sqrt_beta_t), float(sqrt_alpha_t), float(norm), float(weight),
          B, C, H, W, h, w, *((pt,) if pt else ()), _stream())
    return out


def gather2d(inp, out, src_n, rows, cols):
    """out[n,c,i,j] = inp[src_n[n],c,rows[n,i],cols[n,j]] (0 where an index is negative)."""
    _, C, H, W = inp.shape
    N, C2, oh, ow = out.shape
    assert C2 == C and tuple(rows.shape) == (N, oh) and tuple(cols.shape) == (N, ow) and src_n.numel() == N
    _call("ed_gather2d", _dev(inp, None, "inp"), _code(inp, "inp"), _dev(out, None, "out"), _code(out, "out"),
          C, H, W, _dev(src_n, torch.int32), _dev(rows, torch.int32), _dev(cols, torch.int32),
          N, oh, ow, _stream())
    return out


def tile_gather_pad(latent, tiles, tile_y0, tile_x0, scaling_factor):
    """latent f32 [B,C,H,W] -> tiles [(T*B),C,Ts,Ts] = zero-haloed windows / scaling_factor."""
    B, C, H, W = latent.shape
    T = tile_y0.numel()
    rows, C2, Ts, Ts2 = tiles.shape
    assert rows == T * B and C2 == C and Ts == Ts2
    _call("ed_tile_gather_pad", _dev(latent, torch.float32), _dev(tiles, None, "tiles"), _code(tiles, "tiles"),
          B, C, H, W, _dev(tile_y0, torch.int32), _dev(tile_x0, torch.int32), T, Ts,
          float(scaling_factor), _stream())
    return tiles


TILE_MAXC = 4


def tile_accumulate_normalise(decoded, image, n_col_tiles, row_tile, row_src, col_tile, col_src):
    """decoded [(T*B),3,TP,TP] raw VAE output -> image f32 [B,3,HP,WP] = mean over covering tiles of clamp(v/2+.5)."""
    B, Cimg, HP, WP = image.shape
    rows, C2, TP, TP2 = decoded.shape
    assert C2 == Cimg and TP == TP2 and rows % B == 0
    assert row_tile.numel() == HP * TILE_MAXC == row_src.numel() and col_tile.numel() == WP * TILE_MAXC == col_src.numel()
    _call("ed_tile_accumulate_normalise", _dev(decoded, None, "decoded"), _code(decoded, "decoded"),
          _dev(image, torch.float32), B, Cimg, HP, WP, TP, n_col_tiles,
          _dev(row_tile, torch.int32), _dev(row_src, torch.int32),
          _dev(col_tile, torch.int32), _dev(col_src, torch.int32), _stream())
    return image


# ---- fused kernels inside the UNet (csrc/unet_kernels.hip) ---------------------------------------------------------
def geglu(x2, inner):
    """x2 [..., 2*inner] (16-bit, contiguous) -> [..., inner] = x2[..., :inner] * gelu(x2[..., inner:])."""
    assert x2.shape[-1] == 2 * inner
    out = torch.empty(x2.shape[:-1] + (inner,), dtype=x2.dtype, device=x2.device)
    TIMER.note_work("ed_geglu", nbytes=1.5 * x2.numel() * x2.element_size())  # read 2I, write I
    _call("ed_geglu", _dev(x2, None, "x2"), _dev(out, None, "out"), _code(x2, "x2"), x2.numel() // (2 * inner), inner,
          _stream())
    return out


# ---- dense contractions (csrc/gemm_kernels.hip) ---------------------------------------------------------------------
GEMM_BM, GEMM_BN = 256, 128   # rows / value columns of one workgroup tile (256 output columns for the plain epilogue)
GEMM_MIN_BLOCKS = 96          # below this many workgroups the 256-CU chip is mostly idle: the library call stays
GEMM_CUS = 256                # one 128-KiB-LDS workgroup per CU: the grid runs in rounds of 256 tiles
GEMM_MIN_ROUND_FILL = 0.7     # a multi-round grid whose rounds are on average emptier than this loses to the library's stream-K


GEMM_ROWS_TILE_COST = 0.72    # csrc/gemm_kernels.hip ROWS_TILE_COST: a round of 128-row tiles relative to a round of 256-row ones
GEMM_ROWS_MIN_BLOCKS_LINEAR = 200   # ... for projections (short kernels: the in-situ measurement, linear_wins)
GEMM_ROWS_MIN_BLOCKS = 80      # 128-row tiles below which even the half-height grid leaves the chip mostly idle (SD 1.5's 8 x 8 level: 50)


def gemm_rows_mode(M, n_col_blocks):
    """Does the launcher run this grid as 128-row tiles (csrc/gemm_kernels.hip, launch(): fewer effective rounds)?  The mirror of its rule."""
    b256, b128 = -(-M // GEMM_BM) * n_col_blocks, -(-M // (GEMM_BM // 2)) * n_col_blocks
    return -(-b128 // GEMM_CUS) * GEMM_ROWS_TILE_COST < -(-b256 // GEMM_CUS) - 1e-9


def _gemm_grid_ok(blocks, M=None, n_col_blocks=None, min_fill=None):
    """Is a grid of ``blocks`` 256 x 256 tiles worth launching?  Measured (profiles/r4_s2_probe_gemm_*.jsonl): 25 tiles lose
    2.4 x, 100-120 tiles win 1.06-1.18 x (the library under-fills the chip as well), 288 tiles = 2 rounds, the second 12 %
    full, lose 0.83-0.90 x; 400 tiles (78 %) and everything fuller win.  Round 6: an under-filled grid runs as 128-row tiles when that
    takes fewer effective rounds (``gemm_rows_mode``; profiles/r6_s4_gemm_rows_mode.jsonl: 120 tiles 1.35-1.45 x faster than as 256-row
    tiles -- 1.95 x MIOpen on the batch-6 32 x 32 convolutions -- and 20-60 tiles, the 1- / 3-row per-rank forwards of the multi-GPU layout,
    1.24-1.93 x the library call), so such a grid is taken from GEMM_ROWS_MIN_BLOCKS half-height tiles on."""
    if M is not None and n_col_blocks is not None and gemm_rows_mode(M, n_col_blocks):
        return -(-M // (GEMM_BM // 2)) * n_col_blocks >= (GEMM_ROWS_MIN_BLOCKS if GEMM_MIN_BLOCKS > 1 else 1)
    if blocks < GEMM_MIN_BLOCKS:
        return False
    rounds = -(-blocks // GEMM_CUS)
    return rounds == 1 or blocks / (rounds * GEMM_CUS) >= (GEMM_MIN_ROUND_FILL if min_fill is None else min_fill)


def _gemm_x(x, name):
    """A [..., K] activation as the kernel sees it: M rows of K contiguous 16-bit values."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16):
        _reject(f"{name} must be a 16-bit tensor on the MI355X; no CPU fallback")
    if not x.is_contiguous():
        _reject(f"{name} must be contiguous")
    return x.numel() // x.shape[-1], x.shape[-1]


def geglu_gemm_ok(M, K, I):
    return K % 64 == 0 and K >= 64 and I % GEMM_BN == 0 and M * K * 2 < 2 ** 31 - 16 and 2 * I * K * 2 < 2 ** 31 - 16


def geglu_gemm_wins(M, K, I):
    """Where the model uses ed_geglu_gemm: every shape the kernel takes whose grid fills the chip.  The fused pair beats hipBLASLt +
    ed_geglu by 1.11-1.91 x on full grids, but it is the same main loop as ed_linear, which loses 2.4 x on a 25-tile grid
    (one 128-KiB-LDS workgroup per CU): a batch-1 / batch-2 forward at the 16 x 16 or 32 x 32 level stays with the library
    (ADVICE r4).  The GEGLU kernel is persistent (one workgroup per CU walking the tiles), so there is no round-fill condition."""
    return geglu_gemm_ok(M, K, I) and -(-M // GEMM_BM) * (I // GEMM_BN) >= GEMM_MIN_BLOCKS


def geglu_gemm(x, w, bias=None):
    """x [..., K], w [2I, K], bias [2I] -> [..., I] = (x w_v^T + b_v) * gelu(x w_g^T + b_g).  See ed_geglu_gemm."""
    M, K = _gemm_x(x, "x")
    I = w.shape[0] // 2
    if tuple(w.shape) != (2 * I, K) or not geglu_gemm_ok(M, K, I):
        _reject(f"geglu_gemm: unsupported shape x {tuple(x.shape)} w {tuple(w.shape)}")
    out = torch.empty(x.shape[:-1] + (I,), dtype=x.dtype, device=x.device)
    TIMER.note_work("ed_geglu_gemm", flops=4.0 * M * K * I, nbytes=2.0 * (M * K + 2 * I * K + M * I))
    _call("ed_geglu_gemm", _dev(x, None, "x"), _dev(w, x.dtype, "w"), _opt(bias, x.dtype, "bias"), _dev(out, None, "out"),
          _code(x, "x"), M, K, I, _stream())
    return out


def linear_ok(M, K, N):
    """what the kernel takes (linear_wins: where the model uses it)"""
    return K % 64 == 0 and K >= 64 and N % 8 == 0 and M * K * 2 < 2 ** 31 - 16 and N * K * 2 < 2 ** 31 - 16


def linear_wins(M, K, N):
    """Where ed_linear measured faster than hipBLASLt on the MI355X in fp16, over every projection shape of the SDXL (batch 20
    and 6) and SD1.5 (batch 20) forwards (profiles/r4_s2_probe_gemm_*.jsonl): hipBLASLt is weak when K <= 640 or N <= 640
    (388-900 TFLOP/s; this kernel 1.09-1.58 x) and strong on the K >= 1280, N >= 1280 projections (930-1320 TFLOP/s; this
    kernel 0.70-0.95 x there), whenever the grid fills the chip (_gemm_grid_ok)."""
    ncb = -(-N // (2 * GEMM_BN))
    if linear_ok(M, K, N) and K <= 1280 and gemm_rows_mode(M, ncb):
        # round 6: an under-filled grid as 128-row tiles beats the library up to K = 1280 whatever N in an isolated loop (6144 x 1280 -> 1280:
        # 1.06 x, 3072 x 1280 -> 1280: 1.27 x, 4096 x 640 -> 640: 1.40 x; K = 5120 does not -- the library splits K) -- but IN the forward only the
        # batch-6 shapes keep that (240 half tiles: + 0.35 %); the 40-120-tile grids of the 3- and 1-row forwards measured 1.27-1.40 x alone
        # cost those forwards 4.0 % and 2.1 % (profiles/r6_s7_policy_split.jsonl: a 128-KiB-LDS workgroup cannot start beside the
        # previous kernel's tail, the library's small tiles can), so projections are taken from GEMM_ROWS_MIN_BLOCKS_LINEAR half tiles on
        return -(-M // (GEMM_BM // 2)) * ncb >= GEMM_ROWS_MIN_BLOCKS_LINEAR
    blocks = -(-M // GEMM_BM) * ncb
    if K > 1280 and blocks < 200:      # long K on a grid well under one round: the library splits K (12288 x 2560 -> 640, 144 tiles: 0.80 x)
        return False
    return linear_ok(M, K, N) and (K <= 640 or N <= 640) and _gemm_grid_ok(blocks)


def linear(x, w, bias=None, residual=None):
    """x [..., K], w [N, K] -> x w^T + bias (+ residual [..., N]).  See ed_linear."""
    M, K = _gemm_x(x, "x")
    N = w.shape[0]
    if tuple(w.shape) != (N, K) or not linear_ok(M, K, N):
        _reject(f"linear: unsupported shape x {tuple(x.shape)} w {tuple(w.shape)}")
    out = torch.empty(x.shape[:-1] + (N,), dtype=x.dtype, device=x.device)
    if residual is not None and (residual.shape != out.shape or residual.dtype != x.dtype):
        _reject("linear: residual must match the output")
    TIMER.note_work("ed_linear", flops=2.0 * M * K * N, nbytes=2.0 * (M * K + N * K + M * N * (2 if residual is not None else 1)))
    _call("ed_linear", _dev(x, None, "x"), _dev(w, x.dtype, "w"), _opt(bias, x.dtype, "bias"), _opt(residual, x.dtype, "residual"),
          _dev(out, None, "out"), _code(x, "x"), M, K, N, _stream())
    return out


def conv3x3_ok(B, H, W, Cin, N):
    """what the kernel takes (conv3x3_wins: where the model uses it)"""
    M = B * H * W
    return Cin % 64 == 0 and N % 8 == 0 and M * Cin * 2 < 2 ** 31 - 16 and N * 9 * Cin * 2 < 2 ** 31 - 16


def conv3x3_wins(B, H, W, Cin, N):
    """Where ed_conv3x3_nhwc measured faster than MIOpen's CK kernels (fp16, profiles/r4_s2_probe_gemm_*.jsonl): every
    ResnetBlock / upsampler shape whose grid fills the chip -- 1.10-1.59 x at batch 20, 1.06-1.49 x at batch 6 except the
    288-tile 64 x 64 x 640 shapes (0.83-0.90 x in round 4, 1.17 x since round 6), 0.4 x on SD1.5's 25-tile 8 x 8 level."""
    ncb = -(-N // (2 * GEMM_BN))
    # round 6: with the long-K loop, half column tiles and the channel-block-major walk the 288-tile 64 x 64 x 640 shapes of the batch-6
    # forward now measure 1.17 x MIOpen (profiles/r6_s4_gemm_rows_mode.jsonl; round 4: 0.83-0.90 x): no round-fill condition for convolutions
    return conv3x3_ok(B, H, W, Cin, N) and _gemm_grid_ok(-(-(B * H * W) // GEMM_BM) * ncb, B * H * W, ncb, min_fill=0.5)


def conv3x3_nhwc(x, w, bias=None, sample_bias=None, residual=None):
    """x [B,Cin,H,W] and w [N,Cin,3,3] in torch.channels_last memory format (16-bit) -> conv2d(x, w, stride 1, padding 1)
    + bias[n] + sample_bias[b, n] + residual, channels_last.  See ed_conv3x3_nhwc."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16)):
        _reject("conv3x3_nhwc: x must be a 16-bit [B,C,H,W] tensor on the MI355X; no CPU fallback")
    B, Cin, H, W = x.shape
    N = w.shape[0]
    cl = torch.channels_last
    if tuple(w.shape) != (N, Cin, 3, 3) or w.dtype != x.dtype or not conv3x3_ok(B, H, W, Cin, N):
        _reject(f"conv3x3_nhwc: unsupported shape x {tuple(x.shape)} w {tuple(w.shape)}")
    if not x.is_contiguous(memory_format=cl) or not w.is_contiguous(memory_format=cl):
        _reject("conv3x3_nhwc: x and w must be channels_last")
    out = torch.empty((B, N, H, W), dtype=x.dtype, device=x.device, memory_format=cl)
    if residual is not None and (residual.shape != out.shape or residual.dtype != x.dtype or not residual.is_contiguous(memory_format=cl)):
        _reject("conv3x3_nhwc: residual must be a channels_last tensor of the output's shape")
    if sample_bias is not None and tuple(sample_bias.shape) != (B, N):
        _reject("conv3x3_nhwc: sample_bias must be [B, N]")
    TIMER.note_work("ed_conv3x3_nhwc", flops=2.0 * B * H * W * 9 * Cin * N,
                    nbytes=2.0 * (B * H * W * (Cin + N * (2 if residual is not None else 1)) + 9 * Cin * N))
    BA = conv3x3_batch_split(B, H, W, N) if CONV_BATCH_SPLIT else None
    for b0, nb in (((0, B),) if BA is None else ((0, BA), (BA, B - BA))):
        # (the tail of a batch whose grid ends in a nearly empty round of 256-row tiles is launched on its own: the launcher runs it as 128-row tiles)
        px, po = b0 * H * W * Cin * x.element_size(), b0 * H * W * N * x.element_size()
        _call("ed_conv3x3_nhwc", x.data_ptr() + px, w.data_ptr(), _opt(bias, x.dtype, "bias"),
              None if sample_bias is None else _dev(sample_bias, x.dtype, "sample_bias") + b0 * N * x.element_size(),
              None if residual is None else residual.data_ptr() + po, out.data_ptr() + po, _code(x, "x"), nb, H, W, Cin, N, _stream_of(x))
    return out


CONV_BATCH_SPLIT = True


def conv3x3_batch_split(B, H, W, N):
    """Samples of a batch ed_conv3x3_nhwc should run in a first launch (the rest in a second), or None for one launch.  One 128-KiB-LDS
    workgroup per CU: a grid runs in rounds of 256 tiles, and the SDXL forwards of the default bench end some of them badly -- the 32 x 32
    convolutions at 40 rows are 800 tiles: three full rounds and a fourth 12.5 % full.  Splitting the batch at a SAMPLE boundary (whole images:
    the pixel geometry of either part is unchanged, and so is every output bit) lets the launcher run the short tail as 128-row tiles (0.72 of a
    round): 3.72 rounds instead of 4.  Taken when the launcher's own cost model says the two launches finish at least 0.1 round sooner."""
    HW = H * W
    if HW % GEMM_BM or B < 2:
        return None
    ncb = -(-N // (2 * GEMM_BN))
    tps = HW // GEMM_BM * ncb                      # 256-row tiles per sample
    total = B * tps

    def rounds(tiles):                             # the launcher's choice for a grid of `tiles` full tiles (csrc/gemm_kernels.hip, launch())
        return min(-(-tiles // GEMM_CUS), -(-2 * tiles // GEMM_CUS) * GEMM_ROWS_TILE_COST)

    full = total // GEMM_CUS
    # measured (profiles/r6_s25_*): 800 tiles (3 full rounds + 32 tiles) +5.6...5.9 % per convolution, bit-identical, +0.23 % of the 40-row forward;
    # 576 tiles (2 + 64) -4 % and 288 (1 + 32) +2.6 % alone, nothing in the forward: the model is only trusted from three full rounds on
    if full < 3 or total % GEMM_CUS == 0:
        return None
    BA = full * GEMM_CUS // tps
    if BA <= 0 or BA >= B:
        return None
    return BA if -(-BA * tps // GEMM_CUS) + rounds((B - BA) * tps) < rounds(total) - 0.1 else None


def conv3x3_up2x_wins(B, H, W, Cin, N):
    """Where Upsample2D runs as ONE ed_conv3x3_nhwc_up2x launch (H, W = the OUTPUT size): wherever the convolution on the materialised
    upsampling would run as 256-row tiles of ed_conv3x3_nhwc (the fused kernel has no 128-row instantiation: the upsamplers' grids are
    80+ tiles per row of the batch) -- the upsampled tensor is then never written or read back (4x the source)."""
    ncb = -(-N // (2 * GEMM_BN))
    return (H % 2 == 0 and W % 2 == 0 and conv3x3_wins(B, H, W, Cin, N) and not gemm_rows_mode(B * H * W, ncb)
            and B * (H // 2) * (W // 2) * Cin * 2 < 2 ** 31 - 16)


def conv3x3_nhwc_up2x(x, w, bias=None):
    """x [B,Cin,H/2,W/2] and w [N,Cin,3,3] channels_last 16-bit -> conv2d(nearest_upsample_2x(x), w, stride 1, padding 1) + bias as
    channels_last [B,N,H,W]; the upsampled tensor never exists.  See ed_conv3x3_nhwc_up2x."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16)):
        _reject("conv3x3_nhwc_up2x: x must be a 16-bit [B,C,H,W] tensor on the MI355X; no CPU fallback")
    B, Cin, Hs, Ws = x.shape
    H, W = 2 * Hs, 2 * Ws
    N = w.shape[0]
    cl = torch.channels_last
    if tuple(w.shape) != (N, Cin, 3, 3) or w.dtype != x.dtype or not conv3x3_ok(B, H, W, Cin, N):
        _reject(f"conv3x3_nhwc_up2x: unsupported shape x {tuple(x.shape)} w {tuple(w.shape)}")
    if not x.is_contiguous(memory_format=cl) or not w.is_contiguous(memory_format=cl):
        _reject("conv3x3_nhwc_up2x: x and w must be channels_last")
    out = torch.empty((B, N, H, W), dtype=x.dtype, device=x.device, memory_format=cl)
    TIMER.note_work("ed_conv3x3_nhwc_up2x", flops=2.0 * B * H * W * 9 * Cin * N, nbytes=2.0 * (B * Hs * Ws * Cin + B * H * W * N + 9 * Cin * N))
    _call("ed_conv3x3_nhwc_up2x", x.data_ptr(), w.data_ptr(), _opt(bias, x.dtype, "bias"), out.data_ptr(), _code(x, "x"), B, H, W, Cin, N,
          _stream_of(x))
    return out


def conv3x3_s2_wins(B, H, W, Cin, N):
    """Where Downsample2D runs as ed_conv3x3_nhwc_s2 (H, W = the OUTPUT size): full grids of 256-row tiles, as for the stride-1 kernel
    (no 128-row instantiation)."""
    ncb = -(-N // (2 * GEMM_BN))
    return (conv3x3_wins(B, H, W, Cin, N) and not gemm_rows_mode(B * H * W, ncb) and 4 * B * H * W * Cin * 2 < 2 ** 31 - 16)


def conv3x3_nhwc_s2(x, w, bias=None):
    """x [B,Cin,2H,2W] and w [N,Cin,3,3] channels_last 16-bit -> conv2d(x, w, stride 2, padding 1) + bias as channels_last [B,N,H,W].
    See ed_conv3x3_nhwc_s2."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16)):
        _reject("conv3x3_nhwc_s2: x must be a 16-bit [B,C,H,W] tensor on the MI355X; no CPU fallback")
    B, Cin, Hi, Wi = x.shape
    if Hi % 2 or Wi % 2:
        _reject("conv3x3_nhwc_s2: even input height and width")
    H, W = Hi // 2, Wi // 2
    N = w.shape[0]
    cl = torch.channels_last
    if tuple(w.shape) != (N, Cin, 3, 3) or w.dtype != x.dtype or not conv3x3_ok(B, Hi, Wi, Cin, N):
        _reject(f"conv3x3_nhwc_s2: unsupported shape x {tuple(x.shape)} w {tuple(w.shape)}")
    if not x.is_contiguous(memory_format=cl) or not w.is_contiguous(memory_format=cl):
        _reject("conv3x3_nhwc_s2: x and w must be channels_last")
    out = torch.empty((B, N, H, W), dtype=x.dtype, device=x.device, memory_format=cl)
    TIMER.note_work("ed_conv3x3_nhwc_s2", flops=2.0 * B * H * W * 9 * Cin * N, nbytes=2.0 * (B * Hi * Wi * Cin + B * H * W * N + 9 * Cin * N))
    _call("ed_conv3x3_nhwc_s2", x.data_ptr(), w.data_ptr(), _opt(bias, x.dtype, "bias"), out.data_ptr(), _code(x, "x"), B, H, W, Cin, N,
          _stream_of(x))
    return out


GROUPNORM_SPLIT = True  # large groups: statistics + apply as two fully parallel launches (A/B switch)


def groupnorm(x, gamma, beta, groups, eps, silu=False, tokens=False, chan_bias=None, conv_bias=None):
    """x [N,C,H,W] NCHW 16-bit -> GroupNorm(+SiLU) as [N,C,H,W], or [N,H*W,C] when ``tokens``.
    ``conv_bias`` [C] / ``chan_bias`` [N,C] (optional): normalise round16(round16(x + conv_bias) + chan_bias) instead of
    x (each add only when given) -- see ed_groupnorm."""
    N, C, H, W = x.shape
    if chan_bias is not None:
        assert tuple(chan_bias.shape) == (N, C)
    if conv_bias is not None:
        assert tuple(conv_bias.shape) == (C,)
    out = torch.empty((N, H * W, C) if tokens else (N, C, H, W), dtype=x.dtype, device=x.device)
    TIMER.note_work("ed_groupnorm", nbytes=3.0 * x.numel() * x.element_size())  # statistics pass + apply pass + write
    ws = None
    if GROUPNORM_SPLIT:
        nbytes = _hip.lib().ed_groupnorm_workspace(N, C, H * W, groups)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    _call("ed_groupnorm", _dev(x, None, "x"), _dev(gamma, x.dtype, "gamma"), _dev(beta, x.dtype, "beta"),
          _opt(conv_bias, x.dtype, "conv_bias"), _opt(chan_bias, x.dtype, "chan_bias"), _dev(out, None, "out"),
          _opt(ws, torch.float32, "workspace"), _code(x, "x"), N, C, H * W, groups, float(eps),
          int(silu), int(tokens), _stream())
    return out


def groupnorm_nhwc(x, gamma, beta, groups, eps, silu=False, chan_bias=None, conv_bias=None):
    """x [N,C,H,W] in torch.channels_last memory format (16-bit) -> GroupNorm(+SiLU), same format; optional
    ``conv_bias`` [C] / ``chan_bias`` [N,C] as in ``groupnorm``."""
    N, C, H, W = x.shape
    if not x.is_cuda:
        _reject("x must be a tensor on the MI355X; no CPU fallback")
    if not x.is_contiguous(memory_format=torch.channels_last):
        _reject("x must be channels_last")
    out = torch.empty_like(x, memory_format=torch.channels_last)
    nbytes = _hip.lib().ed_groupnorm_nhwc_workspace(N, C, H * W, groups)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    TIMER.note_work("ed_groupnorm_nhwc", nbytes=3.0 * x.numel() * x.element_size())
    _call("ed_groupnorm_nhwc", x.data_ptr(), _dev(gamma, x.dtype, "gamma"), _dev(beta, x.dtype, "beta"),
          _opt(conv_bias, x.dtype, "conv_bias"), _opt(chan_bias, x.dtype, "chan_bias"), out.data_ptr(),
          _dev(ws, torch.float32, "workspace"), _code(x, "x"), N, C, H * W, groups, float(eps), int(silu), _stream())
    return out


def groupnorm_nhwc_cat_ok(x1, x2, groups):
    """can ed_groupnorm_nhwc_cat normalise cat([x1, x2], 1) of these two tensors in place?"""
    def cl16(x):
        return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and is_nhwc(x)
    if not (cl16(x1) and cl16(x2) and x1.dtype == x2.dtype and x1.device == x2.device and x1.shape[0] == x2.shape[0]
            and x1.shape[2:] == x2.shape[2:]):
        return False
    C1, C = x1.shape[1], x1.shape[1] + x2.shape[1]
    return C1 % 8 == 0 and C % 8 == 0 and C % groups == 0 and C // groups >= 8 and groups <= 256 and C <= 4096


def groupnorm_nhwc_cat(x1, x2, gamma, beta, groups, eps, silu=False):
    """GroupNorm(+SiLU) of torch.cat([x1, x2], dim=1) for two channels_last 16-bit tensors [N,C1,H,W], [N,C2,H,W], read in place
    (the concatenation is never written) -> channels_last [N, C1 + C2, H, W].  See ed_groupnorm_nhwc_cat."""
    if not groupnorm_nhwc_cat_ok(x1, x2, groups):
        _reject("groupnorm_nhwc_cat: two channels_last 16-bit tensors of the same dtype / batch / size on the MI355X, C1 % 8 == 0, "
                "(C1 + C2) / groups >= 8; no CPU fallback")
    N, C1, H, W = x1.shape
    C2 = x2.shape[1]
    out = torch.empty((N, C1 + C2, H, W), dtype=x1.dtype, device=x1.device, memory_format=torch.channels_last)
    nbytes = _hip.lib().ed_groupnorm_nhwc_workspace(N, C1 + C2, H * W, groups)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x1.device)
    TIMER.note_work("ed_groupnorm_nhwc_cat", nbytes=3.0 * out.numel() * out.element_size())
    _LAUNCH["device"] = x1.device
    _call("ed_groupnorm_nhwc_cat", x1.data_ptr(), x2.data_ptr(), _dev(gamma, x1.dtype, "gamma"), _dev(beta, x1.dtype, "beta"),
          out.data_ptr(), ws.data_ptr(), _DTYPE[x1.dtype], N, C1, C2, H * W, groups, float(eps), int(silu), _stream())
    return out


def layernorm(x, gamma, beta, eps):
    """x [..., D] contiguous 16-bit -> LayerNorm over D."""
    D = x.shape[-1]
    out = torch.empty_like(x)
    TIMER.note_work("ed_layernorm", nbytes=2.0 * x.numel() * x.element_size())
    _call("ed_layernorm", _dev(x, None, "x"), _dev(gamma, x.dtype, "gamma"), _dev(beta, x.dtype, "beta"),
          _dev(out, None, "out"), _code(x, "x"), x.numel() // D, D, float(eps), _stream())
    return out


def add_layernorm(a, b, gamma, beta, eps):
    """a, b [..., D] contiguous 16-bit -> (a + b, LayerNorm(a + b)); the sum is rounded to the 16-bit type first."""
    D = a.shape[-1]
    assert a.shape == b.shape and a.dtype == b.dtype
    s, out = torch.empty_like(a), torch.empty_like(a)
    TIMER.note_work("ed_add_layernorm", nbytes=4.0 * a.numel() * a.element_size())
    _call("ed_add_layernorm", _dev(a, None, "a"), _dev(b, a.dtype, "b"), _dev(gamma, a.dtype, "gamma"),
          _dev(beta, a.dtype, "beta"), _dev(s, None, "sum"), _dev(out, None, "out"), _code(a, "a"), a.numel() // D, D,
          float(eps), _stream())
    return s, out


# ---- the fp32-residual-stream mode (models.UNet2DConditionModel.residual_fp32): the layers that read / write the stream ----------------
def _stream_ok(x, w):
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and w.dtype in (torch.float16, torch.bfloat16)
            and w.device == x.device)


def layernorm_s32(x, gamma, beta, eps):
    """x [..., D] contiguous fp32 (the residual stream) -> LayerNorm over D in gamma's 16-bit dtype (ed_layernorm_s32)."""
    if not _stream_ok(x, gamma) or not x.is_contiguous():
        _reject("layernorm_s32: x must be a contiguous fp32 tensor on the MI355X and gamma 16-bit; no CPU fallback")
    D = x.shape[-1]
    out = torch.empty(x.shape, dtype=gamma.dtype, device=x.device)
    TIMER.note_work("ed_layernorm_s32", nbytes=x.numel() * 6.0)
    _LAUNCH["device"] = x.device
    _call("ed_layernorm_s32", x.data_ptr(), _dev(gamma, None, "gamma"), _dev(beta, gamma.dtype, "beta"), out.data_ptr(),
          _DTYPE[gamma.dtype], x.numel() // D, D, float(eps), _stream())
    return out


def add_layernorm_s32(a, b, gamma, beta, eps):
    """a [..., D] 16-bit (a branch result), b [..., D] fp32 (the residual stream) -> (a + b in fp32, LayerNorm(a + b) in a's dtype)."""
    if not (_stream_ok(b, a) and a.shape == b.shape and a.is_contiguous() and b.is_contiguous() and gamma.dtype == a.dtype):
        _reject("add_layernorm_s32: a must be 16-bit and b fp32, same shape, contiguous, on the MI355X; no CPU fallback")
    D = a.shape[-1]
    s, out = torch.empty_like(b), torch.empty_like(a)
    TIMER.note_work("ed_add_layernorm_s32", nbytes=a.numel() * 12.0)
    _LAUNCH["device"] = a.device
    _call("ed_add_layernorm_s32", a.data_ptr(), b.data_ptr(), _dev(gamma, None, "gamma"), _dev(beta, a.dtype, "beta"), s.data_ptr(),
          out.data_ptr(), _DTYPE[a.dtype], a.numel() // D, D, float(eps), _stream())
    return s, out


def groupnorm_nhwc_s32(x, gamma, beta, groups, eps, silu=False):
    """x [N,C,H,W] fp32 in channels_last memory (the residual stream) -> GroupNorm(+SiLU) in gamma's 16-bit dtype, channels_last."""
    if not _stream_ok(x, gamma) or x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        _reject("groupnorm_nhwc_s32: x must be an fp32 channels_last [N,C,H,W] tensor on the MI355X and gamma 16-bit; no CPU fallback")
    N, C, H, W = x.shape
    out = torch.empty((N, C, H, W), dtype=gamma.dtype, device=x.device, memory_format=torch.channels_last)
    nbytes = _hip.lib().ed_groupnorm_nhwc_workspace(N, C, H * W, groups)
    ws = torch.empty(max(4, nbytes // 4), dtype=torch.float32, device=x.device)
    TIMER.note_work("ed_groupnorm_nhwc_s32", nbytes=x.numel() * 10.0)
    _LAUNCH["device"] = x.device
    _call("ed_groupnorm_nhwc_s32", x.data_ptr(), _dev(gamma, None, "gamma"), _dev(beta, gamma.dtype, "beta"), out.data_ptr(),
          ws.data_ptr(), _DTYPE[gamma.dtype], N, C, H * W, groups, float(eps), int(silu), _stream())
    return out


def bias_residual_add(h, h_bias, res, res_bias=None):
    """round16(res (+ res_bias[c])) + round16(h + h_bias[c]) for 16-bit [N,C,H,W] tensors that are both NCHW-contiguous
    or both channels_last (ResnetBlock2D's closing add); the result has the same memory format."""
    N, C, H, W = h.shape
    assert res.shape == h.shape and res.dtype == h.dtype
    if not (h.is_cuda and res.is_cuda):
        _reject("bias_residual_add: h and res must be tensors on the MI355X; no CPU fallback")
    cl = is_nhwc(h) and C % 8 == 0
    fmt = torch.channels_last if cl else torch.contiguous_format
    # mixed layouts only arise on fallback paths (a torch GroupNorm returning NCHW inside a channels-last model): follow
    # the convolution output's layout, re-laying-out the other operand
    h = h.contiguous(memory_format=fmt)
    res = res.contiguous(memory_format=fmt)
    out = torch.empty_like(h, memory_format=fmt)
    TIMER.note_work("ed_bias_residual_add", nbytes=3.0 * h.numel() * h.element_size())
    _call("ed_bias_residual_add", h.data_ptr(), _opt(h_bias, h.dtype, "h_bias"), res.data_ptr(),
          _opt(res_bias, h.dtype, "res_bias"), out.data_ptr(), _code(h, "h"), N, C, H * W, int(cl), _stream_of(h))
    return out


def tokens_add_nchw(x, tokens):
    """x [N,C,H,W] + tokens [N,H*W,C] (16-bit, contiguous) -> [N,C,H,W]: the residual add closing a transformer."""
    N, C, H, W = x.shape
    assert tuple(tokens.shape) == (N, H * W, C) and tokens.dtype == x.dtype
    out = torch.empty_like(x)
    TIMER.note_work("ed_tokens_add_nchw", nbytes=3.0 * x.numel() * x.element_size())
    _call("ed_tokens_add_nchw", _dev(x, None, "x"), _dev(tokens, None, "tokens"), _dev(out, None, "out"), _code(x, "x"),
          N, C, H * W, _stream())
    return out


def _pixel_weights(what, wx, wy, H, W):
    """the optional fp32 multiplicity vectors wx [W] / wy [H] of a weighted GroupNorm, checked"""
    for name, w, n in (("wx", wx, W), ("wy", wy, H)):
        if w is not None and tuple(w.shape) != (n,):
            _reject(f"{what}: {name} must have shape ({n},), got {tuple(w.shape)}")
    return _opt(wx, torch.float32, "wx"), _opt(wy, torch.float32, "wy")


def groupnorm_f32(x, gamma, beta, groups, eps, silu=False, wx=None, wy=None):
    """x fp32 [N,C,H,W] NCHW-contiguous -> GroupNorm(+SiLU), fp32 (the VAE's normalisation layers; ed_groupnorm_f32).  ``wx`` [W] /
    ``wy`` [H] (fp32, optional): pixel (y, x) counts wy[y] * wx[x] times in the statistics (ed_groupnorm_f32_weighted)."""
    N, C, H, W = x.shape
    if (H * W) % 4:
        _reject("groupnorm_f32: H*W must be a multiple of 4")
    out = torch.empty_like(x)
    nbytes = _hip.lib().ed_groupnorm_f32_workspace(N, C, H * W, groups) * (1 if wx is None and wy is None else 3)   # (+ double partials)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=x.device)
    head = (_dev(x, torch.float32, "x"), _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"),
            _dev(out, torch.float32, "out"), _dev(ws, torch.float32, "workspace"))
    if wx is None and wy is None:
        TIMER.note_work("ed_groupnorm_f32", nbytes=3.0 * x.numel() * 4)
        _call("ed_groupnorm_f32", *head, N, C, H * W, groups, float(eps), int(silu), _stream())
    else:
        px, py = _pixel_weights("groupnorm_f32", wx, wy, H, W)
        TIMER.note_work("ed_groupnorm_f32_weighted", nbytes=3.0 * x.numel() * 4)
        _call("ed_groupnorm_f32_weighted", *head, N, C, H, W, groups, float(eps), int(silu), px, py, _stream())
    return out


# ---- the fp32 VAE's ResnetBlock convolutions on split fp16 operands (csrc/vae_kernels.hip, gemm_kernels.hip OUT32) ------------------
def groupnorm_nhwc_f32_ok(C, groups):
    return C % groups == 0 and (C // groups) % 4 == 0 and groups <= 256 and C <= 4096


def groupnorm_nhwc_f32(x, gamma, beta, groups, eps, silu=False, split=False, wx=None, wy=None):
    """x [N,C,H,W] fp32 in channels_last memory -> GroupNorm(+SiLU) in fp32, returned as fp32 channels_last [N,C,H,W] or, with
    ``split``, as the fp16 channels_last [N,3C,H,W] = [hi | lo | hi] operand of ``conv3x3_f32out`` (hi = fp16(y), lo = fp16(y - hi)).
    See ed_groupnorm_nhwc_f32.  ``wx`` [W] / ``wy`` [H] (fp32, optional): pixel (y, x) counts wy[y] * wx[x] times in the statistics
    (ed_groupnorm_nhwc_f32_weighted)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        _reject("groupnorm_nhwc_f32: x must be an fp32 [N,C,H,W] tensor on the MI355X; no CPU fallback")
    N, C, H, W = x.shape
    cl = torch.channels_last
    if not x.is_contiguous(memory_format=cl):
        _reject("groupnorm_nhwc_f32: x must be channels_last")
    if not groupnorm_nhwc_f32_ok(C, groups):
        _reject(f"groupnorm_nhwc_f32: unsupported C = {C}, groups = {groups}")
    out = (torch.empty((N, 3 * C, H, W), dtype=torch.float16, device=x.device, memory_format=cl) if split
           else torch.empty_like(x, memory_format=cl))
    nbytes = _hip.lib().ed_groupnorm_nhwc_f32_workspace(N, C, H * W, groups) * (1 if wx is None and wy is None else 3)   # (+ double partials)
    ws = torch.empty(max(4, nbytes // 4), dtype=torch.float32, device=x.device)
    traffic = x.numel() * (4.0 + 4.0 + (6.0 if split else 4.0))
    head = (x.data_ptr(), _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"), out.data_ptr(),
            _dev(ws, torch.float32, "workspace"))
    if wx is None and wy is None:
        TIMER.note_work("ed_groupnorm_nhwc_f32", nbytes=traffic)
        _call("ed_groupnorm_nhwc_f32", *head, N, C, H * W, groups, float(eps), int(silu), int(split), _stream_of(x))
    else:
        px, py = _pixel_weights("groupnorm_nhwc_f32", wx, wy, H, W)
        TIMER.note_work("ed_groupnorm_nhwc_f32_weighted", nbytes=traffic)
        _call("ed_groupnorm_nhwc_f32_weighted", *head, N, C, H, W, groups, float(eps), int(silu), int(split), px, py, _stream_of(x))
    return out


def absmax_f32(x):
    """max |x| of a contiguous-in-memory fp32 tensor as a 1-element device tensor (ed_absmax_f32): the per-tensor figure the raw-stream
    split scales by.  No host synchronisation."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        _reject("absmax_f32: x must be an fp32 tensor on the MI355X; no CPU fallback")
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))):
        _reject("absmax_f32: x must be dense (contiguous or channels_last)")
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    TIMER.note_work("ed_absmax_f32", nbytes=x.numel() * 4.0)
    _LAUNCH["device"] = x.device
    _call("ed_absmax_f32", x.data_ptr(), x.numel(), out.data_ptr(), _stream())
    return out


def split_f32(x, upsample2x=False, absmax=None):
    """x [N,C,H,W] fp32 in channels_last memory -> the fp16 channels_last [N,3C,UH,UW] = [hi | lo | hi] operand of ``conv3x3_f32out`` for a
    raw (un-normalised) activation, U = 2 with ``upsample2x`` (nearest-neighbour upsampling folded in).  ``absmax`` (``absmax_f32(x)``, a
    1-element device tensor): the activation is scaled by 2^-e, e = max(0, exponent(absmax) - 14), before the split -- exact over the
    whole fp32 range; hand the SAME tensor to ``conv3x3_f32out(act_absmax=)``, which multiplies by 2^e.  Without it hi and lo saturate at
    fp16's largest finite value (exact up to 65504).  See ed_split_f32_nhwc."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        _reject("split_f32: x must be an fp32 [N,C,H,W] tensor on the MI355X; no CPU fallback")
    if absmax is not None and not (isinstance(absmax, torch.Tensor) and absmax.device == x.device and absmax.dtype == torch.float32
                                   and absmax.numel() == 1):
        _reject("split_f32: absmax must be a 1-element fp32 tensor on x's device")
    N, C, H, W = x.shape
    cl = torch.channels_last
    if not x.is_contiguous(memory_format=cl) or C % 4:
        _reject("split_f32: x must be channels_last with C % 4 == 0")
    u = 2 if upsample2x else 1
    out = torch.empty((N, 3 * C, u * H, u * W), dtype=torch.float16, device=x.device, memory_format=cl)
    TIMER.note_work("ed_split_f32_nhwc", nbytes=x.numel() * (4.0 + 6.0 * u * u))
    _LAUNCH["device"] = x.device
    _call("ed_split_f32_nhwc", x.data_ptr(), out.data_ptr(), N, C, H, W, int(bool(upsample2x)),
          None if absmax is None else absmax.data_ptr(), _stream())
    return out


def split_conv_weight(w):
    """fp32 Conv2d weight [N,Cin,3,3] -> (fp16 channels_last [N,3Cin,3,3] = [wh | wh | wl] of 2^k w, 2^-k): the B operand of
    ``conv3x3_f32out`` for an A operand [xh | xl | xh].  2^k puts max |w| in [2^13, 2^14), so wl = fp16(2^k w - wh) stays out of
    fp16's subnormal range for every weight above 2^-24 of the largest (exact: a power of two)."""
    import math
    wmax = float(w.detach().abs().max())
    k = 0 if not (wmax > 0.0 and math.isfinite(wmax)) else max(-24, min(24, 13 - math.frexp(wmax)[1] + 1))
    ws = w.detach().float() * (2.0 ** k)
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return torch.cat([hi, hi, lo], dim=1).contiguous(memory_format=torch.channels_last), 2.0 ** -k


def conv3x3_f32out_ok(B, H, W, Cin3, N):
    M = B * H * W
    return Cin3 % 64 == 0 and N % 8 == 0 and M * Cin3 * 2 < 2 ** 31 - 16 and N * 9 * Cin3 * 2 < 2 ** 31 - 16 and M < 2 ** 31


def conv3x3_f32out(a, w, bias=None, residual=None, out_scale=1.0, act_absmax=None):
    """a [B,Cin',H,W] fp16 and w [N,Cin',3,3] fp16 in channels_last memory (split operands: Cin' = 3 Cin, ``groupnorm_nhwc_f32(split=True)``
    / ``split_conv_weight``) -> out_scale * conv2d(a, w, stride 1, padding 1) + bias + residual as fp32 channels_last [B,N,H,W]; bias fp32
    [N], residual fp32 channels_last.  ``act_absmax``: the tensor ``split_f32`` scaled ``a`` by (the result is multiplied by 2^e).
    See ed_conv3x3_nhwc_f32out."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dim() == 4 and a.dtype == torch.float16):
        _reject("conv3x3_f32out: a must be an fp16 [B,C,H,W] tensor on the MI355X; no CPU fallback")
    B, C3, H, W = a.shape
    N = w.shape[0]
    cl = torch.channels_last
    if tuple(w.shape) != (N, C3, 3, 3) or w.dtype != torch.float16 or not conv3x3_f32out_ok(B, H, W, C3, N):
        _reject(f"conv3x3_f32out: unsupported shape a {tuple(a.shape)} w {tuple(w.shape)}")
    if not a.is_contiguous(memory_format=cl) or not w.is_contiguous(memory_format=cl):
        _reject("conv3x3_f32out: a and w must be channels_last")
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=a.device, memory_format=cl)
    if residual is not None and (residual.shape != out.shape or residual.dtype != torch.float32 or not residual.is_contiguous(memory_format=cl)):
        _reject("conv3x3_f32out: residual must be an fp32 channels_last tensor of the output's shape")
    TIMER.note_work("ed_conv3x3_nhwc_f32out", flops=2.0 * B * H * W * 9 * C3 * N,
                    nbytes=2.0 * (B * H * W * C3 + 9 * C3 * N) + 4.0 * B * H * W * N * (2 if residual is not None else 1))
    _call("ed_conv3x3_nhwc_f32out", a.data_ptr(), w.data_ptr(), _opt(bias, torch.float32, "bias"),
          None if residual is None else residual.data_ptr(), out.data_ptr(), _DTYPE[torch.float16], B, H, W, C3, N, float(out_scale),
          None if act_absmax is None else act_absmax.data_ptr(), _stream_of(a))
    return out


def conv3x3_f32out_s2_ok(B, Hi, Wi, Cin3, N):
    """can ed_conv3x3_nhwc_f32out_s2 take a split operand [B, Cin3, Hi, Wi] (the INPUT size)?"""
    return (Hi % 2 == 0 and Wi % 2 == 0 and Cin3 % 64 == 0 and N % 8 == 0 and B * Hi * Wi * Cin3 * 2 < 2 ** 31 - 16
            and N * 9 * Cin3 * 2 < 2 ** 31 - 16)


def conv3x3_f32out_s2(a, w, bias=None, out_scale=1.0, act_absmax=None):
    """a [B,Cin',2H,2W] fp16 split operand (``split_f32`` of the raw fp32 stream) and w [N,Cin',3,3] fp16 (``split_conv_weight``), channels_last ->
    out_scale * conv2d(F.pad(a, (0, 1, 0, 1)), w, stride 2) + bias as fp32 channels_last [B,N,H,W]: the VAE encoder's Downsample2D at fp32
    accuracy on the MFMA pipe.  See ed_conv3x3_nhwc_f32out_s2."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dim() == 4 and a.dtype == torch.float16):
        _reject("conv3x3_f32out_s2: a must be an fp16 [B,C,H,W] tensor on the MI355X; no CPU fallback")
    B, C3, Hi, Wi = a.shape
    N = w.shape[0]
    cl = torch.channels_last
    if tuple(w.shape) != (N, C3, 3, 3) or w.dtype != torch.float16 or not conv3x3_f32out_s2_ok(B, Hi, Wi, C3, N):
        _reject(f"conv3x3_f32out_s2: unsupported shape a {tuple(a.shape)} w {tuple(w.shape)}")
    if not a.is_contiguous(memory_format=cl) or not w.is_contiguous(memory_format=cl):
        _reject("conv3x3_f32out_s2: a and w must be channels_last")
    H, W = Hi // 2, Wi // 2
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=a.device, memory_format=cl)
    TIMER.note_work("ed_conv3x3_nhwc_f32out_s2", flops=2.0 * B * H * W * 9 * C3 * N, nbytes=2.0 * (B * Hi * Wi * C3 + 9 * C3 * N) + 4.0 * B * H * W * N)
    _call("ed_conv3x3_nhwc_f32out_s2", a.data_ptr(), w.data_ptr(), _opt(bias, torch.float32, "bias"), out.data_ptr(), _DTYPE[torch.float16],
          B, H, W, C3, N, float(out_scale), None if act_absmax is None else act_absmax.data_ptr(), _stream_of(a))
    return out


def softmax_rows_(x, scale=1.0, bias=None):
    """x fp32 [..., cols] contiguous -> softmax(scale * x [+ bias]) over the last dim, IN PLACE (ed_softmax_rows; with the optional
    fp32 ``bias`` [cols], one value per column, ed_softmax_rows_bias)."""
    cols = x.shape[-1]
    if cols % 4 and x.numel() != cols:
        _reject("softmax_rows_: cols must be a multiple of 4")
    if bias is None:
        TIMER.note_work("ed_softmax_rows", nbytes=3.0 * x.numel() * 4)
        _call("ed_softmax_rows", _dev(x, torch.float32, "x"), x.numel() // cols, cols, float(scale), _stream())
        return x
    if tuple(bias.shape) != (cols,):
        _reject(f"softmax_rows_: bias must have shape ({cols},), got {tuple(bias.shape)}")
    TIMER.note_work("ed_softmax_rows_bias", nbytes=3.0 * x.numel() * 4)
    _call("ed_softmax_rows_bias", _dev(x, torch.float32, "x"), x.numel() // cols, cols, float(scale), _dev(bias, torch.float32, "bias"),
          _stream())
    return x


VAE_ATTENTION_CHUNK_BYTES = 1 << 30  # score-matrix bytes materialised at a time by vae_attention (a few thousand rows keep the GEMMs efficient)


def vae_attention(q, k, v, key_bias=None):
    """softmax(q k^T / sqrt(C) [+ key_bias]) v for the VAE's single-head attention, fp32 [B, N, C]: two library fp32 GEMMs around
    ed_softmax_rows, over chunks of query rows so that the [rows, N] score block stays under VAE_ATTENTION_CHUNK_BYTES
    (N = 32768 tokens for the 1024x2048 decode: 4.3 GB of scores per sample).  Replaces SDPA / AOTriton.  ``key_bias`` fp32 [N]:
    the log multiplicity of every key (the narrowed constant-image encode), added to each chunk's scores by ed_softmax_rows_bias."""
    B, N, C = q.shape
    scale = C ** -0.5
    # rows per chunk: the [B, rows, N] fp32 score block stays under the cap for any B (at least 64 rows)
    rows = max(64, min(N, VAE_ATTENTION_CHUNK_BYTES // (4 * N * B) // 64 * 64)) if N > 256 else N
    kt = k.transpose(1, 2)
    if rows >= N:
        return torch.bmm(softmax_rows_(torch.bmm(q, kt), scale, key_bias), v)
    out = torch.empty_like(q)
    for a in range(0, N, rows):
        s = torch.bmm(q[:, a:a + rows], kt)                      # [B, rows, N]
        out[:, a:a + rows] = torch.bmm(softmax_rows_(s, scale, key_bias), v)
    return out


# kernel variant (identical results): bit 0 = V staging (0: ds_read_b64_tr_b16 from a row-major V tile, 1: V^T tile in
# LDS); bit 1 = 64 query rows per wave (256 per workgroup) instead of 32.  None = choose per shape: the 64-row variant is
# faster only when there is enough work to fill the chip with half as many workgroups (measured, batch 20: N=4096
# 848 vs 776 TFLOP/s; N=1024 and the 77-key cross attention: no gain or slower; profiles/r2_s7_probe_attn.jsonl)
# Round 3: 4 = software-pipelined self-attention kernel, 5 = the same with the lazy row maximum (no per-tile max after the
# first tile; exact redo when a lane's sum of numerators exceeds 2^6), 8 = small-KV kernel (Nk <= 160: the 77-token cross
# attention; two prompt chunks where _stream_two_chunks says so).  Round 4: 6 = 5 on exponent-domain queries (the caller folds scale * log2 e into q -- models.Attention folds it
# into the query projection weights -- and the reference maximum rides in the MFMA accumulator's initial value, so a
# numerator is one v_exp_f32: 157 instead of 189 (lazy) / 214 (exact) instructions per 64-key tile and wave).
FLASH_V_PATH = None
FLASH_HEAD_DIMS = (40, 64, 80, 160)   # 64: SDXL / SD 2.x (all the variants above); 40 / 80 / 160: SD 1.x's 8 heads (k_flash_attn_gen)
# Measured inside the SDXL UNet forward on the MI355X (profiles/r4_s2_unet_forward_ab.txt, batch 20 / 6, all other kernels
# equal): v_path 4 155.2 / 56.5 ms, v_path 5 154.0 / 56.0 ms, v_path 6 155.3 / 56.4 ms.  Removing 12 % (5) and a further 17 % (6)
# of the loop's instructions moves the forward by < 1 %: the kernel is NOT instruction-issue-bound as round 3 concluded from
# SQ_ACTIVE_INST_ANY -- every wave re-reads the whole K and V tile from LDS for its 32 query rows (16 KiB per 16 MFMAs), which
# no variant changes.  5 is the default; 6 stays selectable (FLASH_EXP2 / ED_FLASH_VARIANT=6) and tested.
FLASH_EXP2 = False   # self-attention through v_path 6 where the pipelined kernel applies (see flash_prescale)
_ENV_VARIANT = __import__("os").environ.get("ED_FLASH_VARIANT")  # A/B: "legacy" = the round-2 choice, or a variant number
LOG2E = 1.4426950408889634


def _pipe_fits(Nk, row_stride):
    """The pipelined kernels address K / V with 32-bit byte offsets and want at least two full tiles."""
    return Nk >= 128 and (Nk + 128) * row_stride * 2 < 2 ** 31


def flash_prescale(Nq, Nk, row_stride, scale=0.125):
    """-> the factor a caller must fold into q (softmax scale * log2 e) to run the exponent-domain kernel (v_path 6) for
    a self-attention of this shape, or None when that kernel does not apply (then q stays as it is).  ``row_stride``:
    elements between consecutive tokens of k / v (3 * inner for slices of a fused QKV projection)."""
    if FLASH_V_PATH is not None:
        want = int(FLASH_V_PATH)
    elif _ENV_VARIANT is not None:
        want = -1 if _ENV_VARIANT == "legacy" else int(_ENV_VARIANT)
    else:
        want = 6 if FLASH_EXP2 else -1
    return scale * LOG2E if (want == 6 and _pipe_fits(Nk, row_stride)) else None


def _flash_variant(B, heads, Nq, Nk, k=None, v=None, prescaled=False):
    fits = k is None or _pipe_fits(Nk, max(k.stride(1), v.stride(1)))
    if prescaled:
        if not (Nk >= 128 and fits):
            _reject("flash_attention: exponent-domain q needs the pipelined kernel (Nk >= 128, 32-bit K / V offsets)")
        return 6
    if FLASH_V_PATH is not None and int(FLASH_V_PATH) != 6:
        return int(FLASH_V_PATH)
    legacy = 2 if (Nq >= 2048 and Nk >= 1024 and B * heads * (Nq // 256) >= 1024) else 0
    if _ENV_VARIANT == "legacy":
        return legacy
    if _ENV_VARIANT is not None and int(_ENV_VARIANT) != 6:
        want = int(_ENV_VARIANT)
        if want in (4, 5, 7, 9, 10):
            return want if (Nk >= 128 and fits) else (8 if Nk <= 96 else legacy)
        return want if (want != 8 or Nk <= SMALLKV_MAX_KEYS) else legacy
    if Nk <= 96 or _stream_two_chunks(Nq, Nk):
        return 8
    if Nk >= 128 and fits:
        return FLASH_DEFAULT_PIPE
    return legacy


SMALLKV_MAX_KEYS = 160   # v_path 8: five blocks of 32 keys at the most (ed_flash_attention rejects more)


def _stream_two_chunks(Nq, Nk):
    """Cross attention on a prompt of two 77-token chunks (154 keys) through the streaming kernel instead of the pipelined
    one?  Read off profiles/xattn_long_prompt_timing.json, as a rule on (Nq, Nk) alone: at
    Nq = 4096 the five-block kernel is ahead at 20 and at 40 rows, at Nq = 1024 it loses at 20 rows."""
    return 128 <= Nk <= SMALLKV_MAX_KEYS and Nq >= 4096


FLASH_DEFAULT_PIPE = 5   # pipelined variant for natural-domain q (4 exact / 5 lazy maximum: +0.4-0.8 % on the forward, profiles/r4_s1_attention_variant_in_unet.txt)


def flash_attention(q, k, v, heads, v_path=None, prescaled=False):
    """q [B,Nq,H*d], k / v [B,Nk,H*d] 16-bit, d = head dim in FLASH_HEAD_DIMS (last dim contiguous; batch / token strides free,
    so column slices of a fused QKV projection are fine) -> softmax(q k^T / sqrt(d)) v as a contiguous [B,Nq,H*d] tensor.  ``prescaled``: q already
    carries the factor ``flash_prescale`` returned (exponent-domain kernel, v_path 6).  See ed_flash_attention."""
    B, Nq, HD = q.shape
    Nk = k.shape[1]
    hd = HD // heads
    if HD != heads * hd or hd not in FLASH_HEAD_DIMS or k.shape != (B, Nk, HD) or v.shape != (B, Nk, HD):
        _reject(f"flash_attention: head_dim must be one of {FLASH_HEAD_DIMS} and shapes consistent (q {tuple(q.shape)}, "
                f"k {tuple(k.shape)}, v {tuple(v.shape)}, heads {heads})")
    if hd != 64 and (prescaled or v_path is not None):
        _reject("flash_attention: kernel variants exist for head_dim 64 only")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != q.dtype or t.stride(2) != 1:
            _reject(f"flash_attention: {name} must be a 16-bit tensor on the MI355X with unit last stride; no CPU fallback")
        if _LAUNCH["device"] is None:
            _LAUNCH["device"] = t.device
        elif _LAUNCH["device"] != t.device:
            _reject(f"flash_attention: {name} lives on {t.device}, q on {_LAUNCH['device']}")
    if v_path is not None and (int(v_path) == 6) != bool(prescaled):
        _reject("flash_attention: v_path 6 takes exponent-domain q (prescaled=True) and nothing else does")
    out = torch.empty(B, Nq, HD, dtype=q.dtype, device=q.device)
    # algorithmic work: QK^T and PV contractions (4 B H Nq Nk 64 flop); q, k, v read once, out written once
    TIMER.note_work("ed_flash_attention", flops=4.0 * B * heads * Nq * Nk * hd,
                    nbytes=2.0 * q.element_size() * HD * B * (Nq + Nk))
    variant = 0 if hd != 64 else (_flash_variant(B, heads, Nq, Nk, k, v, prescaled) if v_path is None else int(v_path))
    _call("ed_flash_attention", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _code(q, "q"), B, heads, Nq, Nk,
          hd, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
          hd ** -0.5, variant, _stream())
    return out


IP_MAX_TEXT_KEYS = SMALLKV_MAX_KEYS   # ed_flash_attention_ip: five text blocks of 32 keys ...
IP_MAX_IMAGE_KEYS = 32                # ... and one image block


def flash_attention_ip_ok(head_dim, n_text, n_image):
    """does ed_flash_attention_ip take this shape?  (models.Attention runs two attentions and a torch axpy otherwise)"""
    return head_dim == 64 and 1 <= n_text <= IP_MAX_TEXT_KEYS and 1 <= n_image <= IP_MAX_IMAGE_KEYS


def flash_attention_ip(q, k, v, heads, n_text, ip_scale):
    """IP-Adapter decoupled cross attention in one launch: q [B,Nq,H*64], k / v [B,Nt+Ni,H*64] 16-bit with
    the ``n_text`` = Nt text rows first and the Ni image rows (``to_k_ip`` / ``to_v_ip`` of the image tokens) behind them; strides
    as ``flash_attention`` -> softmax(q k_t^T / 8) v_t + ip_scale * softmax(q k_i^T / 8) v_i, contiguous [B,Nq,H*64].
    1 <= Nt <= 160, 1 <= Ni <= 32, head dim 64.  See ed_flash_attention_ip."""
    B, Nq, HD = q.shape
    N = k.shape[1]
    hd = HD // heads
    n_text, ip_scale = int(n_text), float(ip_scale)
    if HD != heads * hd or hd != 64 or k.shape != (B, N, HD) or v.shape != (B, N, HD):
        _reject(f"flash_attention_ip: head_dim must be 64 and shapes consistent (q {tuple(q.shape)}, k {tuple(k.shape)}, "
                f"v {tuple(v.shape)}, heads {heads})")
    if not flash_attention_ip_ok(hd, n_text, N - n_text):
        _reject(f"flash_attention_ip: needs 1 <= text keys <= {IP_MAX_TEXT_KEYS} and 1 <= image keys <= {IP_MAX_IMAGE_KEYS}, "
                f"got {n_text} and {N - n_text}")
    if ip_scale != ip_scale or ip_scale in (float("inf"), float("-inf")):
        _reject(f"flash_attention_ip: ip_scale must be finite, got {ip_scale}")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != q.dtype or t.dtype not in (torch.float16, torch.bfloat16) or t.stride(2) != 1:
            _reject(f"flash_attention_ip: {name} must be a 16-bit tensor on the MI355X with unit last stride; no CPU fallback")
        if _LAUNCH["device"] is None:
            _LAUNCH["device"] = t.device
        elif _LAUNCH["device"] != t.device:
            _reject(f"flash_attention_ip: {name} lives on {t.device}, q on {_LAUNCH['device']}")
    out = torch.empty(B, Nq, HD, dtype=q.dtype, device=q.device)
    TIMER.note_work("ed_flash_attention_ip", flops=4.0 * B * heads * Nq * N * hd,
                    nbytes=2.0 * q.element_size() * HD * B * (Nq + N))
    _call("ed_flash_attention_ip", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _code(q, "q"), B, heads, Nq, n_text,
          N - n_text, hd, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
          hd ** -0.5, ip_scale, _stream())
    return out


IPN_MAX_ADAPTERS = 4                  # ed_flash_attention_ipn: up to four segments inside the one image block


def flash_attention_ipn_ok(head_dim, n_text, n_image):
    """does ed_flash_attention_ipn take this shape?  ``n_image``: one key count per adapter.  (models.Attention runs A + 1
    attentions and A weighted adds otherwise)"""
    n_image = tuple(int(n) for n in n_image)
    return (head_dim == 64 and 1 <= n_text <= IP_MAX_TEXT_KEYS and 1 <= len(n_image) <= IPN_MAX_ADAPTERS
            and all(n >= 1 for n in n_image) and sum(n_image) <= IP_MAX_IMAGE_KEYS)


def flash_attention_ipn(q, k, v, heads, n_text, n_image, w):
    """Decoupled cross attention with several IP-Adapters in one launch: q [B,Nq,H*64], k / v
    [B,Nt+sum(n_image),H*64] 16-bit with the ``n_text`` text rows first, then each adapter's ``n_image[a]`` rows in order; ``w`` a
    float32 DEVICE tensor [A] the kernel reads when it runs (so a captured graph replays a change of weights) ->
    softmax(q k_t^T / 8) v_t + sum_a w[a] softmax(q k_a^T / 8) v_a, contiguous [B,Nq,H*64].  1 <= Nt <= 160, 1 <= A <= 4,
    sum(n_image) <= 32, head dim 64.  See ed_flash_attention_ipn."""
    B, Nq, HD = q.shape
    N = k.shape[1]
    hd = HD // heads
    n_text, n_image = int(n_text), tuple(int(n) for n in n_image)
    if HD != heads * hd or hd != 64 or k.shape != (B, N, HD) or v.shape != (B, N, HD):
        _reject(f"flash_attention_ipn: head_dim must be 64 and shapes consistent (q {tuple(q.shape)}, k {tuple(k.shape)}, "
                f"v {tuple(v.shape)}, heads {heads})")
    if not flash_attention_ipn_ok(hd, n_text, n_image) or n_text + sum(n_image) != N:
        _reject(f"flash_attention_ipn: needs 1 <= text keys <= {IP_MAX_TEXT_KEYS}, 1 to {IPN_MAX_ADAPTERS} adapters of >= 1 image keys "
                f"each, <= {IP_MAX_IMAGE_KEYS} image keys together and text + image keys = {N} rows, got {n_text} and {n_image}")
    if (not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.shape != (len(n_image),)
            or not w.is_contiguous()):
        _reject(f"flash_attention_ipn: w must be a contiguous float32 tensor [{len(n_image)}] on the MI355X (one weight per adapter)")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != q.dtype or t.dtype not in (torch.float16, torch.bfloat16) or t.stride(2) != 1:
            _reject(f"flash_attention_ipn: {name} must be a 16-bit tensor on the MI355X with unit last stride; no CPU fallback")
        if _LAUNCH["device"] is None:
            _LAUNCH["device"] = t.device
        elif _LAUNCH["device"] != t.device:
            _reject(f"flash_attention_ipn: {name} lives on {t.device}, q on {_LAUNCH['device']}")
    if w.device != q.device:
        _reject(f"flash_attention_ipn: w lives on {w.device}, q on {q.device}")
    out = torch.empty(B, Nq, HD, dtype=q.dtype, device=q.device)
    TIMER.note_work("ed_flash_attention_ipn", flops=4.0 * B * heads * Nq * N * hd,
                    nbytes=2.0 * q.element_size() * HD * B * (Nq + N))
    ni = (ctypes.c_int32 * len(n_image))(*n_image)   # read by the entry point before it returns
    _call("ed_flash_attention_ipn", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _code(q, "q"), B, heads, Nq, n_text,
          len(n_image), ctypes.addressof(ni), hd, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
          out.stride(0), out.stride(1), hd ** -0.5, w.data_ptr(), _stream())
    return out


def flash_attention_ipm_ok(head_dim, n_text, n_image):
    """does ed_flash_attention_ipm take this shape?  ed_flash_attention_ipn's range (the mask changes one coefficient per row and
    segment); models.Attention runs A + 1 attentions and A masked, weighted adds otherwise."""
    return flash_attention_ipn_ok(head_dim, n_text, n_image)


def flash_attention_ipm(q, k, v, heads, n_text, n_image, w, m):
    """``flash_attention_ipn`` with IP-Adapter attention masks: ``m`` a float32 DEVICE tensor [B,A,Nq], or
    [1,A,Nq] / [A,Nq] shared by the batch, unit last stride, any batch / adapter strides (a level of ``ip_mask_rows``' buffer is
    such a view), read when the kernel runs ->
    softmax(q k_t^T / 8) v_t + sum_a (w[a] m[b,a,i]) softmax(q k_a^T / 8) v_a, contiguous [B,Nq,H*64].  See ed_flash_attention_ipm."""
    B, Nq, HD = q.shape
    N = k.shape[1]
    hd = HD // heads
    n_text, n_image = int(n_text), tuple(int(n) for n in n_image)
    A = len(n_image)
    if HD != heads * hd or hd != 64 or k.shape != (B, N, HD) or v.shape != (B, N, HD):
        _reject(f"flash_attention_ipm: head_dim must be 64 and shapes consistent (q {tuple(q.shape)}, k {tuple(k.shape)}, "
                f"v {tuple(v.shape)}, heads {heads})")
    if not flash_attention_ipm_ok(hd, n_text, n_image) or n_text + sum(n_image) != N:
        _reject(f"flash_attention_ipm: needs 1 <= text keys <= {IP_MAX_TEXT_KEYS}, 1 to {IPN_MAX_ADAPTERS} adapters of >= 1 image keys "
                f"each, <= {IP_MAX_IMAGE_KEYS} image keys together and text + image keys = {N} rows, got {n_text} and {n_image}")
    if (not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.shape != (A,) or not w.is_contiguous()):
        _reject(f"flash_attention_ipm: w must be a contiguous float32 tensor [{A}] on the MI355X (one weight per adapter)")
    if isinstance(m, torch.Tensor) and m.dim() == 2:
        m = m[None]
    if (not isinstance(m, torch.Tensor) or not m.is_cuda or m.dtype != torch.float32 or m.dim() != 3 or m.shape[0] not in (1, B)
            or tuple(m.shape[1:]) != (A, Nq) or (Nq > 1 and m.stride(2) != 1) or (A > 1 and m.stride(1) < Nq)
            or (m.shape[0] > 1 and m.stride(0) < 0)):
        _reject(f"flash_attention_ipm: m must be a float32 tensor [{B} or 1,{A},{Nq}] on the MI355X with unit last stride, got "
                f"{tuple(getattr(m, 'shape', ()))} / {getattr(m, 'dtype', None)}")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != q.dtype or t.dtype not in (torch.float16, torch.bfloat16) or t.stride(2) != 1:
            _reject(f"flash_attention_ipm: {name} must be a 16-bit tensor on the MI355X with unit last stride; no CPU fallback")
        if _LAUNCH["device"] is None:
            _LAUNCH["device"] = t.device
        elif _LAUNCH["device"] != t.device:
            _reject(f"flash_attention_ipm: {name} lives on {t.device}, q on {_LAUNCH['device']}")
    if w.device != q.device or m.device != q.device:
        _reject(f"flash_attention_ipm: w lives on {w.device}, m on {m.device}, q on {q.device}")
    m_sb = 0 if m.shape[0] == 1 else m.stride(0)
    m_sa = max(m.stride(1), Nq) if A > 1 else Nq   # one adapter: the stride is never applied
    out = torch.empty(B, Nq, HD, dtype=q.dtype, device=q.device)
    TIMER.note_work("ed_flash_attention_ipm", flops=4.0 * B * heads * Nq * N * hd,
                    nbytes=2.0 * q.element_size() * HD * B * (Nq + N) + 4.0 * m.shape[0] * A * Nq)
    ni = (ctypes.c_int32 * A)(*n_image)   # read by the entry point before it returns
    _call("ed_flash_attention_ipm", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _code(q, "q"), B, heads, Nq, n_text,
          A, ctypes.addressof(ni), hd, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
          out.stride(0), out.stride(1), hd ** -0.5, w.data_ptr(), m.data_ptr(), m_sb, m_sa, _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Canny condition extraction (csrc/canny_kernels.hip): pre-processing of one image before the loop, never graph-captured
# ---------------------------------------------------------------------------------------------------------------------
CANNY_MAX_DIM = 8192


def _canny_dims(t, name, channels):
    """(H, W, C) of a uint8 image tensor [H,W,C] / [H,W] (``channels``: the allowed C), rejected outside the kernels' bounds."""
    if t.dim() == 2 and 1 in channels:
        H, W, C = t.shape[0], t.shape[1], 1
    elif t.dim() == 3 and t.shape[2] in channels:
        H, W, C = t.shape
    else:
        _reject(f"{name} must be uint8 [H,W,C] with C in {sorted(channels)}{' or [H,W]' if 1 in channels else ''}, got {tuple(t.shape)}")
    if not (1 <= H <= CANNY_MAX_DIM and 1 <= W <= CANNY_MAX_DIM):
        _reject(f"{name}: H and W must be in 1..{CANNY_MAX_DIM}, got {H} x {W}")
    return H, W, C


def _canny_threshold(v, name):
    import math
    if not math.isfinite(v):
        _reject(f"canny: {name} threshold must be finite, got {v}")
    return max(-2 ** 31, min(2 ** 31 - 1, int(math.floor(v))))


def canny_map(img, low=100, high=200):
    """img uint8 [H,W,C] (C = 1 or 3; [H,W] = one channel), HWC contiguous -> uint8 map [H,W]: 1 = not an edge, 0 = candidate,
    2 = strong (OpenCV's coding).  Thresholds are floored, and swapped when low > high.  See ed_canny_map."""
    p_img = _dev(img, torch.uint8, "img")
    H, W, C = _canny_dims(img, "img", (1, 3))
    lo, hi = _canny_threshold(low, "low"), _canny_threshold(high, "high")
    cmap = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    TIMER.note_work("ed_canny_map", nbytes=float(H * W * (C + 1)))
    _call("ed_canny_map", p_img, H, W, C, lo, hi, _dev(cmap, torch.uint8, "map"), _stream())
    return cmap


def canny_hysteresis(cmap):
    """In place on a uint8 map [H,W]: candidates (0) that are 8-connected through candidates to a strong pixel (2) become 2.
    -> (cmap, global passes).  Synchronises the stream once per pass (see ed_canny_hysteresis): not for graph capture."""
    import ctypes
    p_map = _dev(cmap, torch.uint8, "map")
    H, W, _ = _canny_dims(cmap, "map", (1,))
    if cmap.dim() != 2:
        _reject(f"map must be [H,W], got {tuple(cmap.shape)}")
    if torch.cuda.is_current_stream_capturing():
        _reject("canny_hysteresis reads a device flag between passes and cannot be captured into a graph")
    ws = torch.empty(_hip.lib().ed_canny_workspace(H, W, 1) // 4, dtype=torch.int32, device=cmap.device)
    passes = ctypes.c_int32(0)
    TIMER.note_work("ed_canny_hysteresis", nbytes=float(H * W))    # per pass: the map is read once, promoted bytes written
    _call("ed_canny_hysteresis", p_map, H, W, _dev(ws, torch.int32, "workspace"), ctypes.addressof(passes), _stream())
    return cmap, int(passes.value)


def canny_edges(cmap, out="u8"):
    """uint8 map [H,W] -> ``out="u8"``: uint8 [H,W,3], 255 where the map is 2, else 0; ``out="cond"``: fp32 [1,3,H,W] with 1.0 / 0.0
    (the ControlNet condition tensor of that image).  See ed_canny_edges."""
    if out not in ("u8", "cond"):
        raise ValueError(f"out must be 'u8' or 'cond', got {out!r}")
    p_map = _dev(cmap, torch.uint8, "map")
    H, W, _ = _canny_dims(cmap, "map", (1,))
    if cmap.dim() != 2:
        _reject(f"map must be [H,W], got {tuple(cmap.shape)}")
    if out == "u8":
        res = torch.empty((H, W, 3), dtype=torch.uint8, device=cmap.device)
        TIMER.note_work("ed_canny_edges", nbytes=float(4 * H * W))
        _call("ed_canny_edges", p_map, H, W, _dev(res, torch.uint8, "edges"), None, _stream())
    else:
        res = torch.empty((1, 3, H, W), dtype=torch.float32, device=cmap.device)
        TIMER.note_work("ed_canny_edges", nbytes=float(13 * H * W))
        _call("ed_canny_edges", p_map, H, W, None, _dev(res, torch.float32, "cond"), _stream())
    return res


def canny(img, low=100, high=200, out="u8"):
    """cv2.Canny(img, low, high) (aperture 3, L1 gradient) of a uint8 HWC image on the device, replicated to three channels:
    ``out="u8"`` -> uint8 [H,W,3] (255 / 0), ``out="cond"`` -> fp32 [1,3,H,W] (1.0 / 0.0).  EDC:1105-1108."""
    if out not in ("u8", "cond"):
        raise ValueError(f"out must be 'u8' or 'cond', got {out!r}")
    cmap, _ = canny_hysteresis(canny_map(img, low, high))
    return canny_edges(cmap, out)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow-exact resize of 8-bit images (csrc/resize_kernels.hip): the condition image before the loop, never graph-captured
# ---------------------------------------------------------------------------------------------------------------------
RESIZE_MAX_DIM = 8192
_RESIZE_TABLES = {}


def _resize_tables(device, key, make):
    """Device copies of one axis' (coeff int32 [out, ksize], bounds int32 [out, 2]), cached per device and ``key``."""
    hit = _RESIZE_TABLES.get((device, key))
    if hit is None:
        if len(_RESIZE_TABLES) >= 64:
            _RESIZE_TABLES.clear()
        coeff, bounds = make()
        hit = (torch.from_numpy(coeff.copy()).to(device), torch.from_numpy(bounds.copy()).to(device))
        _RESIZE_TABLES[(device, key)] = hit
    return hit


def _identity_tables(n):
    import numpy as np
    from . import resample
    coeff = np.full((n, 1), 1 << resample.PRECISION_BITS, np.int32)     # (2^21 + v 2^22) >> 22 == v
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], axis=1)
    return coeff, bounds


def resize_u8(img, size, filter="bicubic", out="u8"):
    """``PIL.Image.resize((W_out, H_out), BICUBIC | LANCZOS)`` of an L / RGB image, bit for bit, on the device.

    img uint8 [H,W,C] (C = 1 or 3) or [H,W], contiguous; ``size = (H_out, W_out)``.  ``out="u8"`` -> uint8 of the input's rank;
    ``out="cond"`` -> fp32 [1,3,H_out,W_out] = bytes / 255 (one channel replicated), the ControlNet condition tensor of that image.
    Horizontal pass (ed_resize_rows_u8) into a uint8 intermediate, then vertical pass (ed_resize_cols_u8); a pass whose size does
    not change is skipped.  See include/elastic_hip.h and resample.py."""
    from . import resample
    if out not in ("u8", "cond"):
        raise ValueError(f"out must be 'u8' or 'cond', got {out!r}")
    if filter not in resample.FILTERS:
        raise ValueError(f"filter must be one of {sorted(resample.FILTERS)}, got {filter!r}")
    p_img = _dev(img, torch.uint8, "img")
    H, W, C = _canny_dims(img, "img", (1, 3))
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        _reject(f"size must be (H_out, W_out), got {size!r}")
    if not (1 <= Ho <= RESIZE_MAX_DIM and 1 <= Wo <= RESIZE_MAX_DIM):
        _reject(f"size: H_out and W_out must be in 1..{RESIZE_MAX_DIM}, got {Ho} x {Wo}")
    dev = img.device
    if (Ho, Wo) == (H, W) and out == "u8":
        _LAUNCH["device"] = None
        return img.clone()
    passes = resample.plan((H, W), (Ho, Wo), filter)
    src, rows, pitch = p_img, H, W * C
    mid = None
    if passes and passes[0][0] == "rows":
        _, kh, _, y0, y1 = passes[0]
        coeff, bounds = _resize_tables(dev, (W, Wo, filter), lambda: resample.coefficients(W, Wo, filter))
        rows, mid_pitch = y1 - y0, (Wo * C + 3) // 4 * 4
        mid = torch.empty((rows, mid_pitch), dtype=torch.uint8, device=dev)
        TIMER.note_work("ed_resize_rows_u8", flops=2.0 * rows * Wo * C * kh.shape[1], nbytes=float(rows * (W * C + mid_pitch)))
        _call("ed_resize_rows_u8", p_img + y0 * pitch, rows, W, C, pitch, _dev(coeff, torch.int32, "coeff"),
              _dev(bounds, torch.int32, "bounds"), kh.shape[1], Wo, _dev(mid, torch.uint8, "intermediate"), mid_pitch, _stream())
        src, pitch = _dev(mid, torch.uint8, "intermediate"), mid_pitch
    if passes and passes[-1][0] == "cols":
        _, kv, bv = passes[-1]
        shift = int(bv[0, 0]) if len(passes) == 2 else None            # two passes: bounds are relative to the intermediate's first row
        coeff, bounds = _resize_tables(dev, (H, Ho, filter, shift), lambda: (kv, bv))
        ksz = kv.shape[1]
    else:                                                               # width only (or a plain copy into "cond"): one tap of weight 1
        coeff, bounds = _resize_tables(dev, (Ho, "identity"), lambda: _identity_tables(Ho))
        ksz = 1
    if out == "u8":
        res = torch.empty((Ho, Wo) if img.dim() == 2 else (Ho, Wo, C), dtype=torch.uint8, device=dev)
        p_u8, p_cond = _dev(res, torch.uint8, "out"), None
    else:
        res = torch.empty((1, 3, Ho, Wo), dtype=torch.float32, device=dev)
        p_u8, p_cond = None, _dev(res, torch.float32, "out")
    TIMER.note_work("ed_resize_cols_u8", flops=2.0 * Ho * Wo * C * ksz,
                    nbytes=float(rows * Wo * C + Ho * Wo * (C if out == "u8" else 12)))
    _call("ed_resize_cols_u8", src, rows, Wo * C, pitch, _dev(coeff, torch.int32, "coeff"), _dev(bounds, torch.int32, "bounds"),
          ksz, Ho, C, p_u8, p_cond, _stream())
    return res


# ---------------------------------------------------------------------------------------------------------------------
# Score PCA maps (csrc/pca_kernels.hip): the reference's per-step diagnostic pictures, no host sync
# ---------------------------------------------------------------------------------------------------------------------
def score_pca_workspace(B, n, device=None):
    """The workspace of score_pca for B samples of n = H * W pixels: an f64 tensor, allocate once and reuse (launches on one
    stream)."""
    nbytes = _hip.lib().ed_score_pca_workspace(int(B), int(n))
    if nbytes <= 0:
        _reject(f"score_pca_workspace: B must be >= 1 and n in 4..2^28, got B = {B}, n = {n}")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def score_pca(score, normalize=False, workspace=None, return_fit=False):
    """score f32 [B, 4, H, W] -> uint8 [B, H, W, 3] on the device: every sample's pixels projected onto the first three principal
    components of that sample and scaled to bytes by the projection's own range -- ``sklearn.decomposition.PCA(3).fit / transform``
    + ``np.uint8((r - r.min()) / (r.max() - r.min()) * 255)`` of pca_diffusion_scores.py:165-179, within one byte step (DESIGN.md
    section 26).  ``normalize``: the script's ``(s - min) / (max - min) * 2 - 1`` of the class direction over the whole tensor, in
    fp32 as there, before the fit.  ``return_fit``: also (components f32 [B,3,4], mean f32 [B,4], explained_variance f32 [B,3]).
    Four launches (five with ``normalize``), no sync.
    workspace = score_pca_workspace(B, H * W); allocated here when absent."""
    p_score = _dev(score, torch.float32, "score")
    if score.dim() != 4 or score.shape[1] != 4:
        _reject(f"score_pca: score must be [B, 4, H, W] (a 4-channel latent score), got {tuple(score.shape)}")
    B, C, H, W = score.shape
    need = _hip.lib().ed_score_pca_workspace(B, H * W)
    if B < 1 or H * W < 4 or need <= 0:
        _reject(f"score_pca: needs B >= 1 and 4 <= H * W <= 2^28 pixels to fit three components, got {tuple(score.shape)}")
    dev = score.device
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.numel() * workspace.element_size() < need:
        _reject(f"workspace must hold {need} bytes (score_pca_workspace({B}, {H * W}))")
    comps, mean, var, norm = (torch.empty(B, k, dtype=torch.float32, device=dev) for k in (12, 4, 3, 2))
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    TIMER.note_work("ed_score_pca_fit", flops=28.0 * B * H * W, nbytes=(32.0 if normalize else 16.0) * B * H * W)
    _call("ed_score_pca_fit", p_score, B, C, H, W, int(bool(normalize)), _dev(comps, torch.float32, "components"),
          _dev(mean, torch.float32, "mean"), _dev(var, torch.float32, "explained_variance"), _dev(norm, torch.float32, "norm"),
          _dev(workspace, None, "workspace"), _stream())
    TIMER.note_work("ed_score_pca_map", flops=2 * 28.0 * B * H * W, nbytes=35.0 * B * H * W)
    _call("ed_score_pca_map", _dev(score, torch.float32, "score"), B, C, H, W,
          _dev(norm, torch.float32, "norm") if normalize else None, _dev(out, torch.uint8, "out"),
          _dev(workspace, None, "workspace"), _stream())
    if return_fit:
        return out, (comps.view(B, 3, 4), mean, var)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Image-to-image and masked inpainting: once per image before the loop, the blend once per phase
# ---------------------------------------------------------------------------------------------------------------------
VAE_INPUT_MAX_DIM = 8192


def u8_to_vae_input(img, dtype=torch.float32):
    """img uint8 [H,W,3] (RGB, contiguous) -> [1,3,H,W] of ``dtype`` = 2 * (v / 255) - 1: what ``VaeImageProcessor.preprocess``
    hands the VAE encoder, bit-identical to ``np.float32(v) / 255`` then ``2 * x - 1`` on the CPU.  See ed_u8_to_vae_input."""
    p_img = _dev(img, torch.uint8, "img")
    if img.dim() != 3 or img.shape[2] != 3:
        _reject(f"img must be uint8 [H,W,3], got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    if not (1 <= H <= VAE_INPUT_MAX_DIM and 1 <= W <= VAE_INPUT_MAX_DIM):
        _reject(f"img: H and W must be in 1..{VAE_INPUT_MAX_DIM}, got {H} x {W}")
    if dtype not in _DTYPE:
        _reject(f"u8_to_vae_input: unsupported dtype {dtype}")
    out = torch.empty((1, 3, H, W), dtype=dtype, device=img.device)
    _call("ed_u8_to_vae_input", p_img, H, W, _dev(out, dtype, "out"), _DTYPE[dtype], _stream())
    TIMER.note_work("ed_u8_to_vae_input", nbytes=float(3 * H * W * (1 + out.element_size())))
    return out


def u8_to_vae_input_masked(img, mask, dtype=torch.float32, threshold=128):
    """``u8_to_vae_input`` with the hole blanked: exactly +0.0 where ``mask`` uint8 [H,W] is >= ``threshold``, 2 * (v / 255) - 1
    elsewhere -> [1,3,H,W] of ``dtype``; what the masked-image latent of a 9-channel inpainting UNet is encoded from.
    See ed_u8_to_vae_input_masked."""
    p_img = _dev(img, torch.uint8, "img")
    if img.dim() != 3 or img.shape[2] != 3:
        _reject(f"img must be uint8 [H,W,3], got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    if not (1 <= H <= VAE_INPUT_MAX_DIM and 1 <= W <= VAE_INPUT_MAX_DIM):
        _reject(f"img: H and W must be in 1..{VAE_INPUT_MAX_DIM}, got {H} x {W}")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
        _reject(f"u8_to_vae_input_masked: mask must be uint8 [{H},{W}], got {getattr(mask, 'dtype', type(mask).__name__)} "
                f"{tuple(getattr(mask, 'shape', ()))}")
    threshold = int(threshold)
    if not 1 <= threshold <= 255:
        _reject(f"u8_to_vae_input_masked: threshold must be in 1..255, got {threshold}")
    if dtype not in _DTYPE:
        _reject(f"u8_to_vae_input_masked: unsupported dtype {dtype}")
    out = torch.empty((1, 3, H, W), dtype=dtype, device=img.device)
    _call("ed_u8_to_vae_input_masked", p_img, _dev(mask, torch.uint8, "mask"), threshold, H, W, _dev(out, dtype, "out"),
          _DTYPE[dtype], _stream())
    TIMER.note_work("ed_u8_to_vae_input_masked", nbytes=float(H * W * (4 + 3 * out.element_size())))
    return out


CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)   # transformers' OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_resize_size(H, W, size=224):
    """(H', W') of CLIPImageProcessor's resize: the shortest edge becomes ``size``, the long one int(size * long / short)."""
    short, long = (H, W) if H <= W else (W, H)
    new_long = int(size * long / short)
    return (size, new_long) if H <= W else (new_long, size)


def u8_to_clip_input(img, size=224, mean=CLIP_IMAGE_MEAN, std=CLIP_IMAGE_STD):
    """img uint8 [H,W,3] (RGB, contiguous, both sides >= ``size``: the output of ``resize_u8`` to ``clip_resize_size``) ->
    fp32 [1,3,size,size]: CLIPImageProcessor's centre crop, rescale and normalise in one launch.  See ed_u8_to_clip_input."""
    p_img = _dev(img, torch.uint8, "img")
    if img.dim() != 3 or img.shape[2] != 3:
        _reject(f"img must be uint8 [H,W,3], got {tuple(img.shape)}")
    H, W, size = int(img.shape[0]), int(img.shape[1]), int(size)
    if not (1 <= size <= H <= VAE_INPUT_MAX_DIM and size <= W <= VAE_INPUT_MAX_DIM):
        _reject(f"u8_to_clip_input: needs 1 <= size <= H, W <= {VAE_INPUT_MAX_DIM}, got size {size} and {H} x {W}")
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3 or not all(s > 0 for s in std):
        _reject("u8_to_clip_input: mean and std are three numbers each, std positive")
    y0, x0 = (H - size) // 2, (W - size) // 2   # transformers' center_crop: top = (H - size) // 2, left = (W - size) // 2
    out = torch.empty((1, 3, size, size), dtype=torch.float32, device=img.device)
    _call("ed_u8_to_clip_input", p_img, H, W, y0, x0, size, _dev(out, torch.float32, "out"), *mean, *std, _stream())
    TIMER.note_work("ed_u8_to_clip_input", nbytes=float(3 * size * size * 5))
    return out


def img2img_init(mean, std, eps, noise, sf, a, b, z0=None, x=None):
    """z0 = (mean + std * eps) * sf and x = a * z0 + b * noise in one launch -> (z0, x), both f32 of mean's shape.
    mean / std: the encoder's posterior moments, f32 / f16 / bf16 (one dtype for both); eps / noise f32.  See ed_img2img_init."""
    if not isinstance(mean, torch.Tensor) or not isinstance(std, torch.Tensor):
        _reject("img2img_init: mean / std must be tensors on the MI355X; no CPU fallback")
    shape = tuple(mean.shape)
    for name, t in (("std", std), ("eps", eps), ("noise", noise), ("z0", z0), ("x", x)):
        if t is not None and tuple(getattr(t, "shape", ())) != shape:
            _reject(f"img2img_init: {name} must have mean's shape {shape}, got {tuple(getattr(t, 'shape', ()))}")
    if std.dtype != mean.dtype:
        _reject(f"img2img_init: mean and std must share a dtype, got {mean.dtype} / {std.dtype}")
    code = _code(mean, "mean")
    p_mean, p_std = _dev(mean, None, "mean"), _dev(std, None, "std")
    p_eps, p_noise = _dev(eps, torch.float32, "eps"), _dev(noise, torch.float32, "noise")
    z0 = torch.empty(shape, dtype=torch.float32, device=mean.device) if z0 is None else z0
    x = torch.empty(shape, dtype=torch.float32, device=mean.device) if x is None else x
    n = mean.numel()
    _call("ed_img2img_init", p_mean, p_std, code, p_eps, p_noise, float(sf), float(a), float(b),
          _dev(z0, torch.float32, "z0"), _dev(x, torch.float32, "x"), n, _stream())
    TIMER.note_work("ed_img2img_init", flops=5.0 * n, nbytes=float(n * (2 * mean.element_size() + 16)))
    return z0, x


def mask_to_latent(mask, scale=1, threshold=None):
    """mask uint8 / bool [H,W] (or [H,W,1]) -> uint8 [H // scale, W // scale], 1 = repaint, 0 = keep:
    ``out[y, x] = mask[scale * y, scale * x] >= threshold`` -- torch's nearest ``interpolate`` of the mask binarised at 0.5
    (``threshold`` 128, the default for ``scale`` > 1).  ``scale == 1`` with the default threshold 1 normalises a mask that is
    already at latent resolution (non-zero = repaint).  H and W must be multiples of ``scale``.  See ed_mask_to_latent."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
        _reject(f"mask must be a uint8 or bool tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
    src = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    p_src = _dev(src, torch.uint8, "mask")
    if src.dim() == 3 and src.shape[2] == 1:
        src = src[:, :, 0]
    if src.dim() != 2:
        _reject(f"mask must be [H,W] or [H,W,1], got {tuple(mask.shape)}")
    scale = int(scale)
    H, W = int(src.shape[0]), int(src.shape[1])
    if scale < 1 or H == 0 or W == 0 or H % scale or W % scale:
        _reject(f"mask: {H} x {W} is not a non-empty multiple of scale {scale}")
    threshold = (128 if scale > 1 else 1) if threshold is None else int(threshold)
    if not 1 <= threshold <= 255:
        _reject(f"mask: threshold must be in 1..255, got {threshold}")
    Hl, Wl = H // scale, W // scale
    out = torch.empty((Hl, Wl), dtype=torch.uint8, device=mask.device)
    _call("ed_mask_to_latent", p_src, H, W, scale, threshold, _dev(out, torch.uint8, "out"), Hl, Wl, _stream())
    TIMER.note_work("ed_mask_to_latent", nbytes=2.0 * Hl * Wl)  # algorithmic: one sampled byte in, one out
    return out


def inpaint_blend(x, mask, z0, noise, a, b, out=None, clean=False):
    """out = where(mask, x, known) with known = a * z0 + b * noise, or z0 itself with ``clean`` (``noise`` may then be None).
    x / z0 / noise f32 [B,C,H,W], mask uint8 [H,W] (1 = keep x) broadcast over B and C; ``out`` None = in place into ``x``.
    See ed_inpaint_blend."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        _reject(f"inpaint_blend: x must be an f32 [B,C,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(x, 'shape', ()))})")
    B, C, H, W = x.shape
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8:
        _reject(f"inpaint_blend: mask must be uint8 (ops.mask_to_latent), got {getattr(mask, 'dtype', type(mask).__name__)}")
    if tuple(mask.shape) != (H, W):
        _reject(f"inpaint_blend: mask must be [{H}, {W}], got {tuple(mask.shape)}")
    if noise is None and not clean:
        _reject("inpaint_blend: noise is required unless clean")
    out = x if out is None else out
    for name, t in (("z0", z0), ("noise", noise), ("out", out)):
        if t is not None and tuple(getattr(t, "shape", ())) != tuple(x.shape):
            _reject(f"inpaint_blend: {name} must have x's shape {tuple(x.shape)}, got {tuple(getattr(t, 'shape', ()))}")
    _call("ed_inpaint_blend", _dev(x, torch.float32, "x"), _dev(mask, torch.uint8, "mask"), _dev(z0, torch.float32, "z0"),
          _opt(noise, torch.float32, "noise"), float(a), float(b), int(bool(clean)), _dev(out, torch.float32, "out"),
          B * C, H * W, _stream())
    n = x.numel()
    TIMER.note_work("ed_inpaint_blend", flops=0.0 if clean else 3.0 * n, nbytes=float(n * (12 if clean else 16) + n))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Soft-edged inpainting: the mask blur, the level map and the canvas once per image before the loop,
# the graded blend once per phase, the composite once per image after the decode
# ---------------------------------------------------------------------------------------------------------------------
MASK_BLUR_MAX = 256.0


def gaussian_box_parameters(radius):
    """``PIL.ImageFilter.GaussianBlur(radius)`` -> (r, ww, fw): the box radius and the two 24-bit fixed-point weights of each of
    its three box passes per direction, computed as Pillow computes them (the effective radius rounded to float32, the weight
    of an inside pixel ``uint32(float32(2^24) / (2 * fr + 1))`` evaluated in float32).  Pure host arithmetic."""
    import math
    import numpy as np
    try:
        radius = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"the blur radius must be a number in [0, {MASK_BLUR_MAX:g}], got {radius!r}") from None
    if not 0.0 <= radius <= MASK_BLUR_MAX:  # also refuses NaN
        raise ValueError(f"the blur radius must be finite and in [0, {MASK_BLUR_MAX:g}], got {radius!r}")
    sigma2 = radius * radius / 3
    l = math.floor((math.sqrt(12.0 * sigma2 + 1.0) - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2) / (6 * (sigma2 - (l + 1) * (l + 1)))
    fr = np.float32(l + a)
    r = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / (np.float32(2) * fr + np.float32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def _u8_plane(t, name):
    """uint8 [H,W] / [H,W,1] on the device -> (pointer, H, W), sides within RESIZE_MAX_DIM"""
    p = _dev(t, torch.uint8, name)
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 1)):
        _reject(f"{name} must be uint8 [H,W] or [H,W,1], got {tuple(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    if not (1 <= H <= RESIZE_MAX_DIM and 1 <= W <= RESIZE_MAX_DIM):
        _reject(f"{name}: H and W must be in 1..{RESIZE_MAX_DIM}, got {H} x {W}")
    return p, H, W


def gaussian_blur_u8(img, radius):
    """``Image.filter(ImageFilter.GaussianBlur(radius))`` of an 8-bit single-channel image, Pillow's bytes: img uint8 [H,W] or
    [H,W,1] on the device -> a new tensor of the same shape.  Two launches (three box passes along the rows, three along the
    columns, each staged in LDS).  See ed_box_blur3_rows_u8."""
    p_img, H, W = _u8_plane(img, "img")
    try:
        r, ww, fw = gaussian_box_parameters(radius)
    except ValueError as e:
        _reject(f"gaussian_blur_u8: {e}")
    tmp, out = torch.empty_like(img), torch.empty_like(img)
    p_tmp, p_out = _dev(tmp, torch.uint8, "tmp"), _dev(out, torch.uint8, "out")
    stream = _stream()
    dev = _LAUNCH["device"]
    _call("ed_box_blur3_rows_u8", p_img, H, W, r, ww, fw, p_tmp, stream)
    TIMER.note_work("ed_box_blur3_rows_u8", nbytes=2.0 * H * W)
    _LAUNCH["device"] = dev
    _call("ed_box_blur3_cols_u8", p_tmp, H, W, r, ww, fw, p_out, stream)
    TIMER.note_work("ed_box_blur3_cols_u8", nbytes=2.0 * H * W)
    return out


def mask_levels_to_latent(mask, scale=1):
    """mask uint8 / bool [H,W] (or [H,W,1]) -> the level map uint8 [H // scale, W // scale]: ``out[y, x] = mask[scale * y,
    scale * x]``, the byte itself (``scale`` 1: a copy of a map that is already at latent resolution).  A bool mask is taken as
    0 / 255.  See ed_mask_levels_to_latent."""
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.to(torch.uint8) * 255
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8:
        _reject(f"mask must be a uint8 or bool tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
    p_src, H, W = _u8_plane(mask, "mask")
    scale = int(scale)
    if scale < 1 or H % scale or W % scale:
        _reject(f"mask: {H} x {W} is not a non-empty multiple of scale {scale}")
    Hl, Wl = H // scale, W // scale
    out = torch.empty((Hl, Wl), dtype=torch.uint8, device=mask.device)
    _call("ed_mask_levels_to_latent", p_src, H, W, scale, _dev(out, torch.uint8, "out"), Hl, Wl, _stream())
    TIMER.note_work("ed_mask_levels_to_latent", nbytes=2.0 * Hl * Wl)  # algorithmic: one sampled byte in, one out
    return out


def inpaint_blend_level(x, level, thr, z0, noise, a, b, out=None, clean=False):
    """``inpaint_blend`` with a level map: out = where(level > thr, x, known), known = a * z0 + b * noise, or z0 itself with
    ``clean``.  level uint8 [H,W] (``mask_levels_to_latent``), thr an integer in 0..255; ``out`` None = in place into ``x``.
    See ed_inpaint_blend_level."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        _reject(f"inpaint_blend_level: x must be an f32 [B,C,H,W] tensor on the MI355X; no CPU fallback (got "
                f"{tuple(getattr(x, 'shape', ()))})")
    B, C, H, W = x.shape
    if not isinstance(level, torch.Tensor) or level.dtype != torch.uint8:
        _reject(f"inpaint_blend_level: level must be uint8 (ops.mask_levels_to_latent), got "
                f"{getattr(level, 'dtype', type(level).__name__)}")
    if tuple(level.shape) != (H, W):
        _reject(f"inpaint_blend_level: level must be [{H}, {W}], got {tuple(level.shape)}")
    if isinstance(thr, bool) or not isinstance(thr, int) or not 0 <= thr <= 255:
        _reject(f"inpaint_blend_level: thr must be an integer in 0..255, got {thr!r}")
    if noise is None and not clean:
        _reject("inpaint_blend_level: noise is required unless clean")
    out = x if out is None else out
    for name, t in (("z0", z0), ("noise", noise), ("out", out)):
        if t is not None and tuple(getattr(t, "shape", ())) != tuple(x.shape):
            _reject(f"inpaint_blend_level: {name} must have x's shape {tuple(x.shape)}, got {tuple(getattr(t, 'shape', ()))}")
    _call("ed_inpaint_blend_level", _dev(x, torch.float32, "x"), _dev(level, torch.uint8, "level"), thr,
          _dev(z0, torch.float32, "z0"), _opt(noise, torch.float32, "noise"), float(a), float(b), int(bool(clean)),
          _dev(out, torch.float32, "out"), B * C, H * W, _stream())
    n = x.numel()
    TIMER.note_work("ed_inpaint_blend_level", flops=0.0 if clean else 3.0 * n, nbytes=float(n * (12 if clean else 16) + n))
    return out


def composite_u8(decoded, init, mask):
    """``PIL.Image.composite`` of the decoded picture over the init picture through the pixel mask, fused with ``_to_pil``'s
    float -> 8-bit conversion: decoded f32 [1,3,H,W] in [0,1], init uint8 [H,W,3], mask uint8 [H,W] (255 = the decoded
    picture, 0 = the init picture) -> uint8 [H,W,3].  See ed_composite_u8."""
    p_dec = _dev(decoded, torch.float32, "decoded")
    if decoded.dim() != 4 or decoded.shape[0] != 1 or decoded.shape[1] != 3:
        _reject(f"decoded must be f32 [1,3,H,W], got {tuple(decoded.shape)}")
    H, W = int(decoded.shape[2]), int(decoded.shape[3])
    if not (1 <= H <= RESIZE_MAX_DIM and 1 <= W <= RESIZE_MAX_DIM):
        _reject(f"decoded: H and W must be in 1..{RESIZE_MAX_DIM}, got {H} x {W}")
    p_init, p_mask = _dev(init, torch.uint8, "init"), _dev(mask, torch.uint8, "mask")
    if tuple(init.shape) != (H, W, 3):
        _reject(f"init must be uint8 [{H},{W},3], got {tuple(init.shape)}")
    if tuple(mask.shape) not in ((H, W), (H, W, 1)):
        _reject(f"mask must be uint8 [{H},{W}], got {tuple(mask.shape)}")
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=decoded.device)
    _call("ed_composite_u8", p_dec, p_init, p_mask, _dev(out, torch.uint8, "out"), H, W, _stream())
    TIMER.note_work("ed_composite_u8", nbytes=float(H * W * (12 + 3 + 1 + 3)))
    return out


def canvas_pad_u8(img, left, top, right, bottom):
    """The outpainting canvas: img uint8 [H,W,3] -> (canvas uint8 [H',W',3] = ``np.pad(img, mode="edge")`` by the four borders,
    mask uint8 [H',W']: 255 on the new border, 0 over the original).  One launch.  See ed_canvas_pad_u8."""
    p_img = _dev(img, torch.uint8, "img")
    if img.dim() != 3 or img.shape[2] != 3:
        _reject(f"img must be uint8 [H,W,3], got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    pads = (left, top, right, bottom)
    if any(isinstance(p, bool) or not isinstance(p, int) or p < 0 for p in pads):
        _reject(f"canvas_pad_u8: the borders must be integers >= 0, got {pads!r}")
    Ho, Wo = H + top + bottom, W + left + right
    if not (1 <= H and 1 <= W and Ho <= RESIZE_MAX_DIM and Wo <= RESIZE_MAX_DIM):
        _reject(f"canvas_pad_u8: {H} x {W} padded to {Ho} x {Wo}: sides must be in 1..{RESIZE_MAX_DIM}")
    canvas = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device=img.device)
    mask = torch.empty((Ho, Wo), dtype=torch.uint8, device=img.device)
    _call("ed_canvas_pad_u8", p_img, H, W, left, top, right, bottom, _dev(canvas, torch.uint8, "canvas"),
          _dev(mask, torch.uint8, "mask"), _stream())
    TIMER.note_work("ed_canvas_pad_u8", nbytes=float(Ho * Wo * 7))
    return canvas, mask


def lora_merge(table):
    """Merge every touched weight of one model from its pristine copy and its active adapters: ONE launch over ``table``
    (``lora.LoraTable``, uploaded: ``host`` int64 on the CPU and ``dev`` its device copy; layout in include/elastic_hip.h).  The
    tensors the table points to (``table.keep``) are checked here -- on the device of the table, base and destination dense in the
    same order, fp32 factors of matching extents -- and every word of the table again by ed_lora_merge before it launches."""
    host, dev = getattr(table, "host", None), getattr(table, "dev", None)
    p_dev = _dev(dev, torch.int64, "table.dev")
    if not isinstance(host, torch.Tensor) or host.is_cuda or host.dtype != torch.int64 or not host.is_contiguous() or \
            host.shape != dev.shape or host.numel() != 8 * table.n_tensors + 4 * table.n_adapters:
        _reject("table.host must be the int64 CPU tensor table.dev was copied from (8 words per tensor, 4 per adapter)")
    for base, dst, adapters in table.keep:
        for t, what in ((base, "base"), (dst, "destination")):
            if not isinstance(t, torch.Tensor) or t.device != dev.device:
                _reject(f"lora_merge: {what} must be a tensor on {dev.device}; no CPU fallback")
            if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
                _reject(f"lora_merge: {what} must be dense in contiguous or channels-last order")
        if base.shape != dst.shape or base.dtype != dst.dtype or base.stride() != dst.stride() or base.numel() >= 2 ** 31:
            _reject(f"lora_merge: base {tuple(base.shape)} {base.dtype} and destination {tuple(dst.shape)} {dst.dtype} must agree "
                    "in shape, strides and dtype, below 2^31 elements")
        N = int(base.shape[0])
        for up, down, _ in adapters:
            _dev(up, torch.float32, "up")
            _dev(down, torch.float32, "down")
            if up.dim() != 2 or down.dim() != 2 or up.shape[0] != N or up.shape[1] != down.shape[0] or \
                    down.shape[1] * N != base.numel():
                _reject(f"lora_merge: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit a weight of {tuple(base.shape)}")
    _call("ed_lora_merge", host.data_ptr(), p_dev, table.n_tensors, table.n_adapters, table.n_tiles, _stream())
    TIMER.note_work("ed_lora_merge", flops=table.flops, nbytes=table.nbytes)


# ---- Multi-ControlNet hand-off -------------------------------------------------------------------------
CONTROL_MAX_NETS = 4        # ED_CONTROL_MAX_NETS
CONTROL_MAX_LEVELS = 32     # ED_CONTROL_MAX_LEVELS
CONTROL_LEVEL_WORDS = 12    # ED_CONTROL_LEVEL_WORDS
CONTROL_TILE = 4096         # ED_CONTROL_TILE
_CONTROL_PAIRS = {(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32),
                  (torch.float32, torch.float16), (torch.float32, torch.bfloat16)}  # (skip / out, residuals)


def control_residuals_torch(skip, residuals, w, out_dtype=None):
    """One level of ``control_residuals`` as the torch op sequence it replaces: ``acc = f32(skip)`` (or +0), then per net in order
    ``acc = acc + w[:, n] * f32(r_n)`` for the batch rows whose weight is not zero, one cast at the end.  Any device, any strides."""
    r0 = residuals[0]
    acc = torch.zeros(r0.shape, dtype=torch.float32, device=r0.device) if skip is None else skip.float()
    for n, r in enumerate(residuals):
        wn = w[:, n].to(device=r.device, dtype=torch.float32).view(-1, *([1] * (r.dim() - 1)))
        acc = torch.where(wn != 0, acc + wn * r.float(), acc)
    return acc.to(out_dtype or (r0.dtype if skip is None else skip.dtype))


def _control_dense(t):
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def control_table(levels, n_nets):
    """The descriptor table of one ``ed_control_residuals`` launch (layout: include/elastic_hip.h) for ``levels`` = [(skip or None,
    out, [r_0 .. r_{N-1}])] -> (host int64 tensor, n_tiles)."""
    words, tile = [], 0
    for skip, out, rs in levels:
        B = int(out.shape[0])
        count = out.numel() // B
        words += [0 if skip is None else skip.data_ptr(), out.data_ptr(), count, B, _DTYPE[out.dtype], _DTYPE[rs[0].dtype], tile, 0]
        words += [r.data_ptr() for r in rs] + [0] * (CONTROL_MAX_NETS - n_nets)
        tile += B * ((count + CONTROL_TILE - 1) // CONTROL_TILE)
    return torch.tensor(words, dtype=torch.int64), tile


def control_residuals(skips, residuals, w, outs=None):
    """The hand-off of N ControlNets' residuals to the UNet: for every level l,
    ``out[l] = skip[l] + sum_n w[:, n] * residuals[n][l]`` -- fp32 products and sums in net order, one rounding to the type of the
    skip -- in ONE ``ed_control_residuals`` launch over all levels.  ``skips``: list of tensors, entries (or the whole list) may be
    None: the level is then the weighted sum alone, in the residuals' type.  ``residuals``: per net, the list of its raw residuals.
    ``w``: f32 [B, N] on the device, one weight per batch row and net; a zero leaves the term out and the residual unread.
    ``outs``: per level a tensor to write, or None = in place into the skip (a fresh tensor where there is no skip).
    Returns the list of outputs.  The tensors of a level must be dense with identical strides (contiguous or channels-last alike);
    a level where they are not runs ``control_residuals_torch``, and so does every level of tensors that are not on a ROCm device."""
    N = len(residuals)
    if not 1 <= N <= CONTROL_MAX_NETS:
        raise ValueError(f"control_residuals: 1 .. {CONTROL_MAX_NETS} ControlNets, got {N}")
    L = len(residuals[0])
    skips = [None] * L if skips is None else list(skips)
    outs = [None] * L if outs is None else list(outs)
    if L < 1 or any(len(r) != L for r in residuals) or len(skips) != L or len(outs) != L:
        raise ValueError("control_residuals: every net, the skips and the outputs must list the same levels")
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != N:
        raise ValueError(f"control_residuals: w must be a float32 [B, {N}] tensor")
    B = int(w.shape[0])
    result, fused = [None] * L, []
    for l in range(L):
        rs, skip = [residuals[n][l] for n in range(N)], skips[l]
        out = outs[l] if outs[l] is not None else (skip if skip is not None else torch.empty_like(rs[0]))
        like = rs + [out] + ([] if skip is None else [skip])
        if any(t.shape != out.shape or t.device != out.device for t in like) or out.shape[0] != B or out.numel() == 0:
            raise ValueError(f"control_residuals: level {l}: skip, residuals and output must share one shape with {B} batch rows "
                             "and one device")
        if any(r.dtype != rs[0].dtype for r in rs) or (skip is not None and skip.dtype != out.dtype) or \
                (out.dtype, rs[0].dtype) not in _CONTROL_PAIRS or (skip is None and out.dtype != rs[0].dtype):
            raise ValueError(f"control_residuals: level {l}: unsupported types (skip / out {out.dtype}, residuals "
                             f"{[r.dtype for r in rs]})")
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
        if any(r.data_ptr() < hi and lo < r.data_ptr() + r.numel() * r.element_size() for r in rs):
            raise ValueError(f"control_residuals: level {l}: the output overlaps a residual")
        result[l] = out
        if out.is_cuda and w.is_cuda and all(_control_dense(t) and t.stride() == out.stride() for t in like):
            fused.append((skip, out, rs))
        else:
            out.copy_(control_residuals_torch(skip, rs, w, out.dtype))
    for i in range(0, len(fused), CONTROL_MAX_LEVELS):  # (a UNet has 10 -- 13 levels: one launch)
        part = fused[i:i + CONTROL_MAX_LEVELS]
        host, n_tiles = control_table(part, N)
        p_w = _dev(w, torch.float32, "w")
        for skip, out, rs in part:
            for t in rs + [out] + ([] if skip is None else [skip]):
                if t.device != w.device:
                    _reject(f"control_residuals: a level lives on {t.device} but w on {w.device}")
        nbytes = sum(out.numel() * ((0 if skip is None else out.element_size()) + out.element_size() + N * rs[0].element_size())
                     for skip, out, rs in part)
        _call("ed_control_residuals", host.data_ptr(), len(part), N, p_w, n_tiles, _stream())
        TIMER.note_work("ed_control_residuals", nbytes=float(nbytes))
    return result
