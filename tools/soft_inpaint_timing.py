"""Time of the soft-edged inpainting pieces on the MI355X.

    python tools/soft_inpaint_timing.py [--out profiles/soft_inpaint_timing.json] [--repeats 50]

Per ``ops`` call, by HIP events after 5 warm-up calls (median and minimum of ``--repeats`` calls), with the bytes each call has to
move and the GB/s that implies, at 1024 x 2048 and 2048 x 2048 pixels: ``gaussian_blur_u8`` at radius 8 and at radius 33 (two
launches: the rows pass and the columns pass, also timed apart through ``ops.TIMER``), ``mask_levels_to_latent``,
``inpaint_blend_level`` (noised and clean) next to ``inpaint_blend`` on the same latent, ``composite_u8`` and ``canvas_pad_u8`` (a
64-pixel border on every side, so that the canvas has the stated size).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import _hip, ops  # noqa: E402

SIZES = [(1024, 2048), (2048, 2048)]
RADII = [8, 33]


def _timed(fn, repeats, warmup=5):
    """-> (median us, min us) of the HIP-event time of fn() over ``repeats`` calls after ``warmup``"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    return statistics.median(us), min(us)


def _row(name, nbytes, med, mn, **extra):
    return dict({"call": name, "bytes": int(nbytes), "us_median": med, "us_min": mn, "GBps_at_median": nbytes / med * 1e-3}, **extra)


def _blur_launches(mask_px, radius, repeats):
    """the two launches of one blur apart: mean us of each under ops.TIMER"""
    ops.TIMER.start()
    for _ in range(repeats):
        ops.gaussian_blur_u8(mask_px, radius)
    return {k: v[1] for k, v in ops.TIMER.stop().items()}


def rows_for(H, W, repeats, s=8):
    g = torch.Generator().manual_seed(H + W)
    mask_px = torch.zeros(H, W, dtype=torch.uint8)
    mask_px[H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 255
    mask_px = mask_px.cuda()
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    small = img[64:H - 64, 64:W - 64].contiguous()
    decoded = torch.rand(1, 3, H, W, generator=g).cuda()
    shape = (1, 4, H // s, W // s)
    n = 4 * (H // s) * (W // s)
    x, z0, noise = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    out = torch.empty_like(x)
    soft = ops.gaussian_blur_u8(mask_px, 8)
    level = ops.mask_levels_to_latent(soft, s)
    binary = ops.mask_to_latent(soft, s)
    rows = []
    for radius in RADII:
        r, _, _ = ops.gaussian_box_parameters(radius)
        rows.append(_row(f"gaussian_blur_u8(radius={radius})", 4 * H * W, *_timed(lambda: ops.gaussian_blur_u8(mask_px, radius), repeats),
                         box_radius=r, launches_us_mean=_blur_launches(mask_px, radius, repeats),
                         column_strip=_hip.lib().ed_box_blur3_cols_strip(H, W)))
    rows += [
        _row("mask_levels_to_latent", 2 * n // 4, *_timed(lambda: ops.mask_levels_to_latent(soft, s), repeats)),
        _row("inpaint_blend_level", n * 16 + n // 4, *_timed(lambda: ops.inpaint_blend_level(x, level, 127, z0, noise, 0.6, 0.8, out=out), repeats)),
        _row("inpaint_blend_level(clean)", n * 12 + n // 4,
             *_timed(lambda: ops.inpaint_blend_level(x, level, 0, z0, None, 1.0, 0.0, out=out, clean=True), repeats)),
        _row("inpaint_blend (binary, for comparison)", n * 16 + n // 4, *_timed(lambda: ops.inpaint_blend(x, binary, z0, noise, 0.6, 0.8, out=out), repeats)),
        _row("composite_u8", H * W * (12 + 3 + 1 + 3), *_timed(lambda: ops.composite_u8(decoded, img, soft), repeats)),
        _row("canvas_pad_u8", (H - 128) * (W - 128) * 3 + H * W * 4, *_timed(lambda: ops.canvas_pad_u8(small, 64, 64, 64, 64), repeats)),
        _row("torch.empty_like of the mask (allocation only, for scale)", 0, *_timed(lambda: torch.empty_like(mask_px), repeats)),
    ]
    return {"H": H, "W": W, "latent": list(shape), "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_inpaint_timing.json"))
    ap.add_argument("--repeats", type=int, default=50)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats,
              "method": "HIP events around each ops call on the current stream (so each figure includes the wrapper's output "
                        "allocations), warm-up 5, median and minimum of the repeats; bytes = what the call must read and write (the "
                        "blur: the mask in and out once per direction); launches_us_mean: each of the blur's two launches under "
                        "ops.TIMER, mean of the repeats",
              "sizes": [rows_for(H, W, opt.repeats) for H, W in SIZES]}
    for k in result["sizes"]:
        print(json.dumps(k))
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
