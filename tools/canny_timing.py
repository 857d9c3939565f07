"""Per-stage time of the Canny condition extraction (csrc/canny_kernels.hip) on the MI355X.

    python tools/canny_timing.py [--out profiles/canny_timing.json] [--repeats 20] [--sizes 512 1024 2048]

For each size and each input (the sample photo resized as the reference command line does, uniform noise, and for the
hysteresis stage a synthetic one-pixel spiral with one strong pixel) it reports, after warm-up, the MEDIAN over
``--repeats`` runs of the HIP-event time of every stage (ed_canny_map, ed_canny_hysteresis, ed_canny_edges) and of
``ops.canny`` as a whole, the number of global hysteresis passes, the bytes each stage has to move and the share of
the HBM roof that implies, and -- for scale only, it is a test helper -- the wall time of the numpy restatement
(tests/canny_cpu.py) on the same box.  ed_canny_hysteresis includes one stream synchronisation per pass: its event
time is launch + flag read-back round trips, not kernel time.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import ops  # noqa: E402
from tests import canny_cpu as cc  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X peak HBM3E bandwidth


def _timed(fn, repeats, warmup=3):
    """median / min of the HIP-event time (us) of fn() over ``repeats`` runs after ``warmup`` runs; -> (median, min, last result)"""
    for _ in range(warmup):
        res = fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    return statistics.median(us), min(us), res


def spiral_map(n):
    pts = cc.spiral_path(n)
    cmap = np.ones((n, n), np.uint8)
    cmap[pts[:, 0], pts[:, 1]] = 0
    cmap[pts[0, 0], pts[0, 1]] = 2
    return cmap


def measure_image(name, img, repeats):
    H, W, C = img.shape
    dev = torch.from_numpy(np.array(img)).cuda()
    t0 = time.perf_counter()
    want_map = cc.canny_map(img)
    flood, cpu_passes = cc.hysteresis(want_map)
    cpu_s = time.perf_counter() - t0
    map_us, map_min, cmap = _timed(lambda: ops.canny_map(dev, 100, 200), repeats)
    assert np.array_equal(cmap.cpu().numpy(), want_map), "map differs from the restatement"
    hyst_us, hyst_min, (flooded, passes) = _timed(lambda: ops.canny_hysteresis(cmap.clone()), repeats)
    clone_us, _, _ = _timed(lambda: cmap.clone(), repeats)
    assert np.array_equal(flooded.cpu().numpy(), flood), "hysteresis differs from the restatement"
    edges_us, edges_min, _ = _timed(lambda: ops.canny_edges(flooded, "u8"), repeats)
    cond_us, cond_min, _ = _timed(lambda: ops.canny_edges(flooded, "cond"), repeats)
    total_us, total_min, _ = _timed(lambda: ops.canny(dev, 100, 200, out="cond"), repeats)
    px = H * W
    row = {
        "input": name, "H": H, "W": W, "C": C, "edge_fraction": float((flood == 2).mean()),
        "global_passes": passes, "restatement_dilation_passes": cpu_passes,
        "us_median": {"ed_canny_map": map_us, "ed_canny_hysteresis": hyst_us - clone_us, "ed_canny_edges_u8": edges_us,
                      "ed_canny_edges_cond": cond_us, "ops.canny(out=cond)": total_us},
        "us_min": {"ed_canny_map": map_min, "ed_canny_hysteresis": hyst_min - clone_us, "ed_canny_edges_u8": edges_min,
                   "ed_canny_edges_cond": cond_min, "ops.canny(out=cond)": total_min},
        "bytes": {"ed_canny_map": px * (C + 1), "ed_canny_hysteresis_per_pass": px, "ed_canny_edges_u8": 4 * px,
                  "ed_canny_edges_cond": 13 * px},
        "restatement_numpy_s": cpu_s,
    }
    row["share_of_hbm_roof"] = {k: row["bytes"][k] / HBM_BYTES_PER_S / (row["us_median"][k] * 1e-6)
                                for k in ("ed_canny_map", "ed_canny_edges_u8", "ed_canny_edges_cond")}
    return row


def measure_spiral(n, repeats):
    cmap = spiral_map(n)
    dev = torch.from_numpy(cmap).cuda()
    us, us_min, (flooded, passes) = _timed(lambda: ops.canny_hysteresis(dev.clone()), repeats, warmup=1)
    clone_us, _, _ = _timed(lambda: dev.clone(), repeats)
    assert np.array_equal(flooded.cpu().numpy(), np.where(cmap == 0, 2, cmap)), "spiral not fully promoted"
    return {"input": "spiral", "H": n, "W": n, "chain_pixels": int((cmap == 0).sum()), "global_passes": passes,
            "us_median": {"ed_canny_hysteresis": us - clone_us}, "us_min": {"ed_canny_hysteresis": us_min - clone_us},
            "us_per_pass": (us - clone_us) / passes}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canny_timing.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024, 2048])
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    from PIL import Image
    photo = Image.open(os.path.join(ROOT, "tests", "golden", "canny_input_yoga.jpeg"))
    rows = []
    for n in opt.sizes:
        rows.append(measure_image("photo", np.asarray(photo.resize((n, n)).convert("RGB")), opt.repeats))
        rows.append(measure_image("noise", np.random.default_rng(n).integers(0, 256, (n, n, 3), dtype=np.uint8), opt.repeats))
        rows.append(measure_spiral(n, max(3, opt.repeats // 4)))
        for r in rows[-3:]:
            print(json.dumps(r))
    result = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats,
              "method": "HIP events around each ops call on the current stream, warm-up 3, median and minimum of the repeats; the "
                        "hysteresis figure has the time of the map copy it works on subtracted and includes one stream "
                        "synchronisation per global pass; one run, no claim against OpenCV",
              "rows": rows}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
