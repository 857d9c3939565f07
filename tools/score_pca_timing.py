"""Time of the score PCA maps (csrc/pca_kernels.hip) on the MI355X.

    python tools/score_pca_timing.py [--out profiles/score_pca_timing.json] [--rounds 5] [--per-round 20]

Arms, at latent 128 x 256 and 256 x 256 (B = 1): ``ops.score_pca`` without and with ``normalize`` (four / five launches, the
workspace reused), and the x8 BILINEAR enlargement of one map (``ops.resize_u8``, two launches).  The method of section 14.3: HIP
events on the current stream around one call, after warm-up; the arms take turns inside every round; per arm the median of each
round's ``--per-round`` calls, then the median of the round medians with their spread (min, max).  Also the mean per entry point
from ``ops.TIMER`` and the bytes each call moves.  Every timed configuration is first checked against the numpy restatement /
Pillow.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import ops  # noqa: E402
from tests import score_pca_cpu  # noqa: E402
from tests.golden.make_score_pca import make_score  # noqa: E402

SIZES = [(128, 256), (256, 256)]          # latent (H, W): SDXL 1024 x 2048 and 2048 x 2048


def _one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def _rounds(arms, rounds, per_round, warmup=5):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    medians = {name: [] for name in arms}
    for _ in range(rounds):
        us = {name: [] for name in arms}
        for _ in range(per_round):
            for name, fn in arms.items():       # the arms alternate
                us[name].append(_one(fn))
        for name in arms:
            medians[name].append(statistics.median(us[name]))
    return {name: {"median_of_round_medians_us": statistics.median(m), "min_round_us": min(m), "max_round_us": max(m)}
            for name, m in medians.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_pca_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=20)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    from PIL import Image
    rows = []
    for H, W in SIZES:
        host = make_score(26, 1, H, W)
        s = torch.from_numpy(host).cuda()
        ws = ops.score_pca_workspace(1, H * W, s.device)
        for normalize in (False, True):
            worst, share = score_pca_cpu.byte_difference(ops.score_pca(s, normalize=normalize).cpu().numpy(),
                                                         score_pca_cpu.score_pca_map(host, normalize)["bytes"])
            assert worst <= 1 and share <= 1e-3, (H, W, normalize, worst, share)
        small = ops.score_pca(s, workspace=ws)[0].contiguous()
        big = ops.resize_u8(small, (8 * H, 8 * W), filter="bilinear")
        want = np.asarray(Image.fromarray(small.cpu().numpy()).resize((8 * W, 8 * H), Image.BILINEAR))
        assert np.array_equal(big.cpu().numpy(), want), "differs from Pillow"
        arms = {"score_pca": lambda: ops.score_pca(s, workspace=ws),
                "score_pca_normalize": lambda: ops.score_pca(s, normalize=True, workspace=ws),
                "resize_u8_bilinear_x8": lambda: ops.resize_u8(small, (8 * H, 8 * W), filter="bilinear")}
        timed = _rounds(arms, opt.rounds, opt.per_round)
        ops.TIMER.start()
        for _ in range(opt.per_round):
            for fn in arms.values():
                fn()
        per = {k: {"launches": v[0], "mean_us": v[1]} for k, v in ops.TIMER.stop().items()}
        n = H * W
        rows.append({"latent_H": H, "latent_W": W, **timed, "us_per_entry_point": per,
                     "bytes_moved": {"score_pca": 51 * n, "score_pca_normalize": 67 * n,
                                     "resize_u8_bilinear_x8": 3 * n + 2 * 3 * 8 * n + 3 * 64 * n}})
        print(json.dumps(rows[-1]))
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "per_round": opt.per_round,
              "method": "HIP events on the current stream around one call (its launches and the wrapper's allocations), warm-up 5, "
                        "arms alternating inside every round, median per round, then median / min / max of the round medians; "
                        "per entry point: mean of ops.TIMER's events; bytes: 16 per pixel read by each pass over the score (3, "
                        "4 with normalize) + 3 written; the enlargement reads the map, writes and reads the row-resized "
                        "intermediate and writes the picture; one run on one box",
              "sizes": rows}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
