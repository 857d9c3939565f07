"""Time of the GroupNorm entry points of this tree against a library built from the parent commit, on the MI355X.

    python tools/groupnorm_timing.py --parent-lib PATH [--out profiles/groupnorm_timing.json] [--rounds 5] [--repeats 20] [--inner 10]

The statistics passes accumulate x - K and (x - K)^2 instead of x and x^2: one subtraction per element more
in kernels that stream memory.  Arms ``parent`` and ``this_tree`` run the same ops.* call on the same tensors and are alternated
within every round.  One run = HIP events around ``--inner`` back-to-back calls / ``--inner``; per round and arm the median of
``--repeats`` runs after warm-up; us = median of the round medians, spread = max - min of them.  The condition: this tree's figure
exceeds the parent's by no more than the parent's own spread.  Needs the GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import _hip, ops  # noqa: E402


def load_library(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, argtypes in _hip.SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = (ctypes.c_char_p if name == "ed_error_string" else
                      ctypes.c_int64 if name.endswith("_workspace") else ctypes.c_int)
    return L


def cases():
    """(name, bytes moved, callable) at the shapes of the SDXL 1024 x 2048 workload's UNet and VAE"""
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last

    def t(shape, dtype, fmt=torch.contiguous_format):
        return (torch.randn(*shape, generator=g) * 1.7 + 0.3).to("cuda", dtype).contiguous(memory_format=fmt)

    def affine(C, dtype):
        return (1 + 0.2 * torch.randn(C, generator=g)).to("cuda", dtype), (0.1 * torch.randn(C, generator=g)).to("cuda", dtype)

    out = []
    h = torch.float16
    for shape in [(4, 1280, 32, 32), (2, 320, 128, 128)]:            # one workgroup per group / the split path
        x, (w, b) = t(shape, h), affine(shape[1], h)
        out.append((f"ed_groupnorm {shape}", 6 * x.numel(), lambda x=x, w=w, b=b: ops.groupnorm(x, w, b, 32, 1e-5, silu=True)))
    for shape in [(20, 1280, 32, 32), (6, 640, 64, 64), (6, 320, 128, 128)]:
        x, (w, b) = t(shape, h, cl), affine(shape[1], h)
        out.append((f"ed_groupnorm_nhwc {shape}", 6 * x.numel(), lambda x=x, w=w, b=b: ops.groupnorm_nhwc(x, w, b, 32, 1e-5, silu=True)))
    for (N, C1, C2, S) in [(6, 1280, 640, 32), (6, 640, 320, 64)]:
        x1, x2, (w, b) = t((N, C1, S, S), h, cl), t((N, C2, S, S), h, cl), affine(C1 + C2, h)
        out.append((f"ed_groupnorm_nhwc_cat {(N, C1, C2, S, S)}", 6 * (x1.numel() + x2.numel()),
                    lambda x1=x1, x2=x2, w=w, b=b: ops.groupnorm_nhwc_cat(x1, x2, w, b, 32, 1e-5, silu=True)))
    f = torch.float32
    shape = (1, 128, 256, 1024)                                       # the pad-strip encode's first level
    x, xl, (w, b) = t(shape, f), t(shape, f, cl), affine(shape[1], f)
    out.append((f"ed_groupnorm_f32 {shape}", 12 * x.numel(), lambda: ops.groupnorm_f32(x, w, b, 32, 1e-6, silu=True)))
    out.append((f"ed_groupnorm_nhwc_f32 {shape}", 12 * x.numel(), lambda: ops.groupnorm_nhwc_f32(xl, w, b, 32, 1e-6, silu=True)))
    out.append((f"ed_groupnorm_nhwc_f32 split {shape}", 14 * x.numel(),
                lambda: ops.groupnorm_nhwc_f32(xl, w, b, 32, 1e-6, silu=True, split=True)))
    return out


def timed_us(run, repeats, inner):
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            run()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / inner)
    return statistics.median(us)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libelastic_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupnorm_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    product = _hip.lib()
    arms = {"parent": load_library(opt.parent_lib), "this_tree": product}
    rows = []
    try:
        for name, nbytes, run in cases():
            med = {a: [] for a in arms}
            for a, L in arms.items():
                _hip._LIB = L
                for _ in range(10):
                    run()
            torch.cuda.synchronize()
            for _ in range(opt.rounds):
                for a, L in arms.items():
                    _hip._LIB = L
                    med[a].append(timed_us(run, opt.repeats, opt.inner))
            _hip._LIB = product
            us = {a: statistics.median(m) for a, m in med.items()}
            spread = {a: max(m) - min(m) for a, m in med.items()}
            row = {"case": name, "bytes": nbytes, "us_round_medians": med, "us": us, "spread_us": spread,
                   "tb_per_s": {a: nbytes / (us[a] * 1e-6) / 1e12 for a in arms},
                   "this_tree_minus_parent_us": us["this_tree"] - us["parent"],
                   "within_parent_spread": us["this_tree"] - us["parent"] <= spread["parent"]}
            rows.append(row)
            print(json.dumps(row))
    finally:
        _hip._LIB = product
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner,
              "method": "HIP events around `inner` back-to-back ops.* calls / inner; per round the median of `repeats` runs after 10 "
                        "warm-up calls; arms alternated within each round; us = median of the round medians, spread = max - min",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
