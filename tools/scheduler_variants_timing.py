"""Time of the fused phase epilogue (ed_phase_epilogue / ed_phase_epilogue_pt) by prediction type on the MI355X.

    python tools/scheduler_variants_timing.py [--parent-lib PATH] [--out profiles/scheduler_variants_timing.json]
                                              [--rounds 5] [--repeats 20] [--inner 20]

Geometry: the SDXL 1024 x 2048 headline (latent 128 x 256, reduced 64 x 128, model size 128, 8 views), K = 8 resampling
steps, one prompt, fp16 model rows, with the fused RRG term (x_next) and without it.  Arms, alternated within every round:

    parent_epsilon   ed_phase_epilogue of a library built from the parent commit (``--parent-lib``; skipped without it)
    epsilon          ed_phase_epilogue of this tree (the unchanged path: the same kernel instantiation)
    v_prediction     ed_phase_epilogue_pt(ED_PRED_V) of this tree

One run = HIP events around ``--inner`` back-to-back launches on the current stream, divided by ``--inner``; per round and
arm the MEDIAN of ``--repeats`` runs after warm-up; ``--rounds`` rounds.  The spread of an arm is max - min of its round
medians.  The condition the project sets: the epsilon arm's median of round medians may exceed the parent's by no more
than the parent's own spread.  The outputs of the epsilon arms are compared bit for bit.  The bytes are the compulsory
traffic computed from the shapes (every output written once, every needed input element read once), the same for both
prediction types; the v form trades one division for three multiplications per element.  At a few MB per launch the event
figure is dominated by the enqueue of the Python wrapper: device-side kernel durations come from a ``rocprofv3 --kernel-trace``
run of this tool (a run of its own).  Needs the GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import _hip, geometry, host_rng, ops, schedule  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X peak HBM3E bandwidth
HL, WL, H_LOW, W_LOW, MODEL, K, B, C = 128, 256, 64, 128, 128, 8, 1, 4


def load_library(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, argtypes in _hip.SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = (ctypes.c_char_p if name == "ed_error_string" else
                          ctypes.c_int64 if name.endswith("_workspace") else ctypes.c_int)
    return L


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def make_inputs(dtype=torch.float16, seed=0):
    ws = MODEL // 2
    pp, vp = geometry.PickPlan(HL, WL, H_LOW, W_LOW), geometry.ViewPlan(HL, WL, ws, ws, MODEL - ws)
    gpad, vpad = geometry.PadPlan(H_LOW, W_LOW, MODEL), geometry.PadPlan(vp.Sh, vp.Sw, MODEL)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    stamp = torch.empty(H_LOW * W_LOW, 4, dtype=torch.int8)
    host_rng.PickSampler(H_LOW * W_LOW).draw(K, 0.7, lambda: None, stamp=stamp)
    pick = tuple(dev_i32(getattr(pp, k)) for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col"))
    cover = tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left))
    return dict(
        x=torch.randn(B, C, HL, WL, generator=g).cuda(), stamp=stamp.cuda(), pick=pick, cover=cover,
        g_out=torch.randn(2 * K * B, C, gpad.PH, gpad.PW, generator=g).to(dtype).cuda(),
        v_out=torch.randn(vp.V * B, C, vpad.PH, vpad.PW, generator=g).to(dtype).cuda(),
        low_latent=torch.randn(B, C, H_LOW, W_LOW, generator=g).cuda(), ncb=vp.n_col_blocks, g_off=(gpad.top, gpad.left),
        views=vp.V)


def launcher(inp, coef, prediction_type, rrg):
    x = inp["x"]
    out = {k: torch.empty_like(x) for k in ("prev", "x0", "x_next")}
    low_dir, unc = torch.empty_like(inp["low_latent"]), torch.empty_like(inp["low_latent"])
    norm = np.float32(2.0 / (C * HL * WL))

    def run():
        ops.phase_epilogue(inp["g_out"], inp["v_out"], x, inp["stamp"], inp["pick"], inp["cover"], inp["ncb"], inp["g_off"],
                           K, H_LOW, W_LOW, np.float32(10.0), coef, out["prev"], out["x0"], low_dir=low_dir,
                           uncond_last=unc, x_next=out["x_next"] if rrg else None,
                           low_latent=inp["low_latent"] if rrg else None, rrg_norm=norm,
                           rrg_weight=np.float32(437.5) if rrg else 0.0, prediction_type=prediction_type)
    return run, out


def compulsory_bytes(rrg, elem=2):
    n_full, n_low = B * C * HL * WL, B * C * H_LOW * W_LOW
    per_full = 4 + 2 * 4 + 2 * elem + elem + (4 if rrg else 0)  # x; prev, x0; cond, uncond of the covering step; the view centre; x_next
    per_low = 2 * 4 + 3 * elem + (4 if rrg else 0)              # low_dir, uncond_last; their three rows; low_latent
    return n_full * per_full + n_low * per_low


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
    ap.add_argument("--parent-lib", default=None, help="libelastic_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scheduler_variants_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    if opt.repeats < 20:
        raise SystemExit("--repeats must be at least 20")
    product = _hip.lib()
    libs = {"epsilon": (product, "epsilon"), "v_prediction": (product, "v_prediction")}
    parent_version = None
    if opt.parent_lib:
        parent = load_library(opt.parent_lib)
        parent_version = int(parent.ed_version())
        libs = {"parent_epsilon": (parent, "epsilon"), **libs}
    sch = schedule.DDIMSchedule(prediction_type="v_prediction")
    coef = sch.step_coefficients(sch.set_timesteps(50)[7])
    inp = make_inputs()
    rows = []
    try:
        for rrg in (True, False):
            arms = {}
            for name, (L, pt) in libs.items():
                run, out = launcher(inp, coef, pt, rrg)
                arms[name] = dict(lib=L, run=run, out=out, medians=[])
                _hip._LIB = L
                for _ in range(10):  # warm-up: code object load, clocks
                    run()
            torch.cuda.synchronize()
            for _ in range(opt.rounds):
                for name, arm in arms.items():  # alternate the arms inside every round
                    _hip._LIB = arm["lib"]
                    arm["medians"].append(timed_us(arm["run"], opt.repeats, opt.inner))
            _hip._LIB = product
            row = {"rrg_fused": rrg, "bytes": compulsory_bytes(rrg), "us_round_medians": {}, "us": {}, "spread_us": {}}
            for name, arm in arms.items():
                row["us_round_medians"][name] = arm["medians"]
                row["us"][name] = statistics.median(arm["medians"])
                row["spread_us"][name] = max(arm["medians"]) - min(arm["medians"])
            row["share_of_hbm_roof"] = {n: row["bytes"] / HBM_BYTES_PER_S / (row["us"][n] * 1e-6) for n in arms}
            if "parent_epsilon" in arms:
                keys = ("prev", "x0", "x_next") if rrg else ("prev", "x0")
                row["epsilon_bit_identical_to_parent"] = all(
                    torch.equal(arms["epsilon"]["out"][k], arms["parent_epsilon"]["out"][k]) for k in keys)
                row["epsilon_minus_parent_us"] = row["us"]["epsilon"] - row["us"]["parent_epsilon"]
                row["condition_epsilon_not_slower_than_parent_beyond_its_spread"] = (
                    row["epsilon_minus_parent_us"] <= row["spread_us"]["parent_epsilon"])
            row["v_differs_from_epsilon"] = not torch.equal(arms["epsilon"]["out"]["prev"], arms["v_prediction"]["out"]["prev"])
            rows.append(row)
            print(json.dumps(row))
    finally:
        _hip._LIB = product
    result = {"device": torch.cuda.get_device_name(0), "geometry": dict(latent=[HL, WL], reduced=[H_LOW, W_LOW], model=MODEL,
                                                                          K=K, B=B, views=inp["views"], rows_dtype="float16"),
              "abi": {"this_tree": _hip.ABI_VERSION, "parent": parent_version},
              "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner,
              "method": "HIP events around `inner` back-to-back launches on the current stream / inner; per round the median of "
                        "`repeats` such runs after 10 warm-up launches; arms alternated within each round; us = median of the "
                        "round medians, spread = max - min of them; bytes = compulsory traffic from the shapes",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")
    if not all(r.get("condition_epsilon_not_slower_than_parent_beyond_its_spread", True) for r in rows):
        raise SystemExit("the epsilon launch is slower than the parent's by more than the parent's own spread")


if __name__ == "__main__":
    main()
