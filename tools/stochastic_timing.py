"""Time of the fused phase epilogue by sampler on the MI355X: the deterministic DDIM launch (ed_phase_epilogue) of this tree against
the parent commit's, and the noise variants of the stochastic samplers (ed_phase_epilogue_sde).

    python tools/stochastic_timing.py [--parent-lib PATH] [--out profiles/stochastic_timing.json]
                                      [--rounds 5] [--repeats 20] [--inner 20]

Geometry: the SDXL 1024 x 2048 headline (latent 128 x 256, reduced 64 x 128, model size 128, 8 views), K = 8 resampling
steps, one prompt, fp16 model rows, with the fused RRG term (x_next) and without it.  Arms, alternated within every round:

    parent_ddim   ed_phase_epilogue of a library built from the parent commit (``--parent-lib``; skipped without it)
    ddim          ed_phase_epilogue of this tree (the unchanged path: the same kernel instantiation, instruction for instruction)
    eta1          ed_phase_epilogue_sde, the DDIM form at eta = 1 ("euler_a"): one more latent-sized fp32 read
    sde1          ed_phase_epilogue_sde, the multistep form without a history (first-order SDE-DPM-Solver++)
    sde2          ed_phase_epilogue_sde, the multistep form with a history: two more latent-sized fp32 reads
    lcm           ed_phase_epilogue_sde, the multistep form with LCM's scalars (the kernel of sde1)

The method is tools/dpm_solver_timing.py's (DESIGN.md sections 14.3 / 25.6): one run = HIP events around ``--inner`` back-to-back
launches on the current stream, divided by ``--inner``; per round and arm the MEDIAN of ``--repeats`` runs after warm-up;
``--rounds`` rounds; us = the median of the round medians, spread = max - min of them.  The condition the project sets: the ddim
arm's figure may exceed the parent's by no more than the parent's own spread, and its outputs are the parent's bit for bit.  The
stochastic figures are reported as they come.  At a few MB per launch the event figure is dominated by the enqueue of the Python
wrapper.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from elasticdiffusion_official_amd import _hip, ops, schedule  # noqa: E402
from scheduler_variants_timing import (B, C, H_LOW, HBM_BYTES_PER_S, HL, K, MODEL, W_LOW, WL, compulsory_bytes, load_library,  # noqa: E402
                                       make_inputs, timed_us)


def launcher(inp, coef, rrg, **kw):
    x = inp["x"]
    out = {k: torch.empty_like(x) for k in ("prev", "x0", "x_next")}
    low_dir, unc = torch.empty_like(inp["low_latent"]), torch.empty_like(inp["low_latent"])
    norm = np.float32(2.0 / (C * HL * WL))

    def run():
        ops.phase_epilogue(inp["g_out"], inp["v_out"], x, inp["stamp"], inp["pick"], inp["cover"], inp["ncb"], inp["g_off"],
                           K, H_LOW, W_LOW, np.float32(10.0), coef, out["prev"], out["x0"], low_dir=low_dir,
                           uncond_last=unc, x_next=out["x_next"] if rrg else None,
                           low_latent=inp["low_latent"] if rrg else None, rrg_norm=norm,
                           rrg_weight=np.float32(437.5) if rrg else 0.0, **kw)
    return run, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libelastic_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stochastic_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    if opt.repeats < 20:
        raise SystemExit("--repeats must be at least 20")
    product = _hip.lib()
    ddim, eta1 = schedule.DDIMSchedule(), schedule.DDIMSchedule(eta=1.0)
    sde, lcm = schedule.DPMSolverSchedule(algorithm_type="sde-dpmsolver++"), schedule.LCMSchedule()
    for s in (ddim, eta1, sde, lcm):
        ts = s.set_timesteps(25)
    t, t_hist = ts[7], ts[6]
    inp = make_inputs()
    gen = torch.Generator().manual_seed(1)
    x0_hist = torch.randn(B, C, HL, WL, generator=gen).cuda()
    noise = torch.randn(B, C, HL, WL, generator=gen).cuda()
    ms = sde.multistep_coefficients(t, t_hist, False)[2:]
    arms_spec = {
        "ddim": (product, ddim.step_coefficients(t), {}),
        "eta1": (product, eta1.step_coefficients(t), dict(noise=(eta1.noise_coefficient(t), noise))),
        "sde1": (product, sde.step_coefficients(t), dict(multistep=ms + (None,), noise=(sde.noise_coefficient(t), noise))),
        "sde2": (product, sde.step_coefficients(t), dict(multistep=ms + (x0_hist,), noise=(sde.noise_coefficient(t), noise))),
        "lcm": (product, lcm.step_coefficients(t), dict(multistep=lcm.multistep_coefficients(t)[2:] + (None,),
                                                         noise=(lcm.noise_coefficient(t), noise))),
    }
    extra_reads = {"ddim": 0, "parent_ddim": 0, "eta1": 1, "sde1": 1, "sde2": 2, "lcm": 1}
    parent_version = None
    if opt.parent_lib:
        parent = load_library(opt.parent_lib)
        parent_version = int(parent.ed_version())
        arms_spec = {"parent_ddim": (parent, ddim.step_coefficients(t), {}), **arms_spec}
    rows = []
    try:
        for rrg in (True, False):
            arms = {}
            for name, (L, coef, kw) in arms_spec.items():
                run, out = launcher(inp, coef, rrg, **kw)
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
            n_full = B * C * HL * WL
            row = {"rrg_fused": rrg, "bytes": {n: compulsory_bytes(rrg) + 4 * n_full * extra_reads[n] for n in arms},
                   "us_round_medians": {}, "us": {}, "spread_us": {}}
            for name, arm in arms.items():
                row["us_round_medians"][name] = arm["medians"]
                row["us"][name] = statistics.median(arm["medians"])
                row["spread_us"][name] = max(arm["medians"]) - min(arm["medians"])
            row["share_of_hbm_roof"] = {n: row["bytes"][n] / HBM_BYTES_PER_S / (row["us"][n] * 1e-6) for n in arms}
            keys = ("prev", "x0", "x_next") if rrg else ("prev", "x0")
            if "parent_ddim" in arms:
                row["ddim_bit_identical_to_parent"] = all(
                    torch.equal(arms["ddim"]["out"][k], arms["parent_ddim"]["out"][k]) for k in keys)
                row["ddim_minus_parent_us"] = row["us"]["ddim"] - row["us"]["parent_ddim"]
                row["condition_ddim_within_parent_spread"] = row["ddim_minus_parent_us"] <= row["spread_us"]["parent_ddim"]
            row["minus_ddim_us"] = {n: row["us"][n] - row["us"]["ddim"] for n in ("eta1", "sde1", "sde2", "lcm")}
            row["x0_identical_across_samplers"] = all(torch.equal(arms["ddim"]["out"]["x0"], arms[n]["out"]["x0"])
                                                      for n in ("eta1", "sde1", "sde2", "lcm"))
            row["stochastic_differs_from_ddim"] = all(not torch.equal(arms["ddim"]["out"]["prev"], arms[n]["out"]["prev"])
                                                      for n in ("eta1", "sde1", "sde2", "lcm"))
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
    if not all(r.get("ddim_bit_identical_to_parent", True) for r in rows):
        raise SystemExit("the DDIM launch of this tree does not give the parent's bits")
    if not all(r.get("condition_ddim_within_parent_spread", True) for r in rows):
        raise SystemExit("the DDIM launch is slower than the parent's by more than the parent's own spread")


if __name__ == "__main__":
    main()
