"""Cost of regional prompts on the MI355X: the regional assemble and epilogue launches against the plain
ones, and seconds per image with n = 0, 1, 2, 3 regions.

    python tools/regional_timing.py [--parent-lib PATH] [--out profiles/regional_timing.json] [--rounds 5] [--repeats 20]
                                    [--inner 20] [--timesteps 50] [--no-images]

Launches.  Geometry: the SDXL 1024 x 2048 headline (latent 128 x 256, reduced 64 x 128, model size 128), K = 8 resampling steps,
one prompt, fp16 model rows, the epilogue with the fused RRG term.  Arms, alternated within every round:

    parent_assemble / parent_epilogue   ed_assemble_rows / ed_phase_epilogue of a library built from the parent commit
                                        (``--parent-lib``; skipped without it)
    assemble / epilogue                 the same entry points of this tree (the unchanged path; outputs compared bit for bit)
    assemble_n2 / assemble_n4           ed_assemble_rows_n with 2 and 4 rows per step (P = 1 and P = 3: 20 and 36 model rows)
    epilogue_rg1 / _rg2 / _rg3 / _rg4   ed_phase_epilogue_rg with P conditional rows per step and random overlapping weights
    moments / moments_rg3               ed_phase_moments and ed_phase_moments_rg at P = 3 (the guidance-rescale reduction)

The method is tools/scheduler_variants_timing.py's: one run = HIP events around ``--inner`` back-to-back
launches, divided by ``--inner``; per round and arm the median of ``--repeats`` runs after warm-up; us = the median of the round
medians, spread = max - min of them.  At a few MB per launch the event figure is dominated by the enqueue of the Python wrapper.
The condition the project sets: an unchanged arm may exceed the parent's by no more than the parent's own spread, with the
parent's bits.

Images.  ``generate_image`` of the flagship workload of bench.py (SDXL 1024 x 2048, R = 7, ``--timesteps`` steps, fp16, random-init
weights, one image in flight) with n = 0, 1, 2, 3 regions (vertical thirds / halves as boxes over a base prompt; a phase is
K (1 + P) + V = 20, 28, 36, 44 model rows): one warm-up image of 2 timesteps per n (graph capture of both phase shapes), then one
timed image, host clock around the call ending in a device synchronise.  Needs the GPU: there is no fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from elasticdiffusion_official_amd import _hip, geometry, host_rng, ops, schedule  # noqa: E402
from scheduler_variants_timing import B, C, H_LOW, HL, K, MODEL, W_LOW, WL, dev_i32, load_library, timed_us  # noqa: E402


def make_inputs(P_max=4, dtype=torch.float16, seed=0):
    ws = MODEL // 2
    pp, vp = geometry.PickPlan(HL, WL, H_LOW, W_LOW), geometry.ViewPlan(HL, WL, ws, ws, MODEL - ws)
    gpad, vpad = geometry.PadPlan(H_LOW, W_LOW, MODEL), geometry.PadPlan(vp.Sh, vp.Sw, MODEL)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    stamp = torch.empty(H_LOW * W_LOW, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(H_LOW * W_LOW).draw(K, 0.7, lambda: None, stamp=stamp)
    inp = dict(pp=pp, vp=vp, gpad=gpad, vpad=vpad, dtype=dtype, idx=idx.cuda(), stamp=stamp.cuda(),
               x=torch.randn(B, C, HL, WL, generator=g).cuda(), low_latent=torch.randn(B, C, H_LOW, W_LOW, generator=g).cuda(),
               pick=tuple(dev_i32(getattr(pp, k)) for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")),
               cover=tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left)),
               src=(dev_i32(pp.src_row), dev_i32(pp.src_col)), win=(dev_i32(vp.win_y0), dev_i32(vp.win_x0)),
               v_out=torch.randn(vp.V * B, C, vpad.PH, vpad.PW, generator=g).to(dtype).cuda(), g_out={}, region_w={})
    for P in range(1, P_max + 1):
        inp["g_out"][P] = torch.randn((1 + P) * K * B, C, gpad.PH, gpad.PW, generator=g).to(dtype).cuda()
        if P == 1:
            inp["region_w"][P] = torch.ones(1, HL, WL).cuda()
        else:
            masks = torch.randint(0, 256, (P - 1, HL, WL), generator=g, dtype=torch.uint8)
            inp["region_w"][P] = ops.region_weights(masks.cuda(), [1.0] * (P - 1))
    return inp


def assemble_launcher(inp, copies=None):
    gpad, vpad, vp = inp["gpad"], inp["vpad"], inp["vp"]
    rows = torch.empty(((copies or 2) * K + vp.V) * B, C, gpad.PH, gpad.PW, device="cuda", dtype=inp["dtype"])
    n_g = (copies or 2) * K * B
    low = torch.empty(K, B, C, H_LOW, W_LOW, device="cuda")
    args = (inp["x"], inp["idx"], *inp["src"], rows[:n_g], H_LOW, W_LOW, gpad.top, gpad.left, None, low, rows[n_g:], *inp["win"],
            vp.Sh, vp.Sw, vpad.top, vpad.left, None)
    if copies is None:
        return (lambda: ops.assemble_rows(*args)), {"rows": rows, "low": low}
    return (lambda: ops.assemble_rows_n(*args, copies)), {"rows": rows, "low": low}


def epilogue_launcher(inp, coef, P=None):
    x = inp["x"]
    out = {k: torch.empty_like(x) for k in ("prev", "x0", "x_next")}
    low_dir, unc = torch.empty_like(inp["low_latent"]), torch.empty_like(inp["low_latent"])
    norm = np.float32(2.0 / (C * HL * WL))
    kw = {} if P is None else dict(region_w=inp["region_w"][P])
    g_out = inp["g_out"][P or 1]

    def run():
        ops.phase_epilogue(g_out, inp["v_out"], x, inp["stamp"], inp["pick"], inp["cover"], inp["vp"].n_col_blocks,
                           (inp["gpad"].top, inp["gpad"].left), K, H_LOW, W_LOW, np.float32(10.0), coef, out["prev"], out["x0"],
                           low_dir=low_dir, uncond_last=unc, x_next=out["x_next"], low_latent=inp["low_latent"], rrg_norm=norm,
                           rrg_weight=np.float32(437.5), **kw)
    return run, out


def moments_launcher(inp, P=None):
    ratio, ratio_low = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ws = ops.guidance_moments_workspace(B, C * HL * WL, C * H_LOW * W_LOW, "cuda")
    kw = {} if P is None else dict(region_w=inp["region_w"][P])
    g_out = inp["g_out"][P or 1]

    def run():
        ops.phase_moments(g_out, inp["v_out"], inp["x"].shape, inp["stamp"], inp["pick"], inp["cover"], inp["vp"].n_col_blocks,
                          (inp["gpad"].top, inp["gpad"].left), K, H_LOW, W_LOW, np.float32(10.0), ratio, ws, ratio_low=ratio_low, **kw)
    return run, {"ratio": ratio, "ratio_low": ratio_low}


def time_launches(opt, product, parent):
    sch = schedule.DDIMSchedule()
    coef = sch.step_coefficients(sch.set_timesteps(50)[7])
    inp = make_inputs()
    spec = {"assemble": (product, assemble_launcher(inp)), "assemble_n2": (product, assemble_launcher(inp, 2)),
            "assemble_n4": (product, assemble_launcher(inp, 4)), "epilogue": (product, epilogue_launcher(inp, coef)),
            **{f"epilogue_rg{P}": (product, epilogue_launcher(inp, coef, P)) for P in (1, 2, 3, 4)},
            "moments": (product, moments_launcher(inp)), "moments_rg3": (product, moments_launcher(inp, 3))}
    if parent is not None:
        spec = {"parent_assemble": (parent, assemble_launcher(inp)), "parent_epilogue": (parent, epilogue_launcher(inp, coef)), **spec}
    arms = {name: dict(lib=L, run=run, out=out, medians=[]) for name, (L, (run, out)) in spec.items()}
    try:
        for arm in arms.values():
            _hip._LIB = arm["lib"]
            for _ in range(10):  # warm-up: code object load, clocks
                arm["run"]()
        torch.cuda.synchronize()
        for _ in range(opt.rounds):
            for arm in arms.values():  # alternate the arms inside every round
                _hip._LIB = arm["lib"]
                arm["medians"].append(timed_us(arm["run"], opt.repeats, opt.inner))
    finally:
        _hip._LIB = product
    res = {"us_round_medians": {n: a["medians"] for n, a in arms.items()},
           "us": {n: statistics.median(a["medians"]) for n, a in arms.items()},
           "spread_us": {n: max(a["medians"]) - min(a["medians"]) for n, a in arms.items()},
           "model_rows_per_phase": {"assemble": 2 * K + inp["vp"].V, "assemble_n2": 2 * K + inp["vp"].V, "assemble_n4": 4 * K + inp["vp"].V}}
    same = lambda a, b: all(torch.equal(arms[a]["out"][k], arms[b]["out"][k]) for k in arms[a]["out"])  # noqa: E731
    res["assemble_n2_bit_identical_to_assemble"] = same("assemble_n2", "assemble")
    res["epilogue_rg1_bit_identical_to_epilogue"] = same("epilogue_rg1", "epilogue")
    if parent is not None:
        for kind in ("assemble", "epilogue"):
            res[f"{kind}_bit_identical_to_parent"] = same(kind, f"parent_{kind}")
            res[f"{kind}_minus_parent_us"] = res["us"][kind] - res["us"][f"parent_{kind}"]
            res[f"condition_{kind}_within_parent_spread"] = res[f"{kind}_minus_parent_us"] <= res["spread_us"][f"parent_{kind}"]
    return res


def time_images(opt):
    from bench import WORKLOADS
    from elasticdiffusion_official_amd import ElasticDiffusion
    wl = WORKLOADS["sdxl_1024x2048"]
    pipe = ElasticDiffusion(torch.device("cuda:0"), wl["sd"], view_batch_size=wl["vbs"], model_dtype=torch.float16)
    kw = dict(height=wl["H"], width=wl["W"], guidance_scale=wl["guidance"], resampling_steps=wl["R"], new_p=wl["new_p"],
              rrg_stop_t=wl["rrg_stop_t"], rrg_init_weight=wl["rrg_w"], cosine_scale=wl["cosine_scale"], repaint_sampling=True,
              output_type="pt", progress=lambda it: it)
    H, W = wl["H"], wl["W"]
    names = ["snowy mountains", "a harbour at dusk", "a pine forest"]
    rows = []
    for n in (0, 1, 2, 3):
        regions = None
        if n:
            regions = [(names[k], (k * W // n if n > 1 else W // 2, 0, (k + 1) * W // n, H)) for k in range(n)]
        extra = {} if regions is None else dict(regions=regions, region_blur=16.0)
        pipe.seed_everything(1)
        pipe.generate_image("An astronaut riding a corgi on the moon", "blurry, ugly", num_inference_steps=2, **kw, **extra)
        torch.cuda.synchronize()
        pipe.seed_everything(2)
        t0 = time.perf_counter()
        imgs, _ = pipe.generate_image("An astronaut riding a corgi on the moon", "blurry, ugly", num_inference_steps=opt.timesteps,
                                      **kw, **extra)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        row = {"regions": n, "model_rows_per_phase": [(wl["R"] + 1) * (2 + n) + 4, (2 + n) + 4], "s_per_image": round(sec, 3),
               "finite": bool(torch.isfinite(imgs).all())}
        rows.append(row)
        print(json.dumps(row))
    for row in rows:
        row["ratio_to_single_prompt"] = round(row["s_per_image"] / rows[0]["s_per_image"], 3)
    return {"workload": "sdxl_1024x2048", "timesteps": opt.timesteps, "images_timed_per_n": 1, "dtype": "fp16",
            "method": "one warm-up image of 2 timesteps, then host clock around one generate_image ending in a device synchronise",
            "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libelastic_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regional_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--no-images", action="store_true", help="launch timings only")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    product = _hip.lib()
    parent = load_library(opt.parent_lib) if opt.parent_lib else None
    result = {"device": torch.cuda.get_device_name(0),
              "geometry": dict(latent=[HL, WL], reduced=[H_LOW, W_LOW], model=MODEL, K=K, B=B, rows_dtype="float16"),
              "abi": {"this_tree": _hip.ABI_VERSION, "parent": None if parent is None else int(parent.ed_version())},
              "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner,
              "method": "HIP events around `inner` back-to-back launches on the current stream / inner; per round the median of "
                        "`repeats` such runs after 10 warm-up launches; arms alternated within each round; us = median of the "
                        "round medians, spread = max - min of them",
              "launches": time_launches(opt, product, parent)}
    print(json.dumps(result["launches"]))
    if not opt.no_images:
        result["images"] = time_images(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")
    la = result["launches"]
    if not (la["assemble_n2_bit_identical_to_assemble"] and la["epilogue_rg1_bit_identical_to_epilogue"]):
        raise SystemExit("the regional launches at P = 1 do not give the plain launches' bits")
    if not all(v for k, v in la.items() if k.endswith("_bit_identical_to_parent")):
        raise SystemExit("an unchanged launch of this tree does not give the parent's bits")


if __name__ == "__main__":
    main()
