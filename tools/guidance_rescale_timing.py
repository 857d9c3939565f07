"""Cost of ``guidance_rescale`` on the MI355X: the per-phase latent-space glue and whole images, 0.7 against 0.

    python tools/guidance_rescale_timing.py [--out profiles/guidance_rescale_cost.json] [--rounds 5] [--repeats 20]
                                            [--inner 20] [--timesteps 50] [--images 2] [--no-images]

Geometry: the SDXL 1024 x 2048 headline (latent 128 x 256, reduced 64 x 128, model size 128, 8 views), one prompt, fp16
model rows; K = 8 (the first phase of a timestep) and K = 1 (its RePaint phase), with the fused RRG term and without.

Glue arms, alternated within every round (the model call between the two halves is excluded):

    off   ed_assemble_rows -> ed_phase_epilogue                             (guidance_rescale = 0: the loop as it was)
    on    ed_assemble_rows -> ed_phase_moments -> ed_phase_epilogue_gr      (guidance_rescale = 0.7)

and, on their own, ``epilogue`` (ed_phase_epilogue), ``epilogue_gr`` and ``moments`` (ed_phase_moments = the reduction
launch + the finalising launch).  One run = HIP events around ``--inner`` back-to-back repetitions on the current stream,
divided by ``--inner``; per round and arm the MEDIAN of ``--repeats`` runs after warm-up; the figure is the median of the
round medians, the spread max - min of them.  At a few MB per launch these figures are the rate at which the Python
wrappers enqueue, an upper bound of the device time.

Images: ``ElasticDiffusion("XL1.0")`` (random weights, fp16, hipGraph forward) at 1024 x 2048, the benchmark's loop
settings, ``--timesteps`` denoising steps, seconds per image from HIP events around ``generate_latents``; the two arms
alternate, ``--images`` images each after one warm-up image per arm.  Needs the GPU: there is no fallback.
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

from elasticdiffusion_official_amd import geometry, host_rng, ops, schedule  # noqa: E402

HL, WL, H_LOW, W_LOW, MODEL, B, C = 128, 256, 64, 128, 128, 1, 4
GR = 0.7


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def make_phase(K, dtype=torch.float16, seed=0):
    ws = MODEL // 2
    pp, vp = geometry.PickPlan(HL, WL, H_LOW, W_LOW), geometry.ViewPlan(HL, WL, ws, ws, MODEL - ws)
    gpad, vpad = geometry.PadPlan(H_LOW, W_LOW, MODEL), geometry.PadPlan(vp.Sh, vp.Sw, MODEL)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    stamp = torch.empty(H_LOW * W_LOW, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(H_LOW * W_LOW).draw(K, 0.7, lambda: None, stamp=stamp)
    T = {k: dev_i32(getattr(pp, k)) for k in ("src_row", "src_col", "inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")}
    n_g, n_v = 2 * K * B, vp.V * B
    rows = torch.empty(n_g + n_v, C, gpad.PH, gpad.PW, dtype=dtype).cuda()
    return dict(
        K=K, x=torch.randn(B, C, HL, WL, generator=g).cuda(), stamp=stamp.cuda(), idx=idx.cuda(), T=T,
        pick=tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")),
        cover=tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left)), win=(dev_i32(vp.win_y0), dev_i32(vp.win_x0)),
        view=(vp.Sh, vp.Sw, vpad.top, vpad.left), rows=rows, n_g=n_g,
        g_out=torch.randn(n_g, C, gpad.PH, gpad.PW, generator=g).to(dtype).cuda(),
        v_out=torch.randn(n_v, C, vpad.PH, vpad.PW, generator=g).to(dtype).cuda(),
        low=torch.empty(K, B, C, H_LOW, W_LOW).cuda(), ncb=vp.n_col_blocks, g_off=(gpad.top, gpad.left), views=vp.V)


def arms_of(p, coef, rrg):
    x, K = p["x"], p["K"]
    out = {k: torch.empty_like(x) for k in ("prev", "x0", "x_next")}
    low_dir, unc = torch.empty_like(p["low"][0]), torch.empty_like(p["low"][0])
    norm = np.float32(2.0 / (C * HL * WL))
    ratio, ratio_low = torch.empty(B).cuda(), torch.empty(B).cuda()
    wsp = ops.guidance_moments_workspace(B, C * HL * WL, C * H_LOW * W_LOW, x.device)
    geo = (p["ncb"], p["g_off"], K, H_LOW, W_LOW, np.float32(10.0))
    rrg_kw = dict(x_next=out["x_next"], low_latent=p["low"][K - 1], rrg_norm=norm, rrg_weight=np.float32(437.5)) if rrg else {}

    def assemble():
        T = p["T"]
        ops.assemble_rows(x, p["idx"], T["src_row"], T["src_col"], p["rows"][:p["n_g"]], H_LOW, W_LOW, *p["g_off"], None,
                          p["low"], p["rows"][p["n_g"]:], *p["win"], *p["view"], None)

    def moments():
        ops.phase_moments(p["g_out"], p["v_out"], x.shape, p["stamp"], p["pick"], p["cover"], *geo, ratio, wsp,
                          ratio_low=ratio_low if rrg else None)

    def epilogue(**kw):
        ops.phase_epilogue(p["g_out"], p["v_out"], x, p["stamp"], p["pick"], p["cover"], *geo, coef, out["prev"], out["x0"],
                           low_dir=low_dir, uncond_last=unc, **rrg_kw, **kw)

    def epilogue_gr():
        epilogue(ratio=ratio, ratio_low=ratio_low if rrg else None, guidance_rescale=GR)

    return {"off": lambda: (assemble(), epilogue()), "on": lambda: (assemble(), moments(), epilogue_gr()),
            "epilogue": epilogue, "epilogue_gr": epilogue_gr, "moments": moments}


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


def glue_rows(opt):
    sch = schedule.DDIMSchedule()
    coef = sch.step_coefficients(sch.set_timesteps(50)[7])
    rows = []
    for K in (8, 1):
        p = make_phase(K)
        for rrg in (True, False):
            arms = arms_of(p, coef, rrg)
            for run in arms.values():
                for _ in range(10):
                    run()
            torch.cuda.synchronize()
            med = {n: [] for n in arms}
            for _ in range(opt.rounds):
                for n, run in arms.items():
                    med[n].append(timed_us(run, opt.repeats, opt.inner))
            row = {"K": K, "rrg_fused": rrg, "us": {n: statistics.median(v) for n, v in med.items()},
                   "spread_us": {n: max(v) - min(v) for n, v in med.items()}, "us_round_medians": med}
            row["on_minus_off_us"] = row["us"]["on"] - row["us"]["off"]
            row["moments_over_epilogue"] = row["us"]["moments"] / row["us"]["epilogue"]
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "us_round_medians"}))
    return rows


def image_rows(opt):
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
    kw = dict(height=1024, width=2048, num_inference_steps=opt.timesteps, guidance_scale=10.0, resampling_steps=7, new_p=0.3,
              rrg_stop_t=0.2, rrg_init_weight=1000, cosine_scale=10.0)
    secs, finite = {0.0: [], GR: []}, {0.0: True, GR: True}
    for i in range(opt.images + 1):          # image 0 of each arm: warm-up (graph capture, kernel load)
        for gr in secs:
            pipe.seed_everything(i)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            z = pipe.generate_latents("a photo", "", guidance_rescale=gr, **kw)
            b.record()
            b.synchronize()
            if i:
                secs[gr].append(1e-3 * a.elapsed_time(b))
            finite[gr] = finite[gr] and bool(torch.isfinite(z).all())
    row = {"timesteps": opt.timesteps, "images_per_arm": opt.images, "seconds_per_image": {str(k): v for k, v in secs.items()},
           "median_s": {str(k): statistics.median(v) for k, v in secs.items()},
           "latents_finite": {str(k): v for k, v in finite.items()}}
    row["on_over_off"] = row["median_s"][str(GR)] / row["median_s"]["0.0"]
    print(json.dumps(row))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_rescale_cost.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--no-images", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "guidance_rescale": GR,
              "geometry": dict(latent=[HL, WL], reduced=[H_LOW, W_LOW], model=MODEL, B=B, rows_dtype="float16"),
              "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner,
              "method": "HIP events around `inner` back-to-back repetitions on the current stream / inner; per round the median "
                        "of `repeats` such runs after 10 warm-up repetitions; arms alternated within each round; us = median of "
                        "the round medians, spread = max - min of them (enqueue-rate figures: an upper bound of device time)",
              "glue": glue_rows(opt)}
    if not opt.no_images:
        result["images"] = image_rows(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
