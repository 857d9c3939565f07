"""Time of the 9-channel inpainting path on the MI355X.

    python tools/inpaint9_timing.py [--out profiles/inpaint9_timing.json] [--repeats 50] [--steps 50] [--skip-e2e]

``ed_assemble_rows_x`` (rows of 4 + 5 channels) against ``ed_assemble_rows`` (4 channels) at the row shapes of the headline workload
-- SDXL 1024 x 2048: latent 1x4x128x256, reduced latent 64x128, 128x128 model rows, fp16, K = 8 (first phase, R = 7) and K = 1
(RePaint phase) -- by HIP events around each ops call, 5 warm-up calls, median and minimum of ``--repeats`` (the method of
section 18.9), with the bytes each launch has to move.  Unless ``--skip-e2e``: the wall time of one whole image (50 steps, R = 7,
RePaint: 99 phases; ``generate_image`` with ``output_type="pt"``, synchronised) with the 9-channel and with the 4-channel full-width
SDXL UNet on the same init image and mask, random weights, the two arms alternated, two images per arm.  Needs the GPU.
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
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

from elasticdiffusion_official_amd import ElasticDiffusion, geometry, ops  # noqa: E402

H_PX, W_PX, SCALE, MODEL, E = 1024, 2048, 8, 128, 5


def _timed(fn, repeats, warmup=5):
    """-> (median us, min us) of the HIP-event time of fn() over ``repeats`` launches after ``warmup``"""
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


def assemble_rows(repeats, dtype=torch.float16, B=1, C=4):
    Hl, Wl = H_PX // SCALE, W_PX // SCALE
    h, w = geometry.reduced_size(H_PX, W_PX, "XL1.0", SCALE)
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, MODEL // 2, MODEL // 2, MODEL // 2)
    gpad, vpad = geometry.PadPlan(h, w, MODEL), geometry.PadPlan(vp.Sh, vp.Sw, MODEL)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    sr, sc, wy, wx = d(pp.src_row), d(pp.src_col), d(vp.win_y0), d(vp.win_x0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, Hl, Wl, generator=g).cuda()
    extra = torch.randn(B, E, Hl, Wl, generator=g).cuda()
    pad_value = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0]).cuda()
    gframe = torch.randn(C, gpad.PH, gpad.PW, generator=g).cuda() if gpad.padded else None
    vframe = torch.randn(C, vpad.PH, vpad.PW, generator=g).cuda() if vpad.padded else None
    out = []
    for K in (8, 1):
        idx = torch.randint(0, 4, (K, h * w), generator=g, dtype=torch.uint8).cuda()
        low = torch.empty(K, B, C, h, w, device="cuda")
        n_g, n_v = 2 * K * B, vp.V * B
        esz = torch.empty(0, dtype=dtype).element_size()
        row = {"K": K, "rows": n_g + n_v, "row_shape": [gpad.PH, gpad.PW], "views": vp.V, "reduced": [h, w]}
        for name, CT in (("ed_assemble_rows", C), ("ed_assemble_rows_x", C + E)):
            rows = torch.empty(n_g + n_v, CT, gpad.PH, gpad.PW, device="cuda", dtype=dtype)
            args = (x, idx, sr, sc, rows[:n_g], h, w, gpad.top, gpad.left, gframe, low, rows[n_g:], wy, wx, vp.Sh, vp.Sw, vpad.top,
                    vpad.left, vframe)
            fn = (lambda a=args: ops.assemble_rows(*a)) if CT == C else (lambda a=args: ops.assemble_rows_x(*a, extra, pad_value))
            med, mn = _timed(fn, repeats)
            # written: every row element once (+ low); read: one fp32 per distinct gathered element (each CFG pair shares its reads)
            elems = (n_g + n_v) * CT * gpad.PH * gpad.PW
            nbytes = elems * esz + 4 * (elems - (n_g // 2) * CT * gpad.PH * gpad.PW) + 4 * low.numel() + K * h * w
            row[name] = {"channels": CT, "bytes": int(nbytes), "us_median": med, "us_min": mn, "GBps_at_median": nbytes / med * 1e-3}
        row["x_over_plain_median"] = row["ed_assemble_rows_x"]["us_median"] / row["ed_assemble_rows"]["us_median"]
        out.append(row)
    return out


def e2e(steps, rounds=2):
    """seconds per image with the 9-channel and the 4-channel full-width SDXL UNet, same init image and mask, alternated"""
    kw = dict(height=H_PX, width=W_PX, num_inference_steps=steps, guidance_scale=10.0, resampling_steps=7, new_p=0.3, rrg_stop_t=0.2,
              rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True, output_type="pt", progress=lambda it: it)
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (H_PX, W_PX, 3), generator=g, dtype=torch.uint8).cuda()
    mask = torch.zeros(H_PX, W_PX, dtype=torch.uint8)
    mask[:, W_PX // 2:] = 255
    extra = dict(init_image=img, mask_image=mask.cuda())
    pipes = {"9-channel (XL1.0-inpaint)": ElasticDiffusion("cuda:0", "XL1.0-inpaint", view_batch_size=16, model_dtype=torch.float16),
             "4-channel (XL1.0)": ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)}
    for pipe in pipes.values():       # graphs captured, libraries warm
        pipe.seed_everything(0)
        pipe.generate_image("a photo", "", **dict(kw, num_inference_steps=2), **extra)
    times = {k: [] for k in pipes}
    for r in range(rounds):
        for name, pipe in pipes.items():
            pipe.seed_everything(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.generate_image("a photo", "", **kw, **extra)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    launches = {}
    for name, pipe in pipes.items():
        ops.TIMER.start()
        pipe.seed_everything(0)
        pipe.generate_latents("a photo", "", **{k: v for k, v in kw.items() if k != "output_type"}, **extra)
        launches[name] = {k: {"launches": v[0], "us_mean": v[1], "ms_total": v[2]} for k, v in ops.TIMER.stop().items()
                          if k in ("ed_assemble_rows", "ed_assemble_rows_x", "ed_phase_epilogue", "ed_inpaint_blend", "ed_u8_to_vae_input",
                                   "ed_u8_to_vae_input_masked", "ed_img2img_init", "ed_mask_to_latent")}
    a, b = (min(times[k]) for k in pipes)
    return {"steps": steps, "seconds_per_image": {k: {"runs": v, "min": min(v)} for k, v in times.items()},
            "nine_minus_four_seconds_min_vs_min": a - b, "per_kernel_under_the_timer": launches}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint9_timing.json"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--skip-e2e", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats,
              "method": "HIP events around each ops call on the current stream, warm-up 5, median and minimum of the repeats; bytes = "
                        "what the launch must read and write; end to end: wall time of generate_image incl. decode, synchronised, "
                        "random weights, arms alternated, two images per arm",
              "assemble_rows": assemble_rows(opt.repeats)}
    print(json.dumps(result["assemble_rows"]))
    if not opt.skip_e2e:
        result["end_to_end"] = e2e(opt.steps)
        print(json.dumps(result["end_to_end"]))
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
