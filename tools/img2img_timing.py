"""Time of the image-to-image / inpainting pieces on the MI355X.

    python tools/img2img_timing.py [--out profiles/img2img_timing.json] [--repeats 50] [--steps 50] [--skip-e2e]

Per launch, by HIP events after warm-up (median and minimum of ``--repeats`` launches), with the bytes each kernel has to move and the
GB/s that implies: ed_u8_to_vae_input, ed_img2img_init, ed_mask_to_latent, ed_inpaint_blend (noised and clean) at the SDXL
1024 x 2048 sizes (latent 1x4x128x256, pixels 1024x2048x3) and at 2048 x 2048.  Next to them the fp32 VAE *encode* of one image of
both sizes (full-width SDXL architecture, random weights), and -- unless ``--skip-e2e`` -- the headline single image (SDXL
1024 x 2048, fp16, 50 steps, R = 7, RePaint: 99 phases) generated plainly and with ``init_image`` + ``mask_image`` at strength 1 in
the same process, alternated, so that what the feature adds per image is a difference of two numbers measured side by side.
Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # encoder shapes without a find-db record must not start a minutes-long search

from elasticdiffusion_official_amd import ElasticDiffusion, ops  # noqa: E402

SIZES = [(1024, 2048), (2048, 2048)]


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


def _row(name, nbytes, med, mn):
    return {"kernel": name, "bytes": int(nbytes), "us_median": med, "us_min": mn, "GBps_at_median": nbytes / med * 1e-3}


def kernel_rows(H, W, repeats, vae_dtype=torch.float32, s=8):
    g = torch.Generator().manual_seed(H + W)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    mask_px = (torch.randint(0, 2, (H, W), generator=g, dtype=torch.uint8) * 255).cuda()
    shape = (1, 4, H // s, W // s)
    n = 4 * (H // s) * (W // s)
    mean, std, eps, noise, x = (torch.randn(shape, generator=g).cuda() for _ in range(5))
    z0, xo = torch.empty_like(x), torch.empty_like(x)
    m = ops.mask_to_latent(mask_px, s)
    out = torch.empty_like(x)
    rows = [
        _row("ed_u8_to_vae_input", 3 * H * W * (1 + 4), *_timed(lambda: ops.u8_to_vae_input(img, vae_dtype), repeats)),
        _row("ed_img2img_init", n * 24, *_timed(lambda: ops.img2img_init(mean, std, eps, noise, 0.13025, 0.6, 0.8, z0=z0, x=xo), repeats)),
        _row("ed_mask_to_latent", 2 * n // 4, *_timed(lambda: ops.mask_to_latent(mask_px, s), repeats)),
        _row("ed_inpaint_blend", n * 16 + n // 4, *_timed(lambda: ops.inpaint_blend(x, m, z0, noise, 0.6, 0.8, out=out), repeats)),
        _row("ed_inpaint_blend(clean)", n * 12 + n // 4, *_timed(lambda: ops.inpaint_blend(x, m, z0, None, 1.0, 0.0, out=out, clean=True), repeats)),
        _row("torch.empty_like (allocation only, for scale)", 0, *_timed(lambda: torch.empty_like(x), repeats)),
    ]
    return {"H": H, "W": W, "latent": list(shape), "rows": rows}


def encode_ms(pipe, H, W, repeats=3):
    vdt = next(pipe.vae.parameters()).dtype
    g = torch.Generator().manual_seed(1)
    pix = ops.u8_to_vae_input(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda(), vdt)
    with torch.no_grad():
        med, mn = _timed(lambda: pipe.vae.encode(pix).latent_dist, repeats, warmup=1)
    return {"H": H, "W": W, "ms_median": med * 1e-3, "ms_min": mn * 1e-3}


def e2e(pipe, steps, rounds=2):
    """seconds per image (generate_image, output_type='pt', synchronised), plain and with init + mask, alternated"""
    H, W = SIZES[0]
    kw = dict(height=H, width=W, num_inference_steps=steps, guidance_scale=10.0, resampling_steps=7, new_p=0.3, rrg_stop_t=0.2,
              rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True, output_type="pt", progress=lambda it: it)
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    mask = torch.zeros(H, W, dtype=torch.uint8)
    mask[:, W // 2:] = 255
    variants = {"plain": {}, "init_image": dict(init_image=img), "init_image+mask_image": dict(init_image=img, mask_image=mask.cuda())}
    pipe.seed_everything(0)
    pipe.generate_image("a photo", "", **dict(kw, num_inference_steps=2), **variants["init_image+mask_image"])   # graphs captured, warm
    times = {k: [] for k in variants}
    launches = {}
    for r in range(rounds):
        for name, extra in variants.items():
            pipe.seed_everything(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.generate_image("a photo", "", **kw, **extra)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    ops.TIMER.start()
    pipe.seed_everything(0)
    pipe.generate_latents("a photo", "", **{k: v for k, v in kw.items() if k not in ("output_type",)}, **variants["init_image+mask_image"])
    for k, v in ops.TIMER.stop().items():
        if k in ("ed_u8_to_vae_input", "ed_img2img_init", "ed_mask_to_latent", "ed_inpaint_blend", "ed_phase_epilogue", "ed_assemble_rows"):
            launches[k] = {"launches": v[0], "us_mean": v[1], "ms_total": v[2]}
    return {"steps": steps, "seconds_per_image": {k: {"runs": v, "min": min(v)} for k, v in times.items()},
            "added_seconds_min_vs_min": {k: min(v) - min(times["plain"]) for k, v in times.items() if k != "plain"},
            "per_kernel_under_the_timer": launches}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "img2img_timing.json"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-encode", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats,
              "method": "HIP events around each ops call on the current stream (so each figure includes the wrapper's output "
                        "allocation where it has one), warm-up 5, median and minimum of the repeats; bytes = what the kernel must "
                        "read and write; end to end: wall time of generate_image incl. decode, synchronised, variants alternated",
              "kernels": [kernel_rows(H, W, opt.repeats) for H, W in SIZES]}
    for k in result["kernels"]:
        print(json.dumps(k))
    if not (opt.skip_encode and opt.skip_e2e):
        pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
        if not opt.skip_encode:
            result["vae_encode"] = [encode_ms(pipe, H, W) for H, W in SIZES]
            print(json.dumps(result["vae_encode"]))
        if not opt.skip_e2e:
            result["end_to_end"] = e2e(pipe, opt.steps)
            print(json.dumps(result["end_to_end"]))
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
