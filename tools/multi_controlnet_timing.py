"""Cost of the Multi-ControlNet hand-off on the MI355X.

    python tools/multi_controlnet_timing.py [--out profiles/multi_controlnet_timing.json] [--steps 10] [--rounds 3]
                                            [--skip-images] [--skip-kernel]

(a) The hand-off alone: ONE ``ed_control_residuals`` launch against the torch op sequence it replaces (per net and level one
    ``r * scale``, then N - 1 adds per level, then ``skip + sum``), for N = 1, 2, 3 nets at the SDXL skip shapes of a 128 x 128
    model row (nine skips + the mid block, fp16 channels-last) with 40 and with 12 batch rows.  The method of section 18.9: HIP
    events around each call on the current stream, 5 warm-up calls, the median (and minimum) of 50.
(b) Whole images, SDXL + ControlNet at 1024 x 2048 (seeded weights), four arms alternated inside every round of one process:
      legacy        one net given as such, a scalar scale: the path as it always was
      list_of_one   the same net as a list of one: the multi path (raw residuals, the one launch, weights on the device)
      two_nets      two nets, both open on every step
      two_nets_half two nets, the second released after half the steps (control_guidance_end = [1.0, 0.5])
    seconds per image from HIP events around ``generate_latents`` after one warm-up image per arm (graph captures, MIOpen finds).
    The condition the project sets: list_of_one may be slower than legacy by no more than legacy's own run-to-run spread (max - min
    over the rounds) in this run.  Everything else is reported as it comes.

Needs the GPU: there is no fallback.  Without one the file is written with every number ``null`` and ``"measured": false``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, side) of the SDXL UNet's nine skips and its mid-block output for a 128 x 128 model row
SDXL_LEVELS = [(320, 128)] * 3 + [(320, 64)] + [(640, 64)] * 2 + [(640, 32)] + [(1280, 32)] * 2 + [(1280, 32)]


def timed_ms(fn, warmup=5, repeats=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def kernel_rows():
    from elasticdiffusion_official_amd import ops
    rows = []
    for B in (40, 12):
        mk = lambda: [torch.randn(B, c, s, s, device="cuda", dtype=torch.float16).contiguous(memory_format=torch.channels_last)  # noqa: E731
                      for c, s in SDXL_LEVELS]
        skips = mk()
        nets = [mk() for _ in range(3)]
        outs = [torch.empty_like(s) for s in skips]
        elems = sum(s.numel() for s in skips)
        for N in (1, 2, 3):
            scales = [0.3 + 0.2 * n for n in range(N)]
            w = torch.tensor([scales] * B, dtype=torch.float32, device="cuda")

            def fused():
                ops.control_residuals(skips, nets[:N], w, outs)

            def torch_sequence():
                scaled = [[r * sc for r in nets[n]] for n, sc in enumerate(scales)]
                total = scaled[0]
                for more in scaled[1:]:
                    total = [a + b for a, b in zip(total, more)]
                return [s + r for s, r in zip(skips, total)]

            f_med, f_min = timed_ms(fused)
            t_med, t_min = timed_ms(torch_sequence)
            row = {"batch_rows": B, "nets": N, "levels": len(SDXL_LEVELS), "elements": elems,
                   "fused_ms_median": f_med, "fused_ms_min": f_min, "torch_ms_median": t_med, "torch_ms_min": t_min,
                   "fused_bytes": 2 * elems * (2 + N), "torch_launches": len(SDXL_LEVELS) * (2 * N), "fused_launches": 1,
                   "fused_share_of_hbm_roof": 2 * elems * (2 + N) / 8e12 / (f_med * 1e-3)}
            rows.append(row)
            print(json.dumps(row))
        del skips, nets, outs
        torch.cuda.empty_cache()
    return rows


def image_rows(steps, rounds):
    from elasticdiffusion_official_amd import ElasticDiffusionControlNet
    from elasticdiffusion_official_amd.models import build_controlnet, build_models
    dev = torch.device("cuda", torch.cuda.current_device())
    unet, vae, cn0 = build_models("XL1.0", device=dev, controlnet=True)
    cn1 = build_controlnet("XL1.0", dev, index=1)
    H, W = 1024, 2048

    common = dict(unet=unet, vae=vae, view_batch_size=16)  # (no CLIP weights: the pipeline's synthetic prompt embeddings)
    single = ElasticDiffusionControlNet(dev, "XL1.0", "canny", controlnet=cn0, **common)
    one = ElasticDiffusionControlNet(dev, "XL1.0", ["canny"], controlnet=[cn0], **common)
    two = ElasticDiffusionControlNet(dev, "XL1.0", ["canny", "depth"], controlnet=[cn0, cn1], **common)
    h, w = single.get_downsample_size(H, W)
    s = single.vae_scale_factor
    g = torch.Generator().manual_seed(9)
    conds = [torch.rand(1, 3, h * s, w * s, generator=g) for _ in range(2)]
    kw = dict(height=H, width=W, num_inference_steps=steps, resampling_steps=7)
    arms = {
        "legacy": (single, dict(condition_image=conds[0], controlnet_conditioning_scale=0.5)),
        "list_of_one": (one, dict(condition_image=[conds[0]], controlnet_conditioning_scale=[0.5])),
        "two_nets": (two, dict(condition_image=conds, controlnet_conditioning_scale=[0.5, 0.3])),
        "two_nets_half": (two, dict(condition_image=conds, controlnet_conditioning_scale=[0.5, 0.3],
                                    control_guidance_end=[1.0, 0.5])),
    }

    def image(pipe, extra):
        pipe.seed_everything(0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        z = pipe.generate_latents("a photo", "", **kw, **extra)
        b.record()
        b.synchronize()
        assert bool(torch.isfinite(z).all())
        return a.elapsed_time(b) * 1e-3

    seconds = {name: [] for name in arms}
    for name, (pipe, extra) in arms.items():  # warm-up: captures and library searches
        image(pipe, extra)
    for _ in range(rounds):
        for name, (pipe, extra) in arms.items():  # alternate the arms inside every round
            seconds[name].append(image(pipe, extra))
    out = {"steps": steps, "resampling_steps": 7, "size": [H, W], "rounds": rounds, "seconds": seconds,
           "median_s": {n: statistics.median(v) for n, v in seconds.items()},
           "spread_s": {n: max(v) - min(v) for n, v in seconds.items()},
           "graphs": {n: arms[n][0]._runner.stats() for n in arms}}
    out["list_of_one_minus_legacy_s"] = out["median_s"]["list_of_one"] - out["median_s"]["legacy"]
    out["condition_list_of_one_within_legacy_spread"] = out["list_of_one_minus_legacy_s"] <= out["spread_s"]["legacy"]
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_controlnet_timing.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-images", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    opt = ap.parse_args(argv)
    method = ("(a) HIP events around each call on the current stream, 5 warm-up calls, median and minimum of 50 (DESIGN.md section "
              "18.9); (b) HIP events around generate_latents, one warm-up image per arm, arms alternated inside every round, "
              "median and max - min over the rounds")
    if not torch.cuda.is_available():
        result = {"measured": False, "method": method, "handoff": None, "images": None}
    else:
        with torch.no_grad():
            result = {"measured": True, "device": torch.cuda.get_device_name(0), "method": method,
                      "handoff": None if opt.skip_kernel else kernel_rows(),
                      "images": None if opt.skip_images else image_rows(opt.steps, opt.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")
    if result.get("images") and not result["images"]["condition_list_of_one_within_legacy_spread"]:
        raise SystemExit("the list-of-one arm is slower than the legacy arm by more than the legacy arm's own spread")


if __name__ == "__main__":
    main()
