"""Cost of a change of LoRA scale on the MI355X.

    python tools/lora_timing.py [--out profiles/lora_timing.json] [--rounds 7] [--ranks 16 128] [--skip-e2e]

Full-width SDXL UNet, random weights, fp16; a synthetic adapter over every attention projection (to_q, to_k, to_v, to_out.0 of
attn1 and attn2) and both feed-forward projections (ff.net.0.proj, ff.net.2) at each rank.  Two arms on the SAME tensors (the
pristine bases, fp32 factors and Parameters of one ``lora.LoraState``), alternated in one process, two warm-up passes each:

  (a) ``LoraState.set_scale``: the table rebuilt on the host, one host-to-device copy, ONE ``ed_lora_merge`` launch;
  (b) per tensor ``W.copy_((base.float() + c * (up @ down)).to(W.dtype))`` -- what the merge is in torch ops.

Each window is bracketed by HIP events on the current stream and ends in a device synchronise; the host clock around the same
window is recorded next to it (arm (a) includes its host work: the window is what a caller waits for).  Median, minimum and
maximum of ``--rounds``; ``torch.cuda.max_memory_allocated`` above the resident set of each arm; for (a) the bytes and FLOPs the
merge needs and the roof that bounds it (peaks of the MI355X: 157.3 TFLOP/s fp32 vector, 8 TB/s HBM).  The two arms' results
are compared element by element once.  Unless ``--skip-e2e``: on the reduced-width SD 1.5 UNet at 512 x 1024 (the geometry the
suite's loop tests use), the wall time of the first image after a change of scale (graphs re-captured, derived weights rebuilt)
next to a warm image.  Needs the GPU.
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
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

from elasticdiffusion_official_amd import ElasticDiffusion, lora, models  # noqa: E402

DEV = "cuda:0"
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
PROJECTIONS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
               "ff.net.0.proj", "ff.net.2")


def full_unet(fam="sdxl", dtype=torch.float16):
    cfg = models.unet_config(fam)
    with torch.device("meta"):
        unet = models.UNet2DConditionModel(**cfg)
    unet = unet.to_empty(device=DEV)
    models._seeded_init(unet, 0)
    unet = unet.to(dtype=dtype).eval().requires_grad_(False)
    if models.CHANNELS_LAST:
        unet = unet.to(memory_format=torch.channels_last)
    return cfg, unet


def synthetic_adapter(unet, rank, seed=0):
    """a PEFT-spelled state dict, generated on the device (fp16 factors, as adapter files carry them)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    sd = {}
    for name, m in lora.lora_modules(unet).items():
        if name.endswith(PROJECTIONS) and isinstance(m, torch.nn.Linear):
            N, K = m.weight.shape
            sd[f"unet.{name}.lora_B.weight"] = (torch.randn(N, rank, device=DEV, generator=g) * 0.02).half()
            sd[f"unet.{name}.lora_A.weight"] = (torch.randn(rank, K, device=DEV, generator=g) * 0.02).half()
    return sd


def _window(fn):
    """-> (HIP-event ms, host ms) of fn() followed by a device synchronise"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * (time.perf_counter() - t0)


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


@torch.no_grad()
def merge_arms(unet, cfg, rank, rounds):
    state = lora.LoraState({"unet": unet}, torch.device(DEV), cfg)
    state.load(synthetic_adapter(unet, rank), 1.0, name="synthetic")
    items = state.adapters[0]["items"]
    bases = {id(w): base for _, w, base in state.bases.values()}
    scales = [0.7, 0.9]

    def arm_a(i):
        state.set_scale(scales[i % 2])

    def arm_b(i):
        for _, w, up, down, alpha, r in items:
            c = float(lora.coefficient(scales[i % 2], alpha, r))
            w.copy_((bases[id(w)].float() + c * (up @ down)).to(w.dtype))

    for i in range(2):
        arm_a(i)
        arm_b(i)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    ev = {"a": [], "b": []}
    host = {"a": [], "b": []}
    peak = {}
    for i in range(rounds):
        for name, arm in (("a", arm_a), ("b", arm_b)):
            torch.cuda.reset_peak_memory_stats()
            e, h = _window(lambda: arm(i))
            ev[name].append(e)
            host[name].append(h)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - resident)
    # arm (a) again under the wrappers' timer: HIP events around the ed_lora_merge call alone (launch + kernel, no host table work)
    from elasticdiffusion_official_amd import ops
    ops.TIMER.start()
    for i in range(rounds):
        arm_a(i)
        torch.cuda.synchronize()
    launches, kernel_us, _ = ops.TIMER.stop()["ed_lora_merge"]
    # the same scale through both arms: how far apart are the results?
    arm_a(0)
    torch.cuda.synchronize()
    got = [w.detach().clone() for _, w, *_ in items]
    arm_b(0)
    torch.cuda.synchronize()
    n = sum(w.numel() for w in got)
    differing = sum(int((a != w).sum()) for a, (_, w, *_) in zip(got, items))
    table = state.table("unet")
    t_flops, t_bytes = table.flops / PEAK_FLOPS, table.nbytes / PEAK_BYTES
    med_a = statistics.median(ev["a"])
    out = {"rank": rank, "tensors": len(items), "elements": n, "tiles": table.n_tiles,
           "a_set_lora_scale_ms": {"hip_events": _stats(ev["a"]), "host_clock": _stats(host["a"])},
           "b_torch_sequence_ms": {"hip_events": _stats(ev["b"]), "host_clock": _stats(host["b"])},
           "a_ed_lora_merge_alone_ms_mean": {"launches": launches, "ms": 1e-3 * kernel_us},
           "b_over_a_median_hip_events": statistics.median(ev["b"]) / med_a,
           "peak_bytes_above_resident": peak,
           "a_needs": {"flops": table.flops, "bytes": table.nbytes, "ms_at_fp32_vector_peak": 1e3 * t_flops, "ms_at_hbm_peak": 1e3 * t_bytes,
                       "bound_by": "fp32 vector rate" if t_flops > t_bytes else "HBM bandwidth",
                       "share_of_that_roof_window_median": 1e3 * max(t_flops, t_bytes) / med_a,
                       "share_of_that_roof_launch_alone": 1e3 * max(t_flops, t_bytes) / (1e-3 * kernel_us)},
           "elements_differing_between_arms": differing, "fraction_differing": differing / n}
    state.unload()
    return out


def e2e(rounds=3):
    """reduced-width SD 1.5 at 512 x 1024: seconds of the first image after set_lora_scale against a warm image"""
    unet, vae = models.build_models("1.5", device=DEV, small=True)
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=unet, vae=vae)
    kw = dict(height=512, width=1024, num_inference_steps=3, guidance_scale=10.0, resampling_steps=2, new_p=0.3, rrg_stop_t=0.2,
              rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)
    g = torch.Generator().manual_seed(1)
    sd = {}
    for name, m in lora.lora_modules(pipe.unet).items():
        if name.endswith(PROJECTIONS) and isinstance(m, torch.nn.Linear):
            N, K = m.weight.shape
            sd[f"unet.{name}.lora_B.weight"], sd[f"unet.{name}.lora_A.weight"] = torch.randn(N, 8, generator=g) * 0.05, torch.randn(8, K, generator=g) * 0.05
    pipe.load_lora(sd, 1.0, name="synthetic")

    def image():
        pipe.seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.generate_latents("a photo", "", **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    image(), image()
    first, warm = [], []
    for i in range(rounds):
        pipe.set_lora_scale(0.5 + 0.1 * i)
        first.append(image())
        warm.append(image())
    return {"geometry": "SD 1.5 reduced width, 512 x 1024, 3 steps, R = 2, fp16", "tensors": pipe.loras[0][2],
            "first_image_after_set_lora_scale_s": _stats(first), "warm_image_s": _stats(warm)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--skip-e2e", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds,
              "method": "full-width SDXL UNet, fp16, random weights; arms alternated in one process on the same tensors, 2 warm-up passes "
                        "each; every window bracketed by HIP events and ended by a device synchronise, host clock around the same window",
              "merge": []}
    cfg, unet = full_unet()
    for rank in opt.ranks:
        result["merge"].append(merge_arms(unet, cfg, rank, opt.rounds))
        print(json.dumps(result["merge"][-1]), flush=True)
    del unet
    torch.cuda.empty_cache()
    if not opt.skip_e2e:
        result["end_to_end"] = e2e()
        print(json.dumps(result["end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
