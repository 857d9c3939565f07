"""Pad-strip VAE encodes with models.VAE_NARROW_CONSTANT off and on, in one process on the MI355X.

    python tools/strip_encode_timing.py [--out profiles/strip_encode_timing.json] [--reps 5] [--timesteps 50] [--bench-json LABEL=FILE ...]
    python tools/strip_encode_timing.py --add-full-run FILE [--parent-full-run profiles/bench_r6_final2_1gpu.json]     (no GPU)

For the flagship geometry (SDXL 1024 x 2048: two 32 x 128-latent strips, 256 x 1024 px each) and cfg2's (SD 1.5 512 x 1024: 16 x 64
latents) the full-width fp32 VAE encodes one image's strips through ``ElasticDiffusion._strip_frames`` (a stand-in UNet: it is never
called).  The narrowed arm runs FIRST, so its first VAE call is the first convolution of a fresh process: ``first_call_ms`` (wall
clock, synchronised) would show a MIOpen find.  Then per arm: VAE calls per image, ms per call (HIP events around every call), ms per
image's strips (HIP events around ``_strip_frames``, median of ``--reps`` after one warm-up), and the rel-L2 between the two arms'
frames.  ``call_shapes`` lists the one batch a rank issues on 1, 2, 4 and 8 ranks and times one call of each (with ED_MIOPEN_FIND=1
this is the run that records those shapes in miopen_cache/).  ``--bench-json label=FILE`` copies `value` and
`phase_ms_last_image.setup_done` of bench.py result lines into the report (the alternated parent / tree runs).  The measurement needs
the GPU: there is no fallback.  ``--add-full-run FILE`` measures nothing: it adds the live fp32 leg of a ``bench.py --gpus 1 --full`` output
of this tree (`tolerance.fp32_unet_same_workload`: `meets_1e-3`, `worst_rel_l2`) to the report that ``--out`` names, next to the parent's.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import ElasticDiffusion, geometry, models  # noqa: E402

GEOMETRIES = {"flagship_sdxl_1024x2048": ("XL1.0", 1024, 2048), "cfg2_sd15_512x1024": ("1.5", 512, 1024)}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return out, (a, b)


def build_pipe(sd, dev):
    fam = models.family(sd)
    with torch.device("meta"):
        vae = models.AutoencoderKL(scaling_factor=0.13025 if fam == "sdxl" else 0.18215, force_upcast=(fam == "sdxl"))
    vae = vae.to_empty(device=dev)
    models._seeded_init(vae, 1)
    vae = vae.eval().requires_grad_(False)
    unet = torch.nn.Conv2d(4, 4, 1)     # the stand-in: the pipeline reads its sample size, nothing here calls it
    unet.config = SimpleNamespace(sample_size=128 if fam == "sdxl" else 64, in_channels=4)
    return ElasticDiffusion(dev, sd, unet=unet, vae=vae, text_encoder=lambda *a, **k: None, use_graphs=False)


def measure(name, sd, H, W, T, reps, dev):
    pipe = build_pipe(sd, dev)
    h, w = geometry.reduced_size(H, W, sd)
    pad = geometry.PadPlan(h, w, pipe.model_size)
    ts = list(pipe.scheduler.set_timesteps(T))
    calls = []
    for attr in ("encode", "encode_constant"):
        def wrapped(*a, _f=getattr(pipe.vae, attr), _n=attr, **k):
            if _n == "encode" and calls and calls[-1][0] == "encode_constant" and calls[-1][2] is None:
                return _f(*a, **k)                        # encode_constant declining into encode: one call, not two
            rec = [_n, tuple(a[0].shape), None]
            calls.append(rec)
            out, rec[2] = timed(lambda: _f(*a, **k))
            return out
        setattr(pipe.vae, attr, wrapped)
    rep = {"strips": [s[2:4] for s in pad.strips], "timesteps": T}
    frames = {}
    for on in (True, False):
        models.VAE_NARROW_CONSTANT = on
        arm = "narrowed" if on else "full"
        pipe.seed_everything(0)
        del calls[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames[on] = pipe._strip_frames(pad, ts, 4).clone()
        torch.cuda.synchronize()
        first_image_ms = 1e3 * (time.perf_counter() - t0)
        first_call_ms = calls[0][2][0].elapsed_time(calls[0][2][1])
        per_image, per_call = [], []
        for _ in range(reps):
            del calls[:]
            pipe.seed_everything(0)
            _, ev = timed(lambda: pipe._strip_frames(pad, ts, 4))
            torch.cuda.synchronize()
            per_image.append(ev[0].elapsed_time(ev[1]))
            per_call += [c[2][0].elapsed_time(c[2][1]) for c in calls]
        rep[arm] = {"calls_per_image": len(calls), "call_shape": list(calls[0][1]), "first_image_ms_wall": round(first_image_ms, 1),
                    "first_call_ms": round(first_call_ms, 1), "ms_per_call_median": round(statistics.median(per_call), 3),
                    "ms_per_image_strips_median": round(statistics.median(per_image), 2),
                    "ms_per_image_strips_all": [round(v, 2) for v in per_image]}
    rep["rel_l2_narrowed_vs_full"] = rel_l2(frames[True], frames[False])
    # the one call shape of every rank count: colours [group * chunk, 3] at the strip size
    models.VAE_NARROW_CONSTANT = True
    Hs, Ws = pad.strips[0][2:4]
    s = pipe.vae_scale_factor
    chunk = pipe._strip_chunk(Hs, Ws, T)
    n_units = len(pad.strips) * -(-T // chunk)
    real = pipe.sharder
    shapes = {}
    for ranks in (1, 2, 4, 8):
        pipe.sharder = SimpleNamespace(world_size=ranks, exchange=ranks > 1)
        group = pipe._strip_group(Hs, Ws, chunk, n_units)
        colour = torch.rand(group * chunk, 3, device=dev) * 2 - 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.vae.encode_constant(colour, Hs * s, Ws * s)
        torch.cuda.synchronize()
        first = 1e3 * (time.perf_counter() - t0)
        _, ev = timed(lambda: pipe.vae.encode_constant(colour, Hs * s, Ws * s))
        torch.cuda.synchronize()
        shapes[str(ranks)] = {"units_per_call": group, "batch": group * chunk, "calls_on_busiest_rank": -(-(-(-n_units // ranks)) // group),
                              "first_ms_wall": round(first, 1), "ms": round(ev[0].elapsed_time(ev[1]), 3)}
    pipe.sharder = real
    rep["call_shapes_by_ranks"] = shapes
    print(name, json.dumps(rep), flush=True)
    return rep


def result_line(path):
    """the JSON result line of a bench.py output (or a file that holds only that object)"""
    text = open(path).read()
    lines = [ln for ln in text.splitlines() if ln.startswith("{") and '"value"' in ln]
    return json.loads(lines[-1] if lines else text)


def fp32_leg(path):
    r = result_line(path)
    leg = r["tolerance"]["fp32_unet_same_workload"]
    return {"source": os.path.basename(path), "steps": r.get("steps"), "warmup": r.get("warmup"), "value": r["value"], "seed": leg.get("seed"),
            "meets_1e-3": leg["meets_1e-3"], "worst_rel_l2": leg["worst_rel_l2"], "bar": leg["bar"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_encode_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--bench-json", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--add-full-run", metavar="FILE", help="bench.py --gpus 1 --full output of this tree: add its fp32 leg to --out and stop")
    ap.add_argument("--parent-full-run", default=os.path.join(ROOT, "profiles", "bench_r6_final2_1gpu.json"))
    args = ap.parse_args()
    if args.add_full_run:
        doc = json.load(open(args.out))
        doc["bench_1gpu_full_fp32_leg"] = {"tree": fp32_leg(args.add_full_run), "parent": fp32_leg(args.parent_full_run)}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
        return
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda", 0)
    find = os.environ.get("ED_MIOPEN_FIND") == "1"
    if find:   # cache-population mode, as in bench.py: MIOpen benchmarks the solvers once and records the winners in miopen_cache/
        torch.backends.cudnn.benchmark = True
    doc = {"what": "pad-strip VAE encodes, models.VAE_NARROW_CONSTANT off (full) and on (narrowed); full-width fp32 VAE, seeded weights",
           "device": torch.cuda.get_device_name(0), "miopen_find_run": find, "geometries": {}}
    saved = models.VAE_NARROW_CONSTANT
    try:
        for name, (sd, H, W) in GEOMETRIES.items():
            doc["geometries"][name] = measure(name, sd, H, W, args.timesteps, args.reps, dev)
    finally:
        models.VAE_NARROW_CONSTANT = saved
    if args.bench_json:
        runs = []
        for item in args.bench_json:
            label, path = item.split("=", 1)
            r = result_line(path)
            runs.append({"run": label, "value": r["value"], "setup_done_ms": (r.get("phase_ms_last_image") or {}).get("setup_done"),
                         "steps": r.get("steps"), "warmup": r.get("warmup")})
        doc["bench_1gpu_alternated"] = runs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
