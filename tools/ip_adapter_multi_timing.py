"""Several IP-Adapters at once on the MI355X: the one-launch kernel against the fallback it replaces, what 0 /
1 / 2 adapters cost a 10-step SDXL 1024 x 2048 image, and what a change of scales costs with device weights (a replay) against the
single-adapter path's by-value scale (a re-capture).

    python tools/ip_adapter_multi_timing.py [--out profiles/ip_adapter_multi_timing.json] [--rounds 5] [--repeats 5] [--inner 20]
                                            [--no-images]

Kernel arms, alternated within every round, fp16, head dim 64, 40 rows, k / v the two column halves of one [B, Nt + sum Ni, 2 inner]
tensor as the model passes them; (H, Nq) = (10, 4096), (20, 1024), (10, 1024), (20, 4096) against Nt = 77 / 154 and the
segmentations (4, 4), (16, 16), (4, 16):

    fused     ops.flash_attention_ipn                                                   one launch
    fallback  ops.flash_attention(text rows) + per adapter ops.flash_attention(its rows) and out.addcmul_(o_a, w[a]): what
              models.Attention runs where the kernel does not take the shape (A + 1 attentions, A weighted adds, the weights on the device)
    text      ops.flash_attention(text rows, v_path=8): the launch without adapters

The method is tools/ip_adapter_timing.py's: HIP events around ``--inner`` back-to-back calls, per round and arm the median of
``--repeats`` runs after ``--warmup`` untimed calls, the figure the median of the round medians, the spread max - min of them.
``fused_not_slower`` is what ops.flash_attention_ipn_ok is held to: where it is false for a shape, that shape belongs to the fallback.

Images: ``ElasticDiffusion("XL1.0")`` (random weights, fp16), 10 steps at 1024 x 2048 through the graphs, the second image of each
configuration timed (the first captures).  Scale change: seconds from ``set_ip_adapter_scale`` to the end of the next image, minus
an unchanged image, with one adapter (graphs dropped and captured again) and with two (replayed).  Needs the GPU: no fallback.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from elasticdiffusion_official_amd import ops  # noqa: E402
from ip_adapter_timing import make_inputs, random_adapter, timed_us  # noqa: E402

ROWS = 40
SHAPES = [(10, 4096), (20, 1024), (10, 1024), (20, 4096)]   # (H, Nq)
TEXT_KEYS, SEGMENTATIONS, WEIGHTS = (77, 154), ((4, 4), (16, 16), (4, 16)), (0.6, 0.8)


def arms_of(q, k, v, H, nt, segs, w):
    rows, off = [], nt
    for n in segs:
        rows.append((off, off + n))
        off += n

    def fallback():
        o = ops.flash_attention(q, k[:, :nt], v[:, :nt], H)
        wd = w.to(o.dtype)
        for a, (lo, hi) in enumerate(rows):
            o = o.addcmul_(ops.flash_attention(q, k[:, lo:hi], v[:, lo:hi], H), wd[a])
        return o
    return {"fused": lambda: ops.flash_attention_ipn(q, k, v, H, nt, segs, w), "fallback": fallback,
            "text": lambda: ops.flash_attention(q, k[:, :nt], v[:, :nt], H, v_path=8)}


def kernel_rows(opt):
    out = []
    w = torch.tensor(WEIGHTS, dtype=torch.float32, device="cuda")
    for H, Nq in SHAPES:
        for nt in TEXT_KEYS:
            for segs in SEGMENTATIONS:
                q, k, v = make_inputs(ROWS, H, Nq, nt + sum(segs))
                arms = arms_of(q, k, v, H, nt, segs, w)
                outs = {}
                for _ in range(opt.warmup):
                    for n, run in arms.items():
                        outs[n] = run()
                torch.cuda.synchronize()
                med = {n: [] for n in arms}
                for _ in range(opt.rounds):
                    for n, run in arms.items():
                        med[n].append(timed_us(run, opt.repeats, opt.inner))
                us = {n: statistics.median(x) for n, x in med.items()}
                spread = {n: max(x) - min(x) for n, x in med.items()}
                row = {"B": ROWS, "H": H, "Nq": Nq, "Nt": nt, "Ni": list(segs), "us": us, "spread_us": spread, "us_round_medians": med,
                       "max_abs_diff_fused_vs_fallback": float((outs["fused"].float() - outs["fallback"].float()).abs().max()),
                       "fused_over_fallback": us["fused"] / us["fallback"], "fused_over_text": us["fused"] / us["text"],
                       "fused_not_slower": bool(us["fused"] <= us["fallback"]),
                       "fused_faster_by_more_than_the_spread": bool(us["fallback"] - us["fused"] > spread["fallback"] + spread["fused"]),
                       "dispatch_takes_fused": bool(ops.flash_attention_ipn_ok(64, nt, segs))}
                out.append(row)
                print(json.dumps({a: b for a, b in row.items() if a != "us_round_medians"}), flush=True)
    return out


def image_rows(opt):
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
    run = dict(height=1024, width=2048, num_inference_steps=10)
    g = torch.Generator().manual_seed(0)
    e = [torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g)]

    def image(**kw):
        pipe.seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.generate_latents("a photo", "", **run, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def steady(**kw):
        image(**kw)                                          # captures
        return statistics.median(image(**kw) for _ in range(opt.images))
    res = {"steps": 10, "size": [1024, 2048], "dtype": "float16", "seconds_per_image": {}, "scale_change_seconds": {}}
    res["seconds_per_image"]["0_adapters"] = steady()
    pipe.load_ip_adapter(random_adapter(pipe.unet, 4, 1280, seed=1), scale=0.6)
    one = dict(ip_adapter_image_embeds=e[0])
    res["seconds_per_image"]["1_adapter"] = steady(**one)
    pipe.set_ip_adapter_scale(0.5)
    res["scale_change_seconds"]["1_adapter_recapture"] = image(**one) - res["seconds_per_image"]["1_adapter"]
    pipe.load_ip_adapter(random_adapter(pipe.unet, 16, 1280, seed=2), scale=0.8, add=True)
    two = dict(ip_adapter_image_embeds=e)
    res["seconds_per_image"]["2_adapters"] = steady(**two)
    entries = len(pipe._runner.entries)
    pipe.set_ip_adapter_scale([0.5, 0.7])
    res["scale_change_seconds"]["2_adapters_replay"] = image(**two) - res["seconds_per_image"]["2_adapters"]
    res["graph_entries_unchanged_by_the_scale_change"] = len(pipe._runner.entries) == entries
    res["graphs"] = pipe._runner.stats()
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter_multi_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=100, help="untimed calls per arm and shape before the first round")
    ap.add_argument("--images", type=int, default=2, help="timed images per configuration")
    ap.add_argument("--no-images", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner, "warmup": opt.warmup,
              "method": "HIP events around `inner` back-to-back calls on the current stream / inner; per round the median of "
                        "`repeats` such runs after `warmup` untimed calls per arm; arms alternated within each round; us = median of the "
                        "round medians, spread = max - min of them; one process, one run",
              "kernel": kernel_rows(opt)}
    result["shapes_where_fused_is_slower"] = [[r["H"], r["Nq"], r["Nt"], r["Ni"]] for r in result["kernel"] if not r["fused_not_slower"]]
    if not opt.no_images:
        result["images"] = image_rows(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
