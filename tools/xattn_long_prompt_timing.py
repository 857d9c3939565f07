"""Cross attention on long prompts on the MI355X: the streaming kernel (``v_path`` 8, K / V staged once per workgroup, up to
160 keys) against the pipelined self-attention kernel the dispatch used for more than 96 keys, and what a longer prompt
costs one SDXL forward.

    python tools/xattn_long_prompt_timing.py [--out profiles/xattn_long_prompt_timing.json] [--rounds 5] [--repeats 5]
                                             [--inner 20] [--no-forward]
    python tools/xattn_long_prompt_timing.py --trace        # a few calls per arm and shape, to run under a kernel trace
    [ED_TREE=DIR] python tools/xattn_long_prompt_timing.py --counts   # launches of a default 77-token image, per entry point

Kernel arms, alternated within every round, fp16, head dim 64, k / v the two column halves of one [B, Nk, 2 inner] tensor
as the model passes them; the shapes are the SDXL forward's cross attentions at 20 and 40 rows, (B H, Nq) = (20 x 10, 4096),
(20 x 20, 1024), (40 x 10, 4096), (40 x 20, 1024), against Nk = 154 (two 77-token chunks):

    pipe     ops.flash_attention(v_path=ops.FLASH_DEFAULT_PIPE)    k_flash_attn_pipe: K / V re-staged per 128 query rows
    stream   ops.flash_attention(v_path=8)                         k_flash_attn_smallkv<., 5>

One run = HIP events around ``--inner`` back-to-back calls on the current stream, divided by ``--inner``; per round and arm
the median of ``--repeats`` runs after ``--warmup`` untimed calls per arm; the figure is the median of the round medians, the spread max - min of
them.  The outputs of the two arms are compared on the timed inputs (max |difference|).

Forward: ``ElasticDiffusion("XL1.0")`` (random weights, fp16), one 20-row forward replayed as a hipGraph with text rows of 1, 2
and 3 chunks (77 / 154 / 231 tokens), the cross-attention k|v hoisted as in the loop; milliseconds per replay, same
round / spread scheme.

``--counts``: one default (77-token) SD 2.1 (head dim 64) 512 x 1024 image with the hipGraph runner off, so that every launch goes through
``ops._call``: launches per entry point and, for ``ed_flash_attention``, per (Nk, variant).  ``ED_TREE=DIR`` runs any of this against
another checkout of the package (the parent commit), to compare the two lists.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(os.environ.get("ED_TREE", ROOT)))

from elasticdiffusion_official_amd import ops  # noqa: E402

SHAPES = [(20, 10, 4096), (20, 20, 1024), (40, 10, 4096), (40, 20, 1024)]   # (B, H, Nq)
KEYS = [154]


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


def make_inputs(B, H, Nq, Nk, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, device="cuda", generator=g).half()
    kv = torch.randn(B, Nk, 2 * H * 64, device="cuda", generator=g).half()
    return q, kv[..., :H * 64], kv[..., H * 64:]


def arms_of(q, k, v, H):
    return {"pipe": lambda: ops.flash_attention(q, k, v, H, v_path=ops.FLASH_DEFAULT_PIPE),
            "stream": lambda: ops.flash_attention(q, k, v, H, v_path=8)}


def kernel_rows(opt):
    rows = []
    for B, H, Nq in SHAPES:
        for Nk in KEYS:
            q, k, v = make_inputs(B, H, Nq, Nk)
            arms = arms_of(q, k, v, H)
            outs = {}
            for _ in range(opt.warmup):     # alternated, long enough for the clocks to settle before the first round
                for n, run in arms.items():
                    outs[n] = run()
            torch.cuda.synchronize()
            med = {n: [] for n in arms}
            for _ in range(opt.rounds):
                for n, run in arms.items():
                    med[n].append(timed_us(run, opt.repeats, opt.inner))
            flop = 4.0 * B * H * Nq * Nk * 64
            nbytes = 2.0 * 2 * H * 64 * B * (Nq + Nk)
            row = {"B": B, "H": H, "Nq": Nq, "Nk": Nk, "us": {n: statistics.median(x) for n, x in med.items()},
                   "spread_us": {n: max(x) - min(x) for n, x in med.items()}, "us_round_medians": med,
                   "max_abs_diff": float((outs["pipe"].float() - outs["stream"].float()).abs().max()),
                   "algorithmic_flop": flop, "algorithmic_bytes": nbytes}
            row["stream_over_pipe"] = row["us"]["stream"] / row["us"]["pipe"]
            row["stream_tb_per_s"] = nbytes / row["us"]["stream"] * 1e-6
            row["rounds_stream_faster"] = sum(s_ < p_ for p_, s_ in zip(med["pipe"], med["stream"]))
            row["stream_wins_by_more_than_the_spread"] = bool(
                row["us"]["pipe"] - row["us"]["stream"] > row["spread_us"]["pipe"] + row["spread_us"]["stream"])
            rows.append(row)
            print(json.dumps({a: b for a, b in row.items() if a != "us_round_medians"}), flush=True)
    return rows


def forward_rows(opt):
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
    cfg = pipe.unet.config
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20, 4, 128, 128, generator=g).to("cuda", torch.float16)
    pooled = torch.randn(20, cfg.pooled_projection_dim, generator=g).to("cuda", torch.float16)
    t = torch.tensor(500, device="cuda")
    texts = {n: torch.randn(20, 77 * n, cfg.cross_attention_dim, generator=g).to("cuda", torch.float16) for n in (1, 2, 3)}
    with torch.no_grad():
        for txt in texts.values():     # capture + warm every graph
            for _ in range(3):
                pipe._runner(x, t, txt, pooled)
        torch.cuda.synchronize()
        med = {n: [] for n in texts}
        for _ in range(opt.rounds):
            for n, txt in texts.items():
                med[n].append(1e-3 * timed_us(lambda: pipe._runner(x, t, txt, pooled), opt.repeats, 4))   # noqa: B023
    row = {"rows": 20, "dtype": "float16", "graphs": pipe._runner.stats(),
           "flash_variant": {str(n): {f"Nq{nq}": ops._flash_variant(20, h, nq, 77 * n) for h, nq in ((10, 4096), (20, 1024))} for n in texts},
           "ms": {str(n): statistics.median(v) for n, v in med.items()}, "spread_ms": {str(n): max(v) - min(v) for n, v in med.items()},
           "ms_round_medians": {str(n): v for n, v in med.items()}}
    row["over_one_chunk"] = {n: row["ms"][n] / row["ms"]["1"] for n in row["ms"]}
    print(json.dumps({a: b for a, b in row.items() if a != "ms_round_medians"}), flush=True)
    return row


def trace_calls():
    """Three calls per arm and shape after two warm-ups: what a kernel trace of its own reads the device-side times from."""
    for B, H, Nq in SHAPES:
        for Nk in KEYS:
            q, k, v = make_inputs(B, H, Nq, Nk)
            for run in arms_of(q, k, v, H).values():
                for _ in range(5):
                    run()
            torch.cuda.synchronize()
    print("trace calls done")


def launch_counts():
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    counts, flash, orig = {}, {}, ops._call

    def spy(name, *a):
        counts[name] = counts.get(name, 0) + 1
        if name == "ed_flash_attention":
            key = f"Nk{a[8]}_hd{a[9]}_variant{a[-2]}"
            flash[key] = flash.get(key, 0) + 1
        return orig(name, *a)
    ops._call = spy
    try:
        pipe = ElasticDiffusion("cuda:0", "2.1", view_batch_size=4, model_dtype=torch.float16, use_graphs=False)
        pipe.seed_everything(0)
        z = pipe.generate_latents("a photo", "", height=512, width=1024, num_inference_steps=2, resampling_steps=2)
    finally:
        ops._call = orig
    row = {"tree": os.path.abspath(os.environ.get("ED_TREE", ROOT)), "launches": dict(sorted(counts.items())),
           "flash_attention": dict(sorted(flash.items())), "finite": bool(torch.isfinite(z).all())}
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xattn_long_prompt_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=300, help="untimed calls per arm and shape before the first round")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--counts", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    if opt.trace:
        return trace_calls()
    if opt.counts:
        return launch_counts()
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner, "warmup": opt.warmup,
              "method": "HIP events around `inner` back-to-back calls on the current stream / inner; per round the median of "
                        "`repeats` such runs after `warmup` untimed calls per arm; arms alternated within each round; us = median of the round "
                        "medians, spread = max - min of them",
              "kernel": kernel_rows(opt)}
    if not opt.no_forward:
        result["forward"] = forward_rows(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
