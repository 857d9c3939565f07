"""IP-Adapter decoupled cross attention on the MI355X: what the one-launch kernel costs over the text-only
launch, what it saves over two launches plus an axpy, and what an adapter costs one full-width SDXL forward.

    python tools/ip_adapter_timing.py [--out profiles/ip_adapter_timing.json] [--rounds 5] [--repeats 5] [--inner 20] [--no-forward]

Kernel arms, alternated within every round, fp16, head dim 64, k / v the two column halves of one [B, Nt + Ni, 2 inner] tensor as
the model passes them; the shapes are the SDXL forward's cross attentions at 12 and 40 rows, (B, H, Nq) = (12, 10, 4096),
(12, 20, 1024), (40, 10, 4096), (40, 20, 1024), against Nt = 77 / 154 text keys and Ni = 4 / 16 image keys:

    fused      ops.flash_attention_ip                                            one launch
    text       ops.flash_attention(text rows, v_path=8)                          the launch without an adapter: fused - text = the price
    two        ops.flash_attention(text rows) + ops.flash_attention(image rows), then out.add_(image, alpha=scale): the default
               dispatch of each (at Nt = 154, Nq = 1024 the text pass is the pipelined kernel), what the unfused path runs
    two_small  the same with v_path=8 forced for the text pass (differs from ``two`` only where the dispatch picks the pipelined kernel)

One run = HIP events around ``--inner`` back-to-back calls on the current stream, divided by ``--inner``; per round and arm the
median of ``--repeats`` runs after ``--warmup`` untimed calls per arm; the figure is the median of the round medians, the spread
max - min of them.  ``fused`` and ``two`` are compared on the timed inputs (max |difference|).

Forward: ``ElasticDiffusion("XL1.0")`` (random weights, fp16), one 40-row forward replayed as a hipGraph on 77 text tokens without
an adapter, then with a random 4-token adapter installed on 77 + 4 tokens (the k|v hoisted as in the loop); milliseconds per
replay, same round / spread scheme.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elasticdiffusion_official_amd import ops  # noqa: E402

SHAPES = [(12, 10, 4096), (12, 20, 1024), (40, 10, 4096), (40, 20, 1024)]   # (B, H, Nq)
TEXT_KEYS, IMAGE_KEYS, SCALE = (77, 154), (4, 16), 0.6


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


def make_inputs(B, H, Nq, N, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, device="cuda", generator=g).half()
    kv = torch.randn(B, N, 2 * H * 64, device="cuda", generator=g).half()
    return q, kv[..., :H * 64], kv[..., H * 64:]


def arms_of(q, k, v, H, nt):
    kt, vt, ki, vi = k[:, :nt], v[:, :nt], k[:, nt:], v[:, nt:]

    def two(v_path=None):
        return ops.flash_attention(q, kt, vt, H, v_path=v_path).add_(ops.flash_attention(q, ki, vi, H), alpha=SCALE)
    return {"fused": lambda: ops.flash_attention_ip(q, k, v, H, nt, SCALE),
            "text": lambda: ops.flash_attention(q, kt, vt, H, v_path=8),
            "two": two, "two_small": lambda: two(8)}


def kernel_rows(opt):
    rows = []
    for B, H, Nq in SHAPES:
        for nt in TEXT_KEYS:
            for ni in IMAGE_KEYS:
                q, k, v = make_inputs(B, H, Nq, nt + ni)
                arms = arms_of(q, k, v, H, nt)
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
                row = {"B": B, "H": H, "Nq": Nq, "Nt": nt, "Ni": ni, "us": us, "spread_us": spread, "us_round_medians": med,
                       "text_variant_of_two": ops._flash_variant(B, H, Nq, nt),
                       "max_abs_diff_fused_vs_two": float((outs["fused"].float() - outs["two"].float()).abs().max()),
                       "fused_over_text": us["fused"] / us["text"], "fused_over_two": us["fused"] / us["two"],
                       "fused_beats_two_by_more_than_the_spread": bool(us["two"] - us["fused"] > spread["two"] + spread["fused"]),
                       "algorithmic_bytes": 2.0 * 2 * H * 64 * B * (Nq + nt + ni)}
                row["fused_tb_per_s"] = row["algorithmic_bytes"] / us["fused"] * 1e-6
                rows.append(row)
                print(json.dumps({a: b for a, b in row.items() if a != "us_round_medians"}), flush=True)
    return rows


def random_adapter(unet, ni, clip_dim, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cross = unet.config.cross_attention_dim

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)
    state = {"image_proj.proj.weight": rn(ni * cross, clip_dim) / clip_dim ** 0.5, "image_proj.proj.bias": 0.2 * rn(ni * cross),
             "image_proj.norm.weight": 1.0 + 0.2 * rn(cross), "image_proj.norm.bias": 0.1 * rn(cross)}
    for n, a in enumerate(unet.ip_attentions()):
        for name in ("to_k_ip", "to_v_ip"):
            state[f"ip_adapter.{2 * n + 1}.{name}.weight"] = (rn(a.to_k.out_features, cross) / cross ** 0.5).half()
    return state


def forward_rows(opt, rows=40, ni=4):
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
    cfg = pipe.unet.config
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, 4, 128, 128, generator=g).to("cuda", torch.float16)
    pooled = torch.randn(rows, cfg.pooled_projection_dim, generator=g).to("cuda", torch.float16)
    t = torch.tensor(500, device="cuda")
    text = torch.randn(rows, 77, cfg.cross_attention_dim, generator=g).to("cuda", torch.float16)
    image = torch.randn(rows, ni, cfg.cross_attention_dim, generator=g).to("cuda", torch.float16)
    med = {}

    def measure(name, txt):
        with torch.no_grad():
            for _ in range(3):      # capture + warm
                pipe._runner(x, t, txt, pooled)
            torch.cuda.synchronize()
            med[name] = [1e-3 * timed_us(lambda: pipe._runner(x, t, txt, pooled), opt.repeats, 4) for _ in range(opt.rounds)]
    measure("text_only", text)
    pipe.load_ip_adapter(random_adapter(pipe.unet, ni, 1280), scale=SCALE)
    measure("with_adapter", torch.cat([text, image], dim=1).contiguous())
    pipe.unload_ip_adapter()
    measure("text_only_again", text)
    row = {"rows": rows, "dtype": "float16", "Nt": 77, "Ni": ni, "graphs": pipe._runner.stats(),
           "ms": {n: statistics.median(v) for n, v in med.items()}, "spread_ms": {n: max(v) - min(v) for n, v in med.items()},
           "ms_round_medians": med}
    row["with_adapter_over_text_only"] = row["ms"]["with_adapter"] / row["ms"]["text_only"]
    print(json.dumps({a: b for a, b in row.items() if a != "ms_round_medians"}), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=100, help="untimed calls per arm and shape before the first round")
    ap.add_argument("--no-forward", action="store_true")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    result = {"device": torch.cuda.get_device_name(0), "rounds": opt.rounds, "repeats": opt.repeats, "inner": opt.inner, "warmup": opt.warmup,
              "method": "HIP events around `inner` back-to-back calls on the current stream / inner; per round the median of "
                        "`repeats` such runs after `warmup` untimed calls per arm; arms alternated within each round; us = median of the "
                        "round medians, spread = max - min of them; one process, one run",
              "kernel": kernel_rows(opt)}
    if not opt.no_forward:
        result["forward"] = forward_rows(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
