"""IP-Adapter attention masks on the MI355X: what the mask costs the one-launch kernel, the masked kernel
against the masked fallback, the mask-rows launch against the torch ops that restate it, and what masks -- and a change of masks --
cost a 10-step SDXL 1024 x 2048 image with two adapters.

    python tools/ip_adapter_mask_timing.py [--out profiles/ip_adapter_mask_timing.json] [--rounds 5] [--repeats 5] [--inner 20]
                                           [--no-images]

Kernel arms, alternated within every round, the method and shapes of tools/ip_adapter_multi_timing.py (fp16, head dim 64, 40 rows;
(H, Nq) = (10, 4096), (20, 1024), (10, 1024), (20, 4096) against Nt = 77 / 154 and the segmentations (4, 4), (16, 16), (4, 16)):

    ipm       ops.flash_attention_ipm, m a level view [40, A, Nq] of a [40, A, S] buffer as the model passes it
    ipn       ops.flash_attention_ipn: the launch without masks -- ipm / ipn is the price of the mask
    fallback  ops.flash_attention(text rows) + per adapter ops.flash_attention(its rows) and out.addcmul_(o_a, (w[a] m_a)[..., None]):
              what models.Attention runs with masks where the kernel does not take the shape

``ipm_not_slower`` is what ops.flash_attention_ipm_ok is held to: where it is false for a shape, that shape belongs to the fallback.

Mask rows: ops.ip_mask_rows for the SDXL 1024 x 2048 batch (128 x 128 rows, 8 steps x 2 copies + 4 views, 2 adapters) against the
torch op sequence that restates it (index gathers into a zero frame, three strided 2 x 2 means, one cat).

Images: ``ElasticDiffusion("XL1.0")`` (random weights, fp16), 10 steps at 1024 x 2048 through the graphs with two adapters, the
median of ``--images`` images after the capturing one, without and with masks; then new masks: seconds of the next image minus an
unchanged image, and the captured-graph count before and after.  Needs the GPU: no fallback.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from elasticdiffusion_official_amd import ops  # noqa: E402
from ip_adapter_timing import make_inputs, random_adapter, timed_us  # noqa: E402

ROWS = 40
SHAPES = [(10, 4096), (20, 1024), (10, 1024), (20, 4096)]   # (H, Nq)
TEXT_KEYS, SEGMENTATIONS, WEIGHTS = (77, 154), ((4, 4), (16, 16), (4, 16)), (0.6, 0.8)


def arms_of(q, k, v, H, nt, segs, w, m):
    rows, off = [], nt
    for n in segs:
        rows.append((off, off + n))
        off += n

    def fallback():
        o = ops.flash_attention(q, k[:, :nt], v[:, :nt], H)
        wd = w.to(o.dtype)
        for a, (lo, hi) in enumerate(rows):
            o = o.addcmul_(ops.flash_attention(q, k[:, lo:hi], v[:, lo:hi], H), (wd[a] * m[:, a].to(o.dtype))[..., None])
        return o
    return {"ipm": lambda: ops.flash_attention_ipm(q, k, v, H, nt, segs, w, m), "ipn": lambda: ops.flash_attention_ipn(q, k, v, H, nt, segs, w),
            "fallback": fallback}


def measure(arms, opt):
    outs = {}
    for _ in range(opt.warmup):
        for n, run in arms.items():
            outs[n] = run()
    torch.cuda.synchronize()
    med = {n: [] for n in arms}
    for _ in range(opt.rounds):
        for n, run in arms.items():
            med[n].append(timed_us(run, opt.repeats, opt.inner))
    return ({n: statistics.median(x) for n, x in med.items()}, {n: max(x) - min(x) for n, x in med.items()}, med, outs)


def kernel_rows(opt):
    out = []
    w = torch.tensor(WEIGHTS, dtype=torch.float32, device="cuda")
    for H, Nq in SHAPES:
        side = int(Nq ** 0.5)
        lay, S_ = ops.ip_mask_layout(2 * side, 2 * side)            # the layer reads level 1 of rows twice its side
        buf = torch.rand(ROWS, 2, S_, device="cuda")
        m = buf[:, :, lay[1][0]:lay[1][0] + Nq]
        for nt in TEXT_KEYS:
            for segs in SEGMENTATIONS:
                q, k, v = make_inputs(ROWS, H, Nq, nt + sum(segs))
                us, spread, med, outs = measure(arms_of(q, k, v, H, nt, segs, w, m), opt)
                row = {"B": ROWS, "H": H, "Nq": Nq, "Nt": nt, "Ni": list(segs), "us": us, "spread_us": spread, "us_round_medians": med,
                       "max_abs_diff_ipm_vs_fallback": float((outs["ipm"].float() - outs["fallback"].float()).abs().max()),
                       "ipm_over_ipn": us["ipm"] / us["ipn"], "ipm_over_fallback": us["ipm"] / us["fallback"],
                       "ipm_not_slower": bool(us["ipm"] <= us["fallback"]),
                       "ipm_slower_by_more_than_the_spread": bool(us["ipm"] - us["fallback"] > spread["fallback"] + spread["ipm"]),
                       "dispatch_takes_ipm": bool(ops.flash_attention_ipm_ok(64, nt, segs))}
                out.append(row)
                print(json.dumps({a: b for a, b in row.items() if a != "us_round_medians"}), flush=True)
    return out


def mask_rows_row(opt):
    """the SDXL 1024 x 2048 batch: 128 x 256 latent, reduced 64 x 128 in 128 x 128 rows, K = 8 steps, 4 views, 2 adapters"""
    from elasticdiffusion_official_amd import geometry
    Hl, Wl, d, K, A_ = 128, 256, 128, 8, 2
    h, w = 64, 128
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, d // 2, d // 2, d - d // 2)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32, device="cuda")   # noqa: E731
    idx = torch.randint(0, 4, (K, h * w), dtype=torch.uint8, device="cuda")
    masks = torch.rand(1, A_, Hl, Wl, device="cuda")
    sr, sc, wy, wx = i32(pp.src_row), i32(pp.src_col), i32(vp.win_y0), i32(vp.win_x0)
    args = (idx, sr, sc, h, w, gpad.top, gpad.left, wy, wx, vp.Sh, vp.Sw, vpad.top, vpad.left, d, d, 2)
    V = wy.numel()
    out = torch.empty((K * 2 + V), A_, ops.ip_mask_layout(d, d)[1], device="cuda")
    q = idx.view(K, h, w).long()
    ii = torch.arange(h, device="cuda").view(1, h, 1).expand(K, h, w)
    jj = torch.arange(w, device="cuda").view(1, 1, w).expand(K, h, w)
    ys, xs = torch.arange(vp.Sh, device="cuda"), torch.arange(vp.Sw, device="cuda")

    def torch_ops():
        sy, sx = sr.long()[2 * ii + (q >> 1)], sc.long()[2 * jj + (q & 1)]
        g = torch.zeros(K, 1, A_, d, d, device="cuda")
        g[:, :, :, gpad.top:gpad.top + h, gpad.left:gpad.left + w] = masks[:, :, sy, sx].permute(2, 0, 1, 3, 4)
        vy, vx = wy.long().view(V, 1) + ys, wx.long().view(V, 1) + xs
        ok = ((vy >= 0) & (vy < Hl))[:, :, None] & ((vx >= 0) & (vx < Wl))[:, None, :]
        val = masks[:, :, vy.clamp(0, Hl - 1)[:, :, None], vx.clamp(0, Wl - 1)[:, None, :]]
        vv = torch.zeros(V, 1, A_, d, d, device="cuda")
        vv[:, :, :, vpad.top:vpad.top + vp.Sh, vpad.left:vpad.left + vp.Sw] = torch.where(ok, val, val.new_zeros(())).permute(2, 0, 1, 3, 4)
        l = torch.cat([g[:, None].expand(K, 2, 1, A_, d, d).reshape(2 * K, A_, d, d), vv.reshape(V, A_, d, d)])
        levels = [l]
        for _ in range(3):
            l = 0.25 * ((l[..., 0::2, 0::2] + l[..., 0::2, 1::2]) + (l[..., 1::2, 0::2] + l[..., 1::2, 1::2]))
            levels.append(l)
        return torch.cat([x.reshape(x.shape[0], A_, -1) for x in levels], dim=-1)
    arms = {"kernel": lambda: ops.ip_mask_rows(masks, *args, out=out), "torch_ops": torch_ops}
    us, spread, med, outs = measure(arms, opt)
    row = {"rows": K * 2 + V, "A": A_, "row_size": [d, d], "views": V, "us": us, "spread_us": spread, "us_round_medians": med,
           "bit_equal": bool(torch.equal(outs["kernel"], outs["torch_ops"])), "kernel_over_torch_ops": us["kernel"] / us["torch_ops"]}
    print(json.dumps({a: b for a, b in row.items() if a != "us_round_medians"}), flush=True)
    return row


def image_rows(opt):
    from elasticdiffusion_official_amd import ElasticDiffusion
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    pipe = ElasticDiffusion("cuda:0", "XL1.0", view_batch_size=16, model_dtype=torch.float16)
    run = dict(height=1024, width=2048, num_inference_steps=10)
    g = torch.Generator().manual_seed(0)
    e = [torch.randn(1, 1280, generator=g), torch.randn(1, 1280, generator=g)]
    pipe.load_ip_adapter(random_adapter(pipe.unet, 4, 1280, seed=1), scale=0.6)
    pipe.load_ip_adapter(random_adapter(pipe.unet, 16, 1280, seed=2), scale=0.8, add=True)
    two = dict(ip_adapter_image_embeds=e)

    def image(**kw):
        pipe.seed_everything(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.generate_latents("a photo", "", **run, **two, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def steady(**kw):
        image(**kw)                                          # captures
        return statistics.median(image(**kw) for _ in range(opt.images))
    left = np.zeros((1024, 2048), np.uint8)
    left[:, :1024] = 255
    masks_a = [left, (1024, 0, 2048, 1024)]
    masks_b = [(0, 0, 2048, 512), np.ascontiguousarray(255 - left)]
    res = {"steps": 10, "size": [1024, 2048], "dtype": "float16", "adapters": [4, 16], "seconds_per_image": {}}
    res["seconds_per_image"]["without_masks"] = steady()
    res["seconds_per_image"]["with_masks"] = steady(ip_adapter_masks=masks_a)
    entries, captured = len(pipe._runner.entries), pipe._runner.stats()["captured"]
    res["new_masks_seconds_over_an_unchanged_image"] = image(ip_adapter_masks=masks_b) - res["seconds_per_image"]["with_masks"]
    res["graph_entries_unchanged_by_new_masks"] = len(pipe._runner.entries) == entries
    res["captured_before_and_after_new_masks"] = [captured, pipe._runner.stats()["captured"]]
    res["graphs"] = pipe._runner.stats()
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter_mask_timing.json"))
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
              "kernel": kernel_rows(opt), "mask_rows": mask_rows_row(opt)}
    result["shapes_where_ipm_is_slower_than_the_fallback"] = [[r["H"], r["Nq"], r["Nt"], r["Ni"]] for r in result["kernel"]
                                                              if r["ipm_slower_by_more_than_the_spread"]]
    if not opt.no_images:
        result["images"] = image_rows(opt)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
