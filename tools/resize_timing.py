"""Per-kernel time of the Pillow-exact resize (csrc/resize_kernels.hip) on the MI355X, and ``prepare_condition_image`` end to
end against the host path it replaces.

    python tools/resize_timing.py [--out profiles/resize_timing.json] [--repeats 20]

Kernels: the sample photo (1000 x 1000 RGB) to 512 x 512, 512 x 1024 (H x W) and 2048 x 2048, both filters; HIP events around
each entry point through ``ops.TIMER`` (rows pass, columns pass) and around ``ops.resize_u8`` as a whole, after warm-up, median
and minimum of ``--repeats`` runs.  The result of every timed configuration is first compared with ``PIL.Image.resize``.

End to end, same process, wall clock around a synchronised call, the variants taking turns, median of ``--repeats``: ``prepare_condition_image(photo, H, W,
output_type="pt")`` as it is now (upload the source bytes, resize + Canny on the device) against the parent's host path
re-stated here (``PIL.Image.resize`` + RGB on the host, upload of the resized bytes, the same device Canny), and the resize
step of each alone (PIL on the host + upload of the result; upload of the source + device resize).  Needs the GPU."""
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

from elasticdiffusion_official_amd import ElasticDiffusionControlNet, ops  # noqa: E402
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE  # noqa: E402
from tests.test_hip_parity import _embed_fn  # noqa: E402

SIZES = [(512, 512), (512, 1024), (2048, 2048)]          # (H, W)


def _events(fn, repeats, warmup=3):
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
    return {"median": statistics.median(us), "min": min(us)}


def _wall(fns, repeats, warmup=3):
    """{name: fn} -> {name: {median, min}} of the wall time (us) of a synchronised call; the functions take turns inside every
    repeat, so that whatever else the host is doing falls on all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us[name].append(1e6 * (time.perf_counter() - t0))
    return {name: {"median": statistics.median(v), "min": min(v)} for name, v in us.items()}


def kernels(photo, repeats):
    from PIL import Image
    arr = np.asarray(photo)
    dev = torch.from_numpy(arr.copy()).cuda()
    rows = []
    for H, W in SIZES:
        for name, f in (("bicubic", Image.BICUBIC), ("lanczos", Image.LANCZOS)):
            want = np.asarray(photo.resize((W, H), f))
            assert np.array_equal(ops.resize_u8(dev, (H, W), name).cpu().numpy(), want), "differs from Pillow"
            whole = _events(lambda: ops.resize_u8(dev, (H, W), name, out="cond"), repeats)
            ops.TIMER.start()
            for _ in range(repeats):
                ops.resize_u8(dev, (H, W), name, out="cond")
            per = {k: {"launches": v[0], "mean": v[1]} for k, v in ops.TIMER.stop().items()}
            t0 = time.perf_counter()
            for _ in range(5):
                photo.resize((W, H), f)
            rows.append({"H_out": H, "W_out": W, "filter": name, "us_resize_u8_cond": whole, "us_per_entry_point": per,
                         "us_pil_resize_host": 1e6 * (time.perf_counter() - t0) / 5})
            print(json.dumps(rows[-1]))
    return rows


def end_to_end(photo, repeats):
    pipe = ElasticDiffusionControlNet("cuda:0", "1.5", "canny", view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(),
                                      text_encoder=_embed_fn(False), controlnet=FakeControlNet())
    arr = np.array(photo)
    rows = []
    for H, W in SIZES:
        ds = pipe.get_downsample_size(H, W)
        h_px, w_px = ds[0] * pipe.vae_scale_factor, ds[1] * pipe.vae_scale_factor

        def parent():           # the parent commit's prepare_condition_image with output_type="pt" added: host resize, upload, device Canny
            img = photo.resize((w_px, h_px)).convert("RGB")
            return ops.canny(torch.from_numpy(np.ascontiguousarray(np.array(img))).to(pipe.device), 100, 200, out="cond")

        def host_resize_upload():
            return torch.from_numpy(np.ascontiguousarray(np.array(photo.resize((w_px, h_px)).convert("RGB")))).to(pipe.device)

        def device_resize_upload():
            return ops.resize_u8(torch.from_numpy(np.ascontiguousarray(arr)).to(pipe.device), (h_px, w_px), "bicubic")

        now = lambda: pipe.prepare_condition_image(photo, H, W, output_type="pt")  # noqa: E731
        assert torch.equal(now(), parent()), "the device path and the host path disagree"
        rows.append({"H": H, "W": W, "condition_H": h_px, "condition_W": w_px,
                     **_wall({"us_prepare_condition_image_pt": now, "us_parent_host_path": parent,
                              "us_resize_step_device_incl_upload_of_source": device_resize_upload,
                              "us_resize_step_host_incl_upload_of_result": host_resize_upload}, repeats)})
        print(json.dumps(rows[-1]))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_timing.json"))
    ap.add_argument("--repeats", type=int, default=20)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: timings are taken on the MI355X only")
    import PIL
    from PIL import Image
    photo = Image.open(os.path.join(ROOT, "tests", "golden", "canny_input_yoga.jpeg")).convert("RGB")
    photo.load()
    result = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats, "pillow": PIL.__version__,
              "host_threads": torch.get_num_threads(),
              "method": "kernels: HIP events on the current stream, warm-up 3, median and minimum of the repeats (per entry point: mean "
                        "of ops.TIMER's events); end to end: wall clock around a synchronised call, the variants alternating, warm-up 3, median and minimum; one "
                        "run on one box; the host figures are this box's CPU and Pillow build",
              "kernels": kernels(photo, opt.repeats), "end_to_end": end_to_end(photo, opt.repeats)}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"wrote {opt.out}")


if __name__ == "__main__":
    main()
