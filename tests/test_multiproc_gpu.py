"""-m gpu: the row-sharded multi-rank path end to end.  Two (three) processes share the single GPU of the test box and
talk over gloo (RCCL refuses two ranks on one device).  Every rank must end with bit-identical latents and images (the
glue is replicated and the all-gather is exact), match the unsharded run of the same pipeline to 1e-4 and the
reference's golden vector to BASELINE.json's 1e-3, and leave the host RNG in the reference's end state."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.procs import join_all

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, name, ret):
    import torch.distributed as dist
    from elasticdiffusion_official_amd import ElasticDiffusion
    from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
    from tests.golden import cases
    from tests.test_hip_parity import _embed_fn
    from oracle import elastic_oracle as eo
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = cases.E2E_CASES[name]
        xl = c["sd"].startswith("XL")
        cn = c.get("controlnet", False)
        kw = dict(cases.E2E_KW)
        kw.update(c.get("kw", {}))
        if cn:
            ds = eo.get_downsample_size(c["H"], c["W"], c["sd"])
            kw.update(condition_image=cases.synthetic_condition(ds[0] * 8, ds[1] * 8), controlnet_conditioning_scale=0.2)
        pipe = ElasticDiffusion("cuda:0", c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl),
                                vae=FakeVAE(), text_encoder=_embed_fn(xl), controlnet=FakeControlNet() if cn else None)
        assert pipe.sharder.world_size == world
        pipe.seed_everything(c["seed"])
        imgs, _ = pipe.generate_image("p", "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                                      resampling_steps=c["R"], tiled_decoder=bool(c.get("tiled")), output_type="pt", **kw)
        tail = torch.rand(4).numpy()
        z = pipe.last_latents.clone()
        same_as_unsharded = None
        if rank == 0:  # the invariant: sharding + all-gather is bit-transparent w.r.t. the same pipeline unsharded
            solo = ElasticDiffusion("cuda:0", c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"], xl=xl),
                                    vae=FakeVAE(), text_encoder=_embed_fn(xl), controlnet=FakeControlNet() if cn else None,
                                    process_group=False)
            assert solo.sharder.world_size == 1
            solo.seed_everything(c["seed"])
            imgs1, _ = solo.generate_image("p", "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                                           resampling_steps=c["R"], tiled_decoder=bool(c.get("tiled")), output_type="pt",
                                           **kw)
            same_as_unsharded = float((solo.last_latents - z).norm() / z.norm())
        ret[rank] = (z.cpu().numpy(), imgs.cpu().numpy(), tail, same_as_unsharded)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,name", [(2, "cfg2_sd_512x1024"), (3, "cfg3_xl_1024x2048"), (2, "tiled_sd_640x512"),
                                        (2, "cn_sd_512x1024"), (3, "cfg4_xl_2048x2048_tiled")])
def test_sharded_ranks_reproduce_reference_latents(golden_dir, world, name):
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, ret)) for r in range(world)]
    for p in procs:
        p.start()
    join_all(procs, 300, f"{world} ranks sharing the GPU ({name})")
    want = g[f"{name}/latent"]
    # the exchange (all-gather of model outputs) is exact; what may differ between a sharded and an unsharded run is
    # the model forward itself, because the per-rank batch shape changes the library's kernel choice (rounding order)
    assert ret[0][3] < 1e-4, f"sharded vs unsharded rel-L2 {ret[0][3]}"
    for r in range(world):
        z, img, tail, _ = ret[r]
        rel = np.linalg.norm(z - want) / np.linalg.norm(want)
        assert rel < 1e-3, (r, rel)  # BASELINE.json's bar vs the reference; the strict check is the bitwise one above
        np.testing.assert_array_equal(tail, g[f"{name}/rng_tail"])
        np.testing.assert_array_equal(z, ret[0][0])      # all ranks bit-identical
        np.testing.assert_array_equal(img, ret[0][1])


def _quiet(stderr):
    """stderr of a bench.py run without MIOpen's per-convolution workspace warnings (hundreds of lines that bury the one that matters)"""
    return "\n".join(ln for ln in stderr.splitlines() if "MIOpen(HIP): Warning" not in ln)


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--gpus", "2", "--in-flight", "1"],   # default at N = 2: two images in flight
                                   ["--gpus", "4", "--shard-group", "2", "--in-flight", "2", "--all-layouts"],
                                   ["--gpus", "8"]])   # the driver's largest layout: one 8-way shard group, 4 images in flight
def test_bench_multi_rank_rehearsal(flags):
    """bench.py's N > 1 control flow end to end (process groups, row sharding, images in flight, the alternative
    layouts measured after the timed region, max-over-ranks timing, rank 0 printing ONE JSON line) with N ranks sharing
    this box's single GPU over gloo and the reduced-width architecture.  The numbers mean nothing; the point is that
    the exact code path the driver launches on 2/4/8 GPUs (there over RCCL) runs and reports what it should."""
    import json
    import subprocess
    import sys
    n = int(flags[1])
    env = dict(os.environ, ED_DIST_BACKEND="gloo", MIOPEN_FIND_MODE="FAST", HSA_ENABLE_IPC_MODE_LEGACY="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", *flags, "--steps", "2", "--warmup", "1", "--small",
           "--workload", "sd15_512x1024", "--timesteps", "3", "--no-cpu-baseline", "--full"]
    # every rank's stdout / stderr goes to its OWN file (torchrun --redirects 3): a native abort of one rank keeps that rank's last words
    # instead of a tail of eight interleaved streams buried in MIOpen warnings (round 5 lost the cause of its one SIGABRT that way)
    import glob
    import shutil
    import tempfile
    log_dir = tempfile.mkdtemp(prefix=f"ed_rehearsal_{n}rank_")
    at = cmd.index("bench.py")
    cmd[at:at] = ["--redirects", "3", "--log-dir", log_dir]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=root, env=env, timeout=900)

    def rank_file(rank, which):
        hits = sorted(glob.glob(os.path.join(log_dir, "**", str(rank), which + ".log"), recursive=True))
        return open(hits[-1], errors="replace").read() if hits else ""

    rank_err = {r: _quiet(rank_file(r, "stderr")) for r in range(n)}
    native = out.returncode != 0 and "SIGABRT" in out.stderr and not any("Traceback (most recent call last)" in e for e in rank_err.values())
    if out.returncode != 0:
        # keep the artefacts where gpurun brings them home (no retry-to-green; the evidence travels with the report)
        keep = os.path.join(root, "gpurun_out", f"rehearsal_abort_{n}rank_{os.getpid()}")
        try:
            shutil.copytree(log_dir, keep, dirs_exist_ok=True)
            open(os.path.join(keep, "torchrun_stderr.txt"), "w").write(_quiet(out.stderr))
        except OSError:
            keep = log_dir
        tails = "\n".join(f"--- rank {r} stderr tail ---\n{e[-1500:]}" for r, e in rank_err.items() if e.strip())
        if native:
            # N + 1 processes (this pytest process holds a HIP context too) oversubscribing ONE GPU is the rehearsal's vehicle, not the
            # deployment.  Round 5 saw one SIGABRT inside the native runtime in 23 runs of the 8-rank command and RETRIED it; round 6
            # reports it instead: not green, not a stop of the whole suite for a condition that 1 GPU x 9 processes creates, and the
            # aborting rank's own stderr is attached (DESIGN.md section 7 has what the repetition loop of round 6 found).
            pytest.xfail(f"native abort (no Python exception in any rank) in the {n}-rank one-GPU rehearsal; artefacts: {keep}\n{tails}"[-6000:])
        raise AssertionError(f"bench.py failed (rc {out.returncode}); artefacts: {keep}\n{_quiet(out.stderr)[-3000:]}\n{tails}"[-9000:])
    out.stdout = rank_file(0, "stdout")
    shutil.rmtree(log_dir, ignore_errors=True)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 2 and d["scaling"] == "strong" and d["finite_output"]
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-3
    g = d["config"]["shard_group"]
    assert g == (2 if "--shard-group" in flags else n)
    comp, tot = d["rows_computed_over_rows_total_rank0"]
    assert 0 < comp <= -(-tot // g) + 2 * 50   # a rank computes ~1/g of the rows, never duplicates of others' rows
    assert d["graphs"]["eager"] == 0
    m = int(flags[flags.index("--in-flight") + 1]) if "--in-flight" in flags else max(2, g // 2)
    assert d["config"]["images_in_flight"] == m
    if not (g == n and m == 1) and (n == 2 or "--all-layouts" in flags):
        assert "view_parallel_one_image" in d["layouts"]


def _rccl_worker(port, ret):
    """One rank, backend "nccl" (= RCCL on ROCm), every forward forced through the exchange path."""
    import copy
    import torch.distributed as dist
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.sharding import RowSharder
    from tests import realarch as R
    from tests.fakes import FakeUNet, FakeVAE
    from tests.test_hip_parity import _embed_fn
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        ones = torch.ones(1, device="cuda:0")
        dist.all_reduce(ones)
        c = dict(R.REAL_CASES["cfg3_xl_1024x2048"], steps=2, R=1)
        unet, vae, _ = R.build_small(c["sd"])
        outs = {}
        # (a) deterministic fp32 parity models: the exchange must be bit-transparent; (b) the repo's real (reduced-width)
        # SDXL modules in fp16 -- the production dtype: hipBLASLt's stream-K GEMMs make two 16-bit runs differ at rounding
        # level even without any exchange, so that pair is compared to the 16-bit noise floor, not bit for bit
        for kind in ("fake_fp32", "real_fp16"):
            for forced in (True, False):
                if kind == "fake_fp32":
                    mods = dict(unet=FakeUNet(128, xl=True), vae=FakeVAE(), text_encoder=_embed_fn(True))
                else:
                    mods = dict(unet=copy.deepcopy(unet).to(torch.float16), vae=copy.deepcopy(vae), text_encoder=R.embed_fn(True))
                pipe = ElasticDiffusion("cuda:0", c["sd"], view_batch_size=c["vbs"], process_group=None if forced else False, **mods)
                if forced:
                    pipe.sharder = RowSharder(None, force_exchange=True)
                assert pipe.sharder.exchange == forced and pipe.sharder.world_size == 1
                pipe.seed_everything(c["seed"])
                imgs, _ = pipe.generate_image("p", "", height=c["H"], width=c["W"], num_inference_steps=c["steps"],
                                              resampling_steps=c["R"], output_type="pt", progress=lambda it: it, **R.LOOP_KW)
                # what the exchange count must be: one per model forward + one per pool of same-shape pad strips
                from elasticdiffusion_official_amd import geometry
                h, w = pipe.get_downsample_size(c["H"], c["W"])
                s, vc = pipe.vae_scale_factor, pipe.view_config
                vp = geometry.ViewPlan(c["H"] // s, c["W"] // s, vc["window_size"], vc["stride"], vc["context_size"])
                gpad, vpad = geometry.PadPlan(h, w, pipe.model_size), geometry.PadPlan(vp.Sh, vp.Sw, pipe.model_size)
                per_phase = 1 if (gpad.PH, gpad.PW) == (vpad.PH, vpad.PW) else 2
                phases = 2 * c["steps"] - 1 if c["R"] > 0 else c["steps"]   # RePaint phase on every step but the last
                n_pools = sum(len(pipe.strip_pools(p, c["steps"])) for p in (gpad, vpad) if p.padded)
                outs[(kind, forced)] = (pipe.last_latents.cpu().numpy(), pipe.sharder.exchanges, pipe._runner.stats(),
                                        bool(torch.isfinite(imgs).all()), phases * per_phase + n_pools)
        ret["ranks_seen"] = int(ones.item())
        ret["backend"] = dist.get_backend()
        ret["outs"] = outs
    finally:
        dist.destroy_process_group()


def test_rccl_world_size_one_exchange_path():
    """RCCL itself (backend "nccl") with ONE rank on the test GPU: process-group init, an all-reduce, the
    ``all_gather_into_tensor`` behind every model forward (RowSharder(force_exchange=True); fp32 rows with the parity
    models, fp16 rows with the real reduced-width SDXL modules), its stream ordering against the hipGraph replays that
    produce / consume the exchanged tensors, the fp32 all-gathers of the pad-strip units, and ``destroy_process_group`` all
    execute -- the multi-rank runs on this 1-GPU pool go over gloo, so this is the only place RCCL runs before the
    driver's 8-GPU box.  With deterministic models the latents are BIT-identical to the run without the exchange."""
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), ret))
    p.start()
    join_all([p], 600, "RCCL world-size-1 worker")
    assert ret["backend"] == "nccl" and ret["ranks_seen"] == 1
    outs = ret["outs"]
    for kind in ("fake_fp32", "real_fp16"):
        zf, n_exchanges, graphs, finite_f, n_expected = outs[(kind, True)]
        zp, n_plain, _, finite_p, _ = outs[(kind, False)]
        assert finite_f and finite_p
        # computed from the plans (model forwards + pad-strip pools), not a literal: here (2 steps x 2 phases - 1) + 1
        assert n_expected >= 4 and n_plain == 0 and n_exchanges == n_expected, (n_exchanges, n_expected)
        assert graphs["eager"] == 0 and graphs["captured"] >= 1
        if kind == "fake_fp32":
            np.testing.assert_array_equal(zf, zp)
        else:
            rel = float(np.linalg.norm(zf - zp) / np.linalg.norm(zp))
            assert rel < 0.03, rel   # two fp16 runs of the same loop: ~7e-3 apart (profiles/r3_precision.json "batching_fp16")
