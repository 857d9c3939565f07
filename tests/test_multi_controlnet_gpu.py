"""-m gpu: Multi-ControlNet and guidance windows through the HIP path.

Bars:
  * ``ed_control_residuals`` against the torch-CPU op sequence of tests/multi_controlnet_cpu.py: BIT-EXACT, 16-byte and scalar paths,
    every dtype pair, in place and out of place, misaligned bases, a 13-level table, closed nets holding inf / NaN;
  * on the fakes: a list of one net, two equal nets at half the scale each and all-zero scales are BIT-EQUAL to the legacy single-net
    pipeline (the products involved are exact in binary); two different nets with two windows against the unchanged oracle wrapped
    in ``MultiControlNetSpec`` at the project's end-to-end bar (rel-L2 < 1e-4, identical host RNG end state), alone and with
    ``strength``, DPM-Solver++ and two images in flight (interleaved equals alone at 1e-5);
  * the real (reduced-width) architecture against tests/sd_spec.py in fp64: twice the rel-L2 the existing single-net path has against
    the same spec with one of the nets, measured in the same test.
"""
import copy
import functools
import glob
import os

import numpy as np
import pytest
import torch

from oracle import elastic_oracle as eo
from oracle.ddim import DDIMOracle
from tests import ddim_variants as V
from tests import dpm_solver_cpu as D
from tests import img2img_cpu as I
from tests import multi_controlnet_cpu as mc
from tests import sd_spec as S
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE, synthetic_text_embeds
from tests.golden import cases
from tests.test_img2img import synthetic_image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = [(F16, F16), (BF16, BF16), (F32, F32), (F32, F16), (F32, BF16)]      # (skip / out, residuals)
NULL_SKIP = [F16, BF16, F32]                                                  # without a skip, out has the residuals' type
INVALID = 1                                                                   # hipErrorInvalidValue


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _rand(g, B, count, dtype, misaligned=False):
    """[B, count] values of ``dtype`` on the CPU and the same on the device, there optionally one element off the allocation's base"""
    x = (torch.randn(B, count, generator=g) * 2.0).to(dtype)
    if not misaligned:
        return x, x.to(DEV)
    flat = torch.empty(B * count + 1, dtype=dtype, device=DEV)
    d = flat[1:].view(B, count)
    d.copy_(x)
    assert d.data_ptr() % 16 != 0 and d.is_contiguous()
    return x, d


def _weights(g, B, N):
    return (torch.rand(B, N, generator=g) * 1.5 + 0.05) * torch.where(torch.rand(B, N, generator=g) < 0.3, -1.0, 1.0)


def _check_levels(ops, g, counts, B, N, dt, rdt, skipless, inplace, misaligned, w=None):
    w = _weights(g, B, N) if w is None else w
    skips, res, outs, want = [], [[] for _ in range(N)], [], []
    for count in counts:
        s_cpu, s_dev = (None, None) if skipless else _rand(g, B, count, dt, misaligned)
        rs = [_rand(g, B, count, rdt, misaligned) for _ in range(N)]
        want.append(mc.control_residuals_cpu(s_cpu, [r[0] for r in rs], w))
        skips.append(s_dev)
        for n in range(N):
            res[n].append(rs[n][1])
        outs.append(None if (inplace or skipless) else _rand(g, B, count, dt, misaligned)[1])
    keep = [None if s is None else s.clone() for s in skips]
    got = ops.control_residuals(None if skipless else skips, res, w.to(DEV), None if (inplace or skipless) else outs)
    for l, count in enumerate(counts):
        assert got[l].dtype == (rdt if skipless else dt) and got[l].shape == (B, count)
        if inplace and not skipless:
            assert got[l].data_ptr() == skips[l].data_ptr()
        elif not skipless:
            assert got[l].data_ptr() == outs[l].data_ptr() and torch.equal(skips[l], keep[l])      # the skip is left alone
        assert torch.equal(got[l].cpu(), want[l]), (count, B, N, dt, rdt, skipless, inplace, misaligned)
    return got, want


# ---------------------------------------------------------------------------------------------------
# ed_control_residuals
# ---------------------------------------------------------------------------------------------------
COUNTS = (1, 7, 8, 9, 4100)


@pytest.mark.parametrize("dt,rdt,skipless", [p + (False,) for p in PAIRS] + [(d, d, True) for d in NULL_SKIP],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_kernel_bit_exact(dt, rdt, skipless):
    """per-row counts 1, 7, 8, 9, 4100 (scalar path, 16-byte path, more than one tile) as the five levels of one table; B = 1 and 3;
    N = 1 .. 4; in place and out of place; bases aligned and one element off"""
    ops = _ops()
    g = torch.Generator().manual_seed(31)
    ops.TIMER.start()
    try:
        n = 0
        for B in (1, 3):
            for N in (1, 2, 3, 4):
                for inplace in ((True,) if skipless else (True, False)):
                    for misaligned in (False, True):
                        _check_levels(ops, g, COUNTS, B, N, dt, rdt, skipless, inplace, misaligned)
                        n += 1
    finally:
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert counts == {"ed_control_residuals": n}, counts                       # ONE launch per table, and nothing else


# 13 levels (a SD 1.x UNet's 12 skips + the mid block) of different sizes: tile boundaries (4096 elements per batch row) fall inside
# levels (4097, 8200, 12289), ON level ends (4096, 8192, 12288) and levels smaller than a tile sit between them
LEVELS13 = (4096, 5, 4097, 8192, 64, 8200, 12288, 1, 12289, 4095, 16, 4104, 777)


@pytest.mark.parametrize("dt,rdt", [(F16, F16), (F32, BF16), (F32, F32)], ids=lambda v: str(v).replace("torch.", ""))
def test_table_of_13_levels(dt, rdt):
    ops = _ops()
    g = torch.Generator().manual_seed(32)
    for B, N in ((2, 2), (3, 4)):
        host, n_tiles = ops.control_table([(None, torch.empty(B, c), [torch.empty(B, c)] * N) for c in LEVELS13], N)
        assert n_tiles == B * sum(-(-c // ops.CONTROL_TILE) for c in LEVELS13)
        _check_levels(ops, g, LEVELS13, B, N, dt, rdt, False, True, False)


@pytest.mark.parametrize("dt,rdt", PAIRS, ids=lambda v: str(v).replace("torch.", ""))
def test_zero_weights_leave_the_residual_unread(dt, rdt):
    """per-row weights with zeros: the residual rows of the closed (row, net) pairs hold inf / NaN; the output is finite and exact"""
    ops = _ops()
    g = torch.Generator().manual_seed(33)
    B, N = 3, 3
    w = torch.tensor([[0.2, 0.0, 1.25], [0.0, 0.0, 0.7], [0.5, -0.3, 0.0]])
    for count in (9, 4104):
        s_cpu, s_dev = _rand(g, B, count, dt)
        rs = [_rand(g, B, count, rdt) for _ in range(N)]
        for n in range(N):
            for b in range(B):
                if w[b, n] == 0:
                    bad = torch.tensor([float("inf"), float("nan"), float("-inf")]).to(rdt).repeat(count // 3 + 1)[:count]
                    rs[n][0][b] = bad
                    rs[n][1][b] = bad.to(DEV)
        want = mc.control_residuals_cpu(s_cpu, [r[0] for r in rs], w)
        got = ops.control_residuals([s_dev], [[r[1]] for r in rs], w.to(DEV))[0].cpu()
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, want)


@pytest.mark.parametrize("dt,rdt", PAIRS, ids=lambda v: str(v).replace("torch.", ""))
def test_all_zero_weights(dt, rdt):
    """the output equals the skip (bits); with a null skip it is +0"""
    ops = _ops()
    g = torch.Generator().manual_seed(34)
    B, N = 2, 2
    w = torch.zeros(B, N, device=DEV)
    for count in (7, 4104):
        s_cpu, s_dev = _rand(g, B, count, dt)
        s_cpu[0, 0] = -0.0
        s_dev[0, 0] = -0.0
        rs = [torch.full((B, count), float("nan"), dtype=rdt, device=DEV) for _ in range(N)]
        out = torch.empty_like(s_dev)
        got = ops.control_residuals([s_dev], [[r] for r in rs], w, [out])[0]
        bits = torch.int32 if dt == F32 else torch.int16
        assert torch.equal(got.cpu().view(bits), s_cpu.view(bits))
        if dt == rdt:
            z = ops.control_residuals(None, [[r] for r in rs], w)[0].cpu()
            assert z.dtype == rdt and not z.view(bits).any()                    # +0: all bits clear


def test_rejections_launch_nothing_and_the_next_launch_is_correct():
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    L = _hip.lib()
    g = torch.Generator().manual_seed(35)
    B, N = 2, 2
    s_cpu, s_dev = _rand(g, B, 4100, F32)
    rs = [_rand(g, B, 4100, F16) for _ in range(N)]
    q_cpu, q_dev = _rand(g, B, 9, F32)
    qs = [_rand(g, B, 9, F16) for _ in range(N)]
    w = _weights(g, B, N)
    w_dev = w.to(DEV)
    out0, out1 = torch.full_like(s_dev, 7.0), torch.full_like(q_dev, 7.0)
    h_dev, hs = _rand(g, B, 9, F16)[1], [_rand(g, B, 9, F16)[1] for _ in range(N)]
    out2 = torch.full_like(h_dev, 7.0)
    levels = [(s_dev, out0, [r[1] for r in rs]), (q_dev, out1, [q[1] for q in qs]), (h_dev, out2, hs)]
    good, n_tiles = ops.control_table(levels, N)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    W = ops.CONTROL_LEVEL_WORDS

    def call(host, n_levels=3, n_nets=N, wp=None, tiles=n_tiles):
        return L.ed_control_residuals(host.data_ptr(), n_levels, n_nets, w_dev.data_ptr() if wp is None else wp, tiles, stream)

    def edited(word, value, level=0):
        t = good.clone()
        t[level * W + word] = value
        return t

    bad = [
        ("null out", edited(1, 0)), ("odd out", edited(1, out0.data_ptr() + 2)), ("odd skip", edited(0, s_dev.data_ptr() + 1)),
        ("count 0", edited(2, 0)), ("count < 0", edited(2, -8)), ("B of level 1 differs", edited(3, B + 1, 1)), ("B 0", edited(3, 0)),
        ("dtype code", edited(4, 3)), ("rdtype code", edited(5, -1)), ("f16 skip with bf16 residuals", edited(5, ops.ED_BF16, 2)),
        ("tile0 of level 0", edited(6, 1)), ("tile0 of level 1", edited(6, 1, 1)), ("reserved word", edited(7, 1)),
        ("null residual", edited(8, 0)), ("odd residual", edited(9, rs[1][1].data_ptr() + 1)),
        ("residual past n_nets", edited(10, rs[0][1].data_ptr())), ("out aliases a residual", edited(1, rs[0][1].data_ptr())),
        ("out overlaps the skip", edited(1, s_dev.data_ptr() + 16)),
    ]
    for what, host in bad:
        assert call(host) == INVALID, what
    assert call(good, n_nets=0) == INVALID and call(good, n_nets=ops.CONTROL_MAX_NETS + 1) == INVALID
    assert call(good, n_nets=3) == INVALID                                      # the table lists two residuals per level
    assert call(good, n_levels=0) == INVALID and call(good, n_levels=ops.CONTROL_MAX_LEVELS + 1) == INVALID
    assert call(good, tiles=n_tiles - 1) == INVALID and call(good, tiles=n_tiles + 1) == INVALID and call(good, tiles=0) == INVALID
    assert call(good, wp=0) == INVALID and call(good, wp=w_dev.data_ptr() + 2) == INVALID
    assert L.ed_control_residuals(None, 3, N, w_dev.data_ptr(), n_tiles, stream) == INVALID
    null_skip = good.clone()
    null_skip[0] = 0                                                            # without a skip, f32 out needs f32 residuals
    assert call(null_skip) == INVALID
    torch.cuda.synchronize()
    assert bool((out0 == 7.0).all()) and bool((out1 == 7.0).all()) and bool((out2 == 7.0).all())   # nothing was launched
    with pytest.raises(RuntimeError, match="ed_control_residuals"):             # ... and the wrapper raises on the same error
        ops._LAUNCH["device"] = w_dev.device
        ops._call("ed_control_residuals", edited(6, 1).data_ptr(), 3, N, w_dev.data_ptr(), n_tiles, stream)
    assert ops._LAUNCH["device"] is None
    with pytest.raises(ValueError, match="overlaps a residual"):
        ops.control_residuals([h_dev], [[hs[0]], [hs[1]]], w_dev, [hs[0]])
    assert call(good) == 0                                                      # the valid launch that follows is correct
    assert torch.equal(out0.cpu(), mc.control_residuals_cpu(s_cpu, [r[0] for r in rs], w))
    assert torch.equal(out1.cpu(), mc.control_residuals_cpu(q_cpu, [q[0] for q in qs], w))


def test_mismatched_strides_take_the_torch_sequence():
    """a channels-last skip with NCHW residuals: no launch, the same values"""
    ops = _ops()
    g = torch.Generator().manual_seed(36)
    skip = torch.randn(2, 8, 5, 6, generator=g).to(F16)
    r = torch.randn(2, 8, 5, 6, generator=g).to(F16)
    w = torch.tensor([[0.5], [0.0]])
    want = mc.control_residuals_cpu(skip, [r], w)
    s_dev = skip.to(DEV).contiguous(memory_format=torch.channels_last)
    ops.TIMER.start()
    try:
        got = ops.control_residuals([s_dev], [[r.to(DEV)]], w.to(DEV))[0]
    finally:
        counts = ops.TIMER.stop()
    assert "ed_control_residuals" not in counts and torch.equal(got.cpu(), want)
    cl = [t.to(DEV).contiguous(memory_format=torch.channels_last) for t in (skip, r)]      # both channels-last: the launch
    ops.TIMER.start()
    try:
        got = ops.control_residuals([cl[0]], [[cl[1]]], w.to(DEV))[0]
    finally:
        counts = ops.TIMER.stop()
    assert counts["ed_control_residuals"][0] == 1 and torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------
# end to end on the fakes
# ---------------------------------------------------------------------------------------------------
CASE = cases.E2E_CASES["cn_sd_512x1024"]          # the smallest padded ControlNet geometry: 64 x 128 latent, RePaint on, vbs 4
STARTS, ENDS = [0.0, 0.25], [0.5, 1.0]            # the two windows of the hand table (tests/test_multi_controlnet.py)
SCALES = [0.2, 0.5]


class CountingControlNet(FakeControlNet):
    def __init__(self, seed=11):
        super().__init__(seed)
        self.calls = 0

    def forward(self, *a, **kw):
        self.calls += 1
        return super().forward(*a, **kw)


class TimestepLog(FakeUNet):
    """FakeUNet that notes the timestep of every forward (graphs off: one Python call per forward)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def forward(self, x, t, **kw):
        self.seen.append(int(torch.as_tensor(t).flatten()[0]))
        return super().forward(x, t, **kw)


def _conditions():
    ds = eo.get_downsample_size(CASE["H"], CASE["W"], CASE["sd"])
    a = cases.synthetic_condition(ds[0] * 8, ds[1] * 8)
    b = (1.0 - a).flip(-1).roll(1, 1).contiguous()               # a second, different synthetic condition
    return a, b


def _loop_kw(steps=None):
    return dict(height=CASE["H"], width=CASE["W"], num_inference_steps=steps or CASE["steps"], resampling_steps=CASE["R"],
                **cases.E2E_KW)


def _pipe(controlnet, unet=None, text_encoder=None, **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    return ElasticDiffusion(DEV, CASE["sd"], view_batch_size=CASE["vbs"], unet=unet or FakeUNet(CASE["sample"]), vae=FakeVAE(),
                            text_encoder=text_encoder or V.embed_fn(False), controlnet=controlnet, **extra)


def _run(pipe, seed=None, **kw):
    pipe.seed_everything(CASE["seed"] if seed is None else seed)
    z = pipe.generate_latents("p", "", **kw).clone()
    return z, torch.rand(4)


@functools.lru_cache(maxsize=None)
def _legacy(scale):
    """the legacy single-net pipeline (net A = FakeControlNet(11)) on the first condition: (latent, RNG tail), once per scale"""
    return _run(_pipe(FakeControlNet(11)), **_loop_kw(), condition_image=_conditions()[0], controlnet_conditioning_scale=scale)


def test_list_of_one_net_is_the_legacy_pipeline_bit_for_bit():
    want, wtail = _legacy(0.2)
    z, tail = _run(_pipe([FakeControlNet(11)]), **_loop_kw(), condition_image=[_conditions()[0]], controlnet_conditioning_scale=[0.2])
    assert torch.equal(z, want) and torch.equal(tail, wtail)
    with pytest.raises(ValueError):                                         # a list of conditions with a net that is not listed
        _pipe(FakeControlNet(11)).generate_latents("p", "", **_loop_kw(), condition_image=[_conditions()[0]])
    with pytest.raises(ValueError):                                         # two conditions for one listed net
        _pipe([FakeControlNet(11)]).generate_latents("p", "", **_loop_kw(), condition_image=list(_conditions()))


def test_two_equal_nets_at_half_the_scale_each():
    want, wtail = _legacy(0.5)
    a = FakeControlNet(11)
    c = _conditions()[0]
    z, tail = _run(_pipe([a, copy.deepcopy(a)]), **_loop_kw(), condition_image=[c, c], controlnet_conditioning_scale=[0.25, 0.25])
    assert torch.equal(z, want) and torch.equal(tail, wtail)


def test_zero_scales_run_no_net():
    want, wtail = _legacy(0.0)
    nets = [CountingControlNet(11), CountingControlNet(12)]
    z, tail = _run(_pipe(nets), **_loop_kw(), condition_image=list(_conditions()), controlnet_conditioning_scale=[0.0, 0.0])
    assert torch.equal(z, want) and torch.equal(tail, wtail)
    assert [n.calls for n in nets] == [0, 0]


def _spec_nets(timesteps, starts=STARTS, ends=ENDS):
    return mc.MultiControlNetSpec([FakeControlNet(11), FakeControlNet(12)], timesteps, starts, ends)


def _stacked():
    return torch.cat(_conditions(), dim=1)


@functools.lru_cache(maxsize=None)
def _two_net_oracle(steps=4):
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    ts = [int(t) for t in DDIMSchedule().set_timesteps(steps)]
    spec = _spec_nets(ts)
    orc = eo.ElasticOracle(FakeUNet(CASE["sample"]), FakeVAE(), DDIMOracle(), V.embed_fn(False), sd_version=CASE["sd"],
                           view_batch_size=CASE["vbs"], controlnet=spec)
    orc.seed_everything(CASE["seed"])
    z = orc.generate_latent("p", "", **_loop_kw(steps), condition_image=_stacked(), controlnet_conditioning_scale=SCALES)
    return z, torch.rand(4), ts


MULTI_KW = dict(controlnet_conditioning_scale=SCALES, control_guidance_start=STARTS, control_guidance_end=ENDS)


def test_two_nets_two_windows_vs_oracle():
    """4 steps, windows (0, 0.5) and (0.25, 1): net 0 acts on steps 0 and 1, net 1 on steps 1, 2, 3 -- and neither runs elsewhere"""
    want, wtail, ts = _two_net_oracle()
    z, tail = _run(_pipe([FakeControlNet(11), FakeControlNet(12)]), **_loop_kw(4), condition_image=list(_conditions()), **MULTI_KW)
    err = rel_l2(z, want)
    print(f"two nets, two windows vs oracle: rel-L2 {err:.3e}")
    assert err < 1e-4, err
    assert torch.equal(tail, wtail)
    # graphs off: every forward is one Python call; the nets' call counts are the keep table's
    nets, unet = [CountingControlNet(11), CountingControlNet(12)], TimestepLog(CASE["sample"])
    z2, tail2 = _run(_pipe(nets, unet=unet, use_graphs=False), **_loop_kw(4), condition_image=list(_conditions()), **MULTI_KW)
    assert rel_l2(z2, want) < 1e-4 and torch.equal(tail2, wtail)
    keep = mc.control_keep(4, STARTS, ENDS)
    forwards = [sum(1 for t in unet.seen if t == ts[i]) for i in range(4)]
    assert sum(forwards) == len(unet.seen) and all(f >= 1 for f in forwards)
    for n in range(2):
        assert nets[n].calls == sum(f for f, k in zip(forwards, keep) if k[n] == 1.0), (n, nets[n].calls, forwards, keep)
    assert 0 < nets[0].calls < sum(forwards) and 0 < nets[1].calls < sum(forwards)


def test_with_strength_the_window_counts_executed_steps():
    """strength 0.5 of 4 steps: T = 2 executed steps, i = 0, 1 -- window (0, 0.5) keeps the first of them, (0.25, 1) the second"""
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    steps, strength = 4, 0.5
    t_start = I.window(steps, strength)
    ts = [int(t) for t in DDIMSchedule().set_timesteps(steps)][t_start:]
    assert len(ts) == 2 and mc.control_keep(2, STARTS, ENDS) == [[1.0, 0.0], [0.0, 1.0]]
    img = synthetic_image(CASE["H"], CASE["W"], seed=CASE["seed"])
    orc = I.Img2ImgOracle(FakeUNet(CASE["sample"]), FakeVAE(), V.DDIMVariants(), V.embed_fn(False), sd_version=CASE["sd"],
                          view_batch_size=CASE["vbs"], controlnet=_spec_nets(ts))
    orc.seed_everything(CASE["seed"])
    want = orc.generate_latent("p", "", **_loop_kw(steps), condition_image=_stacked(), controlnet_conditioning_scale=SCALES,
                               init_image=img, strength=strength)
    wtail = torch.rand(4)
    z, tail = _run(_pipe([FakeControlNet(11), FakeControlNet(12)]), **_loop_kw(steps), condition_image=list(_conditions()), **MULTI_KW,
                   init_image=img, strength=strength)
    err = rel_l2(z, want)
    print(f"strength 0.5: rel-L2 {err:.3e}")
    assert err < 1e-4 and torch.equal(tail, wtail)


def test_with_dpm_solver():
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    steps = 4
    ts = [int(t) for t in DDIMSchedule().set_timesteps(steps)]
    orc = D.SolverOracle(FakeUNet(CASE["sample"]), FakeVAE(), D.DPMSolverCPU(solver_order=2), V.embed_fn(False), sd_version=CASE["sd"],
                         view_batch_size=CASE["vbs"], controlnet=_spec_nets(ts))
    orc.seed_everything(CASE["seed"])
    want = orc.generate_latent(["p"], "", **_loop_kw(steps), condition_image=_stacked(), controlnet_conditioning_scale=SCALES)
    wtail = torch.rand(4)
    z, tail = _run(_pipe([FakeControlNet(11), FakeControlNet(12)], sampler="dpmsolver++"), **_loop_kw(steps),
                   condition_image=list(_conditions()), **MULTI_KW)
    err = rel_l2(z, want)
    print(f"dpmsolver++: rel-L2 {err:.3e}")
    assert err < 1e-4 and torch.equal(tail, wtail)


def test_interleaved_two_jobs_match_each_alone():
    def embed(prompts):  # stateless (the programs' calls interleave); the values V.embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe([FakeControlNet(11), FakeControlNet(12)], text_encoder=embed)
    a, b = _conditions()
    jobs = [dict(prompts="p", negative_prompts="", seed=CASE["seed"], condition_image=[a, b]),
            dict(prompts="p", negative_prompts="", seed=11, condition_image=[b, a])]
    alone = []
    for job in jobs:
        alone.append(_run(pipe, seed=job["seed"], **_loop_kw(4), condition_image=job["condition_image"], **MULTI_KW)[0])
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **_loop_kw(4), **MULTI_KW)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], _two_net_oracle()[0]) < 1e-4
    assert not torch.equal(got[0], got[1])


def test_a_change_of_scale_replays_the_captured_graphs():
    pipe = _pipe([FakeControlNet(11), FakeControlNet(12)])
    kw = dict(_loop_kw(), condition_image=list(_conditions()))
    z1, _ = _run(pipe, **kw, controlnet_conditioning_scale=[0.2, 0.5])
    before = pipe._runner.stats()
    assert before["captured"] >= 1 and before["eager"] == 0, before
    z2, _ = _run(pipe, **kw, controlnet_conditioning_scale=[0.4, 0.1])
    after = pipe._runner.stats()
    assert after["captured"] == before["captured"] and after["eager"] == 0 and after["replays"] > before["replays"], (before, after)
    assert rel_l2(z2, z1) > 1e-4                                               # the new weights reached the replays
    fresh, _ = _run(_pipe([FakeControlNet(11), FakeControlNet(12)]), **kw, controlnet_conditioning_scale=[0.4, 0.1])
    assert torch.equal(z2, fresh)


def test_two_single_net_active_sets_do_not_share_a_graph():
    """net 0 alone on the first half, net 1 alone on the second: both forwards take 3 condition channels; a graph keyed on the
    condition shape alone would replay net 0's forward for net 1"""
    kw = dict(_loop_kw(4), condition_image=list(_conditions()), controlnet_conditioning_scale=[0.3, 0.3],
              control_guidance_start=[0.0, 0.5], control_guidance_end=[0.5, 1.0])
    z, _ = _run(_pipe([FakeControlNet(11), FakeControlNet(12)]), **kw)
    eager, _ = _run(_pipe([FakeControlNet(11), FakeControlNet(12)], use_graphs=False), **kw)
    assert rel_l2(z, eager) < 1e-5
    # what the collision would compute: net 0 (on net 1's condition) in both halves
    a = FakeControlNet(11)
    collided, _ = _run(_pipe([a, copy.deepcopy(a)], use_graphs=False), **kw)
    assert rel_l2(z, collided) > 1e-4


# ---------------------------------------------------------------------------------------------------
# the real architecture against the fp64 specification
# ---------------------------------------------------------------------------------------------------
NET_HW = (16, 16)
W_ROWS = [[0.7, 0.3], [0.5, 0.0], [0.2, 0.9]]      # per-row weights of the batch of 3; one (row, net) pair closed


def _rounded(module, seed, dtype):
    from elasticdiffusion_official_amd import models as M
    M._seeded_init(module, seed)
    return {k: v.to(dtype) for k, v in S.randomise(module.state_dict(), seed).items()}


def _load(module, sd, dtype):
    from elasticdiffusion_official_amd import models as M
    module.load_state_dict(sd)
    module = module.to(DEV, dtype).eval().requires_grad_(False)
    return module.to(memory_format=torch.channels_last) if (M.CHANNELS_LAST and dtype != F32) else module


@functools.lru_cache(maxsize=None)
def _real_case(fam, dtype):
    """rounded parameters and inputs of the small UNet and two small ControlNets, and the spec's fp64 outputs: the two nets' lists
    summed with the per-row weights into the UNet, and net 0 alone at the spec's scale (the single-net yardstick)"""
    from elasticdiffusion_official_amd import models as M
    cfg = M.SMALL_UNET_CONFIGS[fam]
    usd = _rounded(M.UNet2DConditionModel(**cfg), 21, dtype)
    csds = [_rounded(M.ControlNetModel(cfg), 22 + n, dtype) for n in range(2)]
    raw = S.unet_inputs(cfg, NET_HW, seed=7)
    i64 = {k: (v.to(dtype).double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in raw.items()}
    if raw["added"] is not None:
        i64["added"] = dict(text_embeds=raw["added"]["text_embeds"].to(dtype).double(), time_ids=raw["added"]["time_ids"])
    conds = [i64["cond"], S.unet_inputs(cfg, NET_HW, seed=8)["cond"].to(dtype).double()]
    u64 = {k: v.double() for k, v in usd.items()}
    a = (i64["sample"], i64["t"], i64["context"])
    w = torch.tensor(W_ROWS, dtype=torch.float64)
    with torch.no_grad():
        lists = []
        for csd, cond in zip(csds, conds):
            down, mid = S.controlnet_forward({k: v.double() for k, v in csd.items()}, cfg, *a, cond, 1.0, i64["added"])
            lists.append(list(down) + [mid])
        summed = [sum(w[:, n].view(-1, 1, 1, 1) * lists[n][l] for n in range(2)) for l in range(len(lists[0]))]
        ref_multi = S.unet_forward(u64, cfg, *a, i64["added"], summed[:-1], summed[-1])
        single = [S.CONDITIONING_SCALE * r for r in lists[0]]
        ref_single = S.unet_forward(u64, cfg, *a, i64["added"], single[:-1], single[-1])
    return cfg, usd, csds, i64, conds, ref_multi, ref_single


@pytest.mark.parametrize("mode", ["fp32", "fp16", "fp16-stream32"])
@pytest.mark.parametrize("fam", ["sd15", "sdxl"])
def test_real_architecture_vs_fp64_spec(fam, mode):
    from elasticdiffusion_official_amd import models as M
    ops = _ops()
    dtype = F32 if mode == "fp32" else F16
    cfg, usd, csds, i64, conds, ref_multi, ref_single = _real_case(fam, dtype)
    unet = _load(M.UNet2DConditionModel(**cfg), usd, dtype)
    unet.residual_fp32 = mode == "fp16-stream32"
    nets = [_load(M.ControlNetModel(cfg), csd, dtype) for csd in csds]
    added = None if i64["added"] is None else dict(text_embeds=i64["added"]["text_embeds"].to(DEV, dtype),
                                                   time_ids=i64["added"]["time_ids"].to(DEV))
    x, t, ctx = i64["sample"].to(DEV, dtype), i64["t"].to(DEV), i64["context"].to(DEV, dtype)
    cds = [c.to(DEV, dtype) for c in conds]
    w = torch.tensor(W_ROWS, dtype=F32, device=DEV)
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    ops.TIMER.start()
    try:
        with torch.no_grad():
            kw = dict(encoder_hidden_states=ctx, added_cond_kwargs=added)
            # the yardstick: today's single-net path with net 0
            d, m = nets[0](x, t, controlnet_cond=cds[0], conditioning_scale=S.CONDITIONING_SCALE, **kw)
            single = unet(x, t, down_block_additional_residuals=d, mid_block_additional_residual=m, **kw).sample
            raws = [net(x, t, controlnet_cond=c, raw_residuals=True, **kw) for net, c in zip(nets, cds)]
            # null-skip sums handed over through the legacy keywords (first: the fused form writes nothing of the raws, but keep order plain)
            sums = ops.control_residuals(None, [list(dn) + [md] for dn, md in raws], w)
            unfused = unet(x, t, down_block_additional_residuals=sums[:-1], mid_block_additional_residual=sums[-1], **kw).sample
            fused = unet(x, t, control_residuals=([dn for dn, _ in raws], [md for _, md in raws], w), **kw).sample
    finally:
        torch.backends.cudnn.deterministic = keep
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert counts["ed_control_residuals"] == 2, counts                         # ONE launch per hand-off
    e_single, e_fused, e_unfused = rel_l2(single, ref_single), rel_l2(fused, ref_multi), rel_l2(unfused, ref_multi)
    e_forms = rel_l2(fused, unfused)
    print(f"{fam} {mode}: single net {e_single:.3e} (bar {2 * e_single:.3e}); two nets fused {e_fused:.3e}, "
          f"null-skip sum then add {e_unfused:.3e}, fused vs that {e_forms:.3e}")
    assert bool(torch.isfinite(fused).all())
    assert e_fused < 2 * e_single, (e_fused, e_single)
    assert e_forms < 2 * e_single, (e_forms, e_single)


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_two_controlnets_and_a_window(tmp_path, golden_dir):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    photo = os.path.join(golden_dir, "canny_input_yoga.jpeg")
    flipped = str(tmp_path / "flipped.png")
    Image.open(photo).transpose(Image.FLIP_LEFT_RIGHT).save(flipped)
    save_dir = main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1",
                     "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4",
                     "--process_condition", "true",
                     "--condition_image", photo, "--controlnet_model", "canny", "--controlnet_conditioning_scale", "0.2",
                     "--condition_image", flipped, "--controlnet_model", "canny", "--controlnet_conditioning_scale", "0.5",
                     "--control_guidance_end", "0.5", "--control_guidance_end", "1.0"])
    files = {os.path.basename(f) for f in glob.glob(os.path.join(save_dir, "*"))}
    assert {"0.png", "condition_0.png", "condition_1.png", "args.txt"} <= files and "condition.png" not in files, files
    assert Image.open(os.path.join(save_dir, "0.png")).size == (512, 512)
    c0, c1 = (np.asarray(Image.open(os.path.join(save_dir, f"condition_{n}.png"))) for n in range(2))
    assert c0.shape == c1.shape == (512, 512, 3) and not np.array_equal(c0, c1)
    args = open(os.path.join(save_dir, "args.txt")).read()
    assert "controlnet_conditioning_scale: [0.2, 0.5]" in args and "control_guidance_end: [0.5, 1.0]" in args
    with pytest.raises(SystemExit):                                             # two conditions, three scales
        main(["--sd_version", "1.5", "--condition_image", photo, "--condition_image", flipped, "--controlnet_model", "canny",
              "--controlnet_model", "canny", "--controlnet_conditioning_scale", "0.1", "--controlnet_conditioning_scale", "0.2",
              "--controlnet_conditioning_scale", "0.3"])
