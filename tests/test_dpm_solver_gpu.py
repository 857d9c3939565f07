"""-m gpu: DPM-Solver++(2M) through the HIP path.

Bars (the project's existing ones):
  * kernels fed identical fp32 inputs: BIT-EXACT against the specification's torch-CPU op sequence (tests/dpm_solver_cpu.py);
  * the fused epilogue with ``multistep``: bit-identical to the chain of separate kernels with ``multistep``;
  * end to end against ``SolverOracle`` and the G16 fixture: latent rel-L2 < 1e-4, host RNG stream in exactly the same end state;
    interleaved against alone 1e-5;
  * the Gaussian-ODE inequality of tests/test_dpm_solver.py again, through the kernel loop;
  * ``sampler="ddim"`` launches exactly the entry points it launched before and gives the same bits.
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import dpm_solver_cpu as D
from tests.ddim_variants import embed_fn
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE, synthetic_text_embeds
from tests.glue_geometries import FUSED_ROWS, misaligned
from tests.golden import cases
from tests.test_hip_parity import DEV, dev_i32, rel_l2

pytestmark = pytest.mark.gpu

NEW_ENTRY_POINTS = ("ed_cfg_ddim_step_ms", "ed_phase_epilogue_ms")
V_TRAILING_ZSNR = dict(prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True)


def _mods():
    from elasticdiffusion_official_amd import geometry, ops, schedule
    return geometry, ops, schedule


def _schedules(kw, steps, order=2):
    _, _, schedule = _mods()
    prod, spec = schedule.DPMSolverSchedule(solver_order=order, **kw), D.DPMSolverCPU(solver_order=order, **kw)
    ts = prod.set_timesteps(steps)
    spec.set_timesteps(steps)
    assert torch.equal(ts, spec.timesteps)
    return prod, spec, ts


# ---------------------------------------------------------------------------------------------------
# the flat step, bit-exact
# ---------------------------------------------------------------------------------------------------
# (scheduler settings, steps, timestep index): mid-schedule at second order, the last step, and -- v-prediction on zero-SNR betas --
# the abar_t = 0 timestep itself (first order, no history) and the one after it (first order forced: abar of the history is 0)
FLAT_SCHEDULES = [(dict(), 20, 7), (dict(), 20, 19), (dict(prediction_type="v_prediction"), 20, 7), (V_TRAILING_ZSNR, 5, 0),
                  (V_TRAILING_ZSNR, 5, 1), (V_TRAILING_ZSNR, 5, 2)]


def _flat_case(kw, steps, ti, n, with_hist, with_ratio, B=1):
    prod, spec, ts = _schedules(kw, steps)
    g = torch.Generator().manual_seed(steps * 1000 + ti * 10 + n % 7)
    local, direction, x, x0h = (torch.randn(n, generator=g) for _ in range(4))
    guidance = 10.0 / 3
    t = ts[ti]
    t_hist = ts[ti - 1] if with_hist and ti > 0 else None
    m = local + guidance * direction
    ratio = None
    if with_ratio:
        from tests.guidance_rescale_cpu import rescale_with_ratio
        ratio = torch.tensor([0.8, 1.1, 0.95, 1.3][:B])
        m = rescale_with_ratio(m.view(B, -1), ratio, 0.7).view(-1)
    want = spec.step(m, t, x, history=None if t_hist is None else (x0h, t_hist), is_last=ti == steps - 1)
    coef = prod.multistep_coefficients(t, t_hist, ti == steps - 1)
    second = coef[5] != 0.0
    assert second == spec.second_order(t, t_hist, ti == steps - 1)
    return prod, coef, (local, direction, x), x0h if second else None, guidance, ratio, want


@pytest.mark.parametrize("with_ratio", [False, True])
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1028, 4 * 1025])
@pytest.mark.parametrize("kw,steps,ti", FLAT_SCHEDULES)
def test_cfg_ddim_step_multistep_bit_exact(kw, steps, ti, n, with_hist, with_ratio):
    _, ops, _ = _mods()
    B = 2 if with_ratio and n == 4 * 1025 else 1      # two samples of 2050 elements: no whole number of float4s, the scalar form
    prod, coef, ins, x0h, guidance, ratio, want = _flat_case(kw, steps, ti, n, with_hist, with_ratio, B)
    if kw.get("rescale_betas_zero_snr") and ti == 0:
        assert float(prod.alphas_cumprod[int(prod.timesteps[0])]) == 0.0 and coef[1] == 0.0
    pt = kw.get("prediction_type", "epsilon")
    kws = dict(prediction_type=pt)
    if ratio is not None:
        kws.update(ratio=ratio.to(DEV), guidance_rescale=0.7)
    dev_ins = [t.to(DEV) for t in ins]
    hist = None if x0h is None else x0h.to(DEV)
    prev, x0 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *coef[:2], 0.0, 0.0, multistep=coef[2:] + (hist,), **kws)
    assert bool(torch.isfinite(prev).all())
    assert torch.equal(x0.cpu(), want["pred_original_sample"])
    assert torch.equal(prev.cpu(), want["prev_sample"])
    # the scalar path: every operand in turn (the history among them) 4 bytes off a 16-byte boundary gives the same bits
    whole = ops.cfg_ddim_step_width(*dev_ins, prev, x0, kws.get("ratio"))
    assert whole == (4 if n % 4 == 0 and (ratio is None or (n // B) % 4 == 0) else 1)
    for k in range(6 if hist is not None else 5):
        args = dev_ins + [torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV), hist]
        args[k] = misaligned(args[k])
        if k < 5:
            assert ops.cfg_ddim_step_width(*args[:5], kws.get("ratio")) == 1
        ops.cfg_ddim_step(*args[:5], np.float32(guidance), *coef[:2], 0.0, 0.0, multistep=coef[2:] + (args[5],), **kws)
        assert torch.equal(args[3], prev) and torch.equal(args[4], x0), k


def test_cfg_ddim_step_multistep_is_not_the_ddim_step_and_order_matters():
    _, ops, _ = _mods()
    prod, coef, ins, x0h, guidance, _, want = _flat_case(dict(), 20, 7, 1028, True, False)
    dev_ins = [t.to(DEV) for t in ins]
    out = {}
    for label, kw in (("ddim", {}), ("ms1", dict(multistep=coef[2:] + (None,))), ("ms2", dict(multistep=coef[2:] + (x0h.to(DEV),)))):
        prev, x0 = torch.empty(1028, device=DEV), torch.empty(1028, device=DEV)
        ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *prod.step_coefficients(prod.timesteps[7]), **kw)
        out[label] = (prev, x0)
    assert torch.equal(out["ddim"][1], out["ms1"][1]) and torch.equal(out["ms1"][1], out["ms2"][1])   # one x0
    assert rel_l2(out["ms1"][0], out["ddim"][0]) < 1e-5 and not torch.equal(out["ms2"][0], out["ms1"][0])  # order 1 IS DDIM, to rounding
    assert torch.equal(out["ms2"][0].cpu(), want["prev_sample"])


def test_cfg_ddim_step_multistep_argument_errors():
    _, ops, _ = _mods()
    prod, coef, ins, x0h, guidance, _, _ = _flat_case(dict(), 20, 7, 1028, True, False)
    dev_ins = [t.to(DEV) for t in ins]
    prev, x0 = torch.full((1028,), 3.0, device=DEV), torch.full((1028,), 3.0, device=DEV)

    def call(ms, prev=prev, x0=x0, **kw):
        ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *coef[:2], 0.0, 0.0, multistep=ms, **kw)

    with pytest.raises(RuntimeError, match="overlaps x0"):      # in place: the history is the x0 being written
        call(coef[2:] + (x0,))
    with pytest.raises(RuntimeError, match="overlaps prev"):
        call(coef[2:] + (prev,))
    buf = torch.zeros(2 * 1028, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):         # a partial overlap
        call(coef[2:] + (buf[514:514 + 1028],), x0=buf[:1028])
    with pytest.raises(RuntimeError, match="multistep must be"):
        call(coef[2:])
    with pytest.raises(RuntimeError, match="x0_hist must be"):
        call(coef[2:] + (x0h.to(DEV)[:100],))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(coef[2:] + (x0h,))
    with pytest.raises(RuntimeError, match="prediction_type"):
        call(coef[2:] + (None,), prediction_type="sample")
    assert float(prev.min()) == 3.0 and float(x0.min()) == 3.0     # nothing was launched
    assert ops._LAUNCH["device"] is None
    # the library refuses the same on its own (hipErrorInvalidValue = 1, before any launch)
    from elasticdiffusion_official_amd import _hip
    L = _hip.lib()
    p = [t.data_ptr() for t in dev_ins] + [prev.data_ptr(), x0.data_ptr()]
    st = torch.cuda.current_stream(DEV).cuda_stream
    assert L.ed_cfg_ddim_step_ms(*p, 1.0, *coef, 1028, 0, None, 0.0, 0.0, 0, x0.data_ptr(), st) == 1
    assert L.ed_cfg_ddim_step_ms(*p, 1.0, *coef, 1028, 0, None, 0.0, 0.0, 0, prev.data_ptr() + 4, st) == 1
    assert L.ed_cfg_ddim_step_ms(*p, 1.0, *coef, 1028, 7, None, 0.0, 0.0, 0, None, st) == 1
    torch.cuda.synchronize()
    assert float(prev.min()) == 3.0 and float(x0.min()) == 3.0


# ---------------------------------------------------------------------------------------------------
# the fused epilogue with multistep == the chain of separate kernels with multistep, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_ROWS)
@pytest.mark.parametrize("B,K,dtype", [(1, 4, torch.float32), (2, 1, torch.bfloat16), (1, 8, torch.float16)])
@pytest.mark.parametrize("kw,with_hist,rescale", [(dict(), True, False), (dict(), False, False),
                                                  (dict(prediction_type="v_prediction"), True, True)])
def test_fused_epilogue_multistep_equals_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype, kw, with_hist, rescale):
    geometry, ops, _ = _mods()
    from elasticdiffusion_official_amd import host_rng
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    g = torch.Generator().manual_seed(Hl * 131 + Wl + K)
    x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    x0h = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    torch.manual_seed(17)
    stamp = torch.empty(h * w, 4, dtype=torch.int8)
    idx = host_rng.PickSampler(h * w).draw(K, 0.7, lambda: None, stamp=stamp).to(DEV)
    stamp = stamp.to(DEV)
    T = {k: dev_i32(getattr(pp, k)) for k in ("src_row", "src_col", "inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col")}
    cover = tuple(dev_i32(a) for a in vp.cover_tables(vpad.top, vpad.left))
    pick = tuple(T[k] for k in ("inv_row", "inv_col", "up_row", "up_col", "down_row", "down_col"))
    n_g, n_v = 2 * K * B, vp.V * B
    g_rows = torch.empty(n_g, 4, gpad.PH, gpad.PW, device=DEV, dtype=dtype)
    low = torch.empty(K, B, 4, h, w, device=DEV)
    ops.pick_assemble(x, idx, T["src_row"], T["src_col"], g_rows, h, w, gpad.top, gpad.left, None, low)
    g_out = torch.randn(n_g, 4, gpad.PH, gpad.PW, generator=g).to(dtype).to(DEV)
    v_cpu = torch.randn(n_v, 4, vpad.PH, vpad.PW, generator=g)
    v_cpu[torch.rand(v_cpu.shape, generator=g) < 0.2] = 0.0
    v_out = v_cpu.to(dtype).to(DEV)
    prod, _, ts = _schedules(kw, 20)
    coef = prod.multistep_coefficients(ts[7], ts[6], False)
    ddim = prod.step_coefficients(ts[7])
    assert coef[5] != 0.0
    ms = coef[2:] + (x0h if with_hist else None,)
    guidance, w_rrg, norm = np.float32(10.0 / 3), np.float32(437.53), np.float32(2.0 / (4 * Hl * Wl))
    pt_kw = dict(prediction_type=kw.get("prediction_type", "epsilon"))
    dirs = torch.empty(K, B, 4, h, w, device=DEV)
    unc1, ldir1 = torch.empty(B, 4, h, w, device=DEV), torch.empty(B, 4, h, w, device=DEV)
    direction1, local1 = torch.empty_like(x), torch.empty_like(x)
    prev1, x01, nxt1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ops.unpad_direction(g_out, dirs, unc1, gpad.top, gpad.left)
    ops.fill_directions(dirs, stamp, T["inv_row"], T["inv_col"], T["up_row"], T["up_col"], T["down_row"], T["down_col"],
                        direction1, ldir1)
    ops.scatter_centres(v_out, local1, vp.n_col_blocks, *cover)
    flat_rs, rrg_rs, epi_rs = {}, {}, {}
    if rescale:
        ratio, ratio_low = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
        wsp = ops.guidance_moments_workspace(B, 4 * Hl * Wl, 4 * h * w, DEV)
        ops.guidance_moments(local1, direction1, guidance, ratio, wsp)
        ops.guidance_moments(unc1, ldir1, guidance, ratio_low, wsp)
        flat_rs = dict(ratio=ratio, guidance_rescale=0.7)
        rrg_rs = dict(ratio_low=ratio_low, guidance_rescale=0.7)
        epi_rs = dict(ratio=ratio, ratio_low=ratio_low, guidance_rescale=0.7)
    ops.cfg_ddim_step(local1, direction1, x, prev1, x01, guidance, *ddim, multistep=ms, **pt_kw, **flat_rs)
    ops.rrg_update(prev1, x01, low[K - 1], unc1, ldir1, T["up_row"], T["up_col"], nxt1, guidance, ddim[0], ddim[1], norm,
                   w_rrg, **pt_kw, **rrg_rs)
    assert bool(torch.isfinite(nxt1).all())
    # with x_next (fused RRG: it reads this step's x0, whatever the sample update) and every by-product
    out = {k: torch.full_like(x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    unc2, ldir2 = torch.full_like(unc1, 5.0), torch.full_like(ldir1, 5.0)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       ddim, out["prev"], out["x0"], low_dir=ldir2, uncond_last=unc2, direction=out["direction"],
                       local=out["local"], x_next=out["x_next"], low_latent=low[K - 1], rrg_norm=norm, rrg_weight=w_rrg,
                       multistep=ms, **pt_kw, **epi_rs)
    for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1)):
        assert torch.equal(out[name], want), name
    assert torch.equal(unc2, unc1) and torch.equal(ldir2, ldir1)
    # without x_next and without the optional outputs
    p3, z3 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       ddim, p3, z3, multistep=ms, **pt_kw, **{k: v for k, v in epi_rs.items() if k != "ratio_low"})
    assert torch.equal(p3, prev1) and torch.equal(z3, x01)
    # the multistep launch is not the DDIM launch, and a history in place is refused
    p4, z4 = torch.empty_like(x), torch.empty_like(x)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       ddim, p4, z4, **pt_kw, **{k: v for k, v in epi_rs.items() if k != "ratio_low"})
    assert torch.equal(z4, z3)                                   # one x0 whatever the sample update
    assert rel_l2(p4, p3) > 1e-4 if with_hist else rel_l2(p4, p3) < 1e-5   # first order IS the DDIM step, to rounding
    with pytest.raises(RuntimeError, match="overlaps x0"):
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                           ddim, p4, z4, multistep=coef[2:] + (z4,), **pt_kw)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _pipe(name, order=2, text_encoder=None, sched=None, **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DPMSolverSchedule
    c = D.SOLVER_CASES[name]
    if c.get("controlnet"):
        extra["controlnet"] = FakeControlNet()
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=D.VBS, unet=FakeUNet(c["sample"]), vae=FakeVAE(),
                            text_encoder=text_encoder or embed_fn(False),
                            scheduler=sched or DPMSolverSchedule(solver_order=order, **c["sched"]), **extra)


_ORACLE = {}


def _oracle_run(name, order=2, **kw):
    """SolverOracle's (latent, RNG tail) for a case with extra loop keywords, computed once and shared"""
    key = (name, order, tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _ORACLE:
        c = D.SOLVER_CASES[name]
        orc = D.SolverOracle(FakeUNet(c["sample"]), FakeVAE(), D.DPMSolverCPU(solver_order=order, **c["sched"]), embed_fn(False),
                             sd_version=c["sd"], view_batch_size=D.VBS, controlnet=FakeControlNet() if c.get("controlnet") else None)
        orc.seed_everything(D.SEED)
        z = orc.generate_latent(["p"], "", **D.case_kwargs(name), **D.condition_kwargs(name), **kw)
        _ORACLE[key] = (z, torch.rand(4))
    return _ORACLE[key]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(D.SOLVER_CASES))
def test_end_to_end_vs_fixture_and_oracle(golden_dir, name, order):
    from elasticdiffusion_official_amd import ops
    g = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    pipe = _pipe(name, order)
    pipe.seed_everything(D.SEED)
    ops.TIMER.start()
    try:
        z = pipe.generate_latents("p", "", **D.case_kwargs(name), **D.condition_kwargs(name)).cpu()
        tail = torch.rand(4)
    finally:
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    want = torch.from_numpy(g[f"{name}/order{order}/latent"])
    err = rel_l2(z, want)
    print(f"{name} order {order}: rel-L2 vs G16 {err:.3e}")
    assert z.shape == want.shape and err < 1e-4, err
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/order{order}/rng_tail"])
    if order == 2:
        oz, otail = _oracle_run(name, 2)
        assert rel_l2(z, oz) < 1e-4 and torch.equal(otail, tail)
    c = D.SOLVER_CASES[name]
    phases = 2 * c["steps"] - 1 if D.case_kwargs(name)["repaint_sampling"] else c["steps"]
    assert counts["ed_phase_epilogue_ms"] == phases and "ed_phase_epilogue" not in counts, counts


def test_end_to_end_with_separate_glue_kernels(golden_dir):
    """FUSED_GLUE off: ed_cfg_ddim_step_ms carries the loop; same bar, and bit-identical to the fused path"""
    from elasticdiffusion_official_amd import ops, pipeline
    name = "eps_leading_repaint"
    g = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    lat, tails, counts = {}, {}, {}
    for fused in (False, True):
        pipeline.FUSED_GLUE = fused
        ops.TIMER.start()
        try:
            pipe = _pipe(name)
            pipe.seed_everything(D.SEED)
            lat[fused] = pipe.generate_latents("p", "", **D.case_kwargs(name)).cpu()
            tails[fused] = torch.rand(4)
        finally:
            pipeline.FUSED_GLUE = True
            counts[fused] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert rel_l2(lat[False], torch.from_numpy(g[f"{name}/order2/latent"])) < 1e-4
    np.testing.assert_array_equal(tails[False].numpy(), g[f"{name}/order2/rng_tail"])
    assert torch.equal(lat[False], lat[True])
    assert counts[False]["ed_cfg_ddim_step_ms"] == 2 * D.SOLVER_CASES[name]["steps"] - 1 and "ed_phase_epilogue_ms" not in counts[False]


def _picture(H, W, seed=5):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H // 8, W // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 255
    return img, mask


def test_img2img_with_mask_at_half_strength_vs_oracle():
    """the history starts empty at t_start: the first executed step is first order"""
    name = "eps_leading_repaint"
    c = D.SOLVER_CASES[name]
    img, mask = _picture(c["H"], c["W"])
    want, otail = _oracle_run(name, 2, init_image=img, strength=0.5, mask_image=mask)
    pipe = _pipe(name)
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs(name), init_image=img, strength=0.5, mask_image=mask).cpu()
    tail = torch.rand(4)
    print(f"img2img + mask, strength 0.5: rel-L2 {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4 and torch.equal(tail, otail)


def test_guidance_rescale_with_v_prediction_vs_oracle():
    name = "v_trailing"
    want, otail = _oracle_run(name, 2, guidance_rescale=0.7)
    pipe = _pipe(name)
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs(name), guidance_rescale=0.7).cpu()
    tail = torch.rand(4)
    print(f"guidance_rescale 0.7, v / trailing: rel-L2 {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4 and torch.equal(tail, otail)
    assert rel_l2(z, _oracle_run(name, 2)[0]) > 1e-3


def test_interleaved_two_jobs_equal_each_alone(golden_dir):
    """the history is per job: two images in flight do not read each other's x0"""
    name = "eps_leading_repaint"
    g = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    kw = D.case_kwargs(name)
    seeds = [D.SEED, 11, 12]

    def embed(prompts):  # stateless (the programs' calls interleave); the values embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe(name, text_encoder=embed)
    alone = []
    for s in seeds:
        pipe.seed_everything(s)
        alone.append(pipe.generate_latents("p", "", **kw).clone())
    got = pipe.generate_latents_interleaved([dict(prompts="p", negative_prompts="", seed=s) for s in seeds], in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], torch.from_numpy(g[f"{name}/order2/latent"])) < 1e-4
    assert rel_l2(got[0], got[1]) > 1e-2


def test_sampler_keyword_builds_the_schedule():
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule, DPMSolverSchedule
    name = "eps_norepaint"
    kw = dict(view_batch_size=D.VBS, unet=FakeUNet(64), vae=FakeVAE())
    pipe = ElasticDiffusion(DEV, "1.5", text_encoder=embed_fn(False), sampler="dpmsolver++", **kw)
    assert type(pipe.scheduler) is DPMSolverSchedule and pipe.scheduler.solver_order == 2
    assert ElasticDiffusion(DEV, "1.5", sampler="dpmsolver++", solver_order=1, **kw).scheduler.solver_order == 1
    assert type(ElasticDiffusion(DEV, "1.5", **kw).scheduler) is DDIMSchedule
    assert type(ElasticDiffusion(DEV, "1.5", sampler="ddim", **kw).scheduler) is DDIMSchedule
    with pytest.raises(ValueError, match="sampler"):
        ElasticDiffusion(DEV, "1.5", sampler="euler", **kw)
    with pytest.raises(ValueError, match="scheduler object"):
        ElasticDiffusion(DEV, "1.5", sampler="dpmsolver++", scheduler=DDIMSchedule(), **kw)
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs(name)).cpu()
    assert torch.equal(z, _pipe_run(name))


_PIPE_RUNS = {}


def _pipe_run(name):
    if name not in _PIPE_RUNS:
        pipe = _pipe(name)
        pipe.seed_everything(D.SEED)
        _PIPE_RUNS[name] = pipe.generate_latents("p", "", **D.case_kwargs(name)).cpu()
    return _PIPE_RUNS[name]


@pytest.mark.parametrize("name", ["gen_sd_pad_32x64", "gen_xl_64x128"])
def test_generate_vs_oracle(name):
    """``generate()``, the plain CFG loop: the previous iteration's x0 is the history"""
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DPMSolverSchedule
    c = cases.G11_CASES[name]
    xl = c["sd"].startswith("XL")
    (un, pun), (co, pco) = synthetic_text_embeds(1, xl=xl)
    text, pooled = torch.cat([un, co]), torch.cat([pun, pco])
    size = (4 * 8 * c["h"], 4 * 8 * c["w"])
    pipe = ElasticDiffusion(DEV, c["sd"], log_freq=1, unet=FakeUNet(c["sample"], xl=xl), vae=FakeVAE(),
                            scheduler=DPMSolverSchedule(lower_order_final=False))
    pipe.default_size = size
    pipe.scheduler.set_timesteps(c["steps"])
    pipe.seed_everything(c["seed"])
    z = torch.randn(1, 4, c["h"], c["w"])
    seen = {}
    dec = pipe.decode_latents
    pipe.decode_latents = lambda lat: (seen.__setitem__("z", lat.clone()), dec(lat))[1]
    _, info = pipe.generate(z, text, pooled, guidance_scale=c["guidance"])
    tail = torch.rand(4)
    results = {}
    for sampler in D.SAMPLERS:
        orc = D.SolverOracle(FakeUNet(c["sample"], xl=xl), FakeVAE(), D.DPMSolverCPU(sampler=sampler, lower_order_final=False),
                             sd_version=c["sd"], pooled_dim=16 if xl else None)
        orc.default_size = size
        orc.scheduler.set_timesteps(c["steps"])
        orc.seed_everything(c["seed"])
        results[sampler] = orc.plain_cfg_generate(torch.randn(1, 4, c["h"], c["w"]), text, pooled, c["guidance"])
        otail = torch.rand(4)
    latent, inter = results["dpmsolver++"]
    assert rel_l2(seen["z"], latent) < 1e-4, rel_l2(seen["z"], latent)
    assert rel_l2(torch.cat(info["inter_x0"]), torch.cat(inter)) < 1e-4
    assert rel_l2(seen["z"], results["ddim"][0]) > 1e-3
    assert torch.equal(tail, otail)


# ---------------------------------------------------------------------------------------------------
# the Gaussian ODE through the kernel loop
# ---------------------------------------------------------------------------------------------------
def _gauss_kernel_error(steps, sampler):
    """the chain of tests/dpm_solver_cpu.py::gauss_error with every step a launch: local = eps*(x, t), direction = 0"""
    _, ops, schedule = _mods()
    sch = schedule.DPMSolverSchedule() if sampler == "dpmsolver++" else schedule.DDIMSchedule()
    ts = sch.set_timesteps(steps)
    x_T = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    x = x_T.to(DEV)
    zero = torch.zeros_like(x)
    hist = None
    for i, t in enumerate(ts):
        abar = sch.alphas_cumprod[int(t)]
        local = ((1 - abar) ** 0.5).item() * x / D.gauss_var(abar).item()
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        kw = {}
        if sampler == "dpmsolver++":
            coef = sch.multistep_coefficients(t, None if hist is None else hist[1], i == steps - 1)
            kw = dict(multistep=coef[2:] + (hist[0] if coef[5] != 0.0 else None,))
        ops.cfg_ddim_step(local, zero, x, prev, x0, np.float32(7.5), *sch.step_coefficients(t), **kw)
        hist, x = (x0, t), prev
    spec = D.DPMSolverCPU()
    spec.set_timesteps(steps)
    want = D.gauss_exact_end(spec, x_T)
    return float((x.cpu().double() - want).norm() / want.norm())


def test_gaussian_ode_through_the_kernels():
    err = {(k, s): _gauss_kernel_error(k, s) for k in (20, 25, 50, 100) for s in D.SAMPLERS if k != 100 or s == "ddim"}
    for k in (20, 25, 50):
        ddim, ms = err[(k, "ddim")], err[(k, "dpmsolver++")]
        print(f"Gaussian ODE on the device, {k} steps: DDIM {ddim:.3e}, 2M {ms:.3e}, ratio {ms / ddim:.2f}")
        assert ms <= 0.5 * ddim, (k, ms, ddim)
    assert err[(25, "dpmsolver++")] < err[(100, "ddim")], err


# ---------------------------------------------------------------------------------------------------
# opt-in: the DDIM sampler is the loop as it was
# ---------------------------------------------------------------------------------------------------
def test_ddim_sampler_launches_what_it_always_launched(golden_dir):
    from elasticdiffusion_official_amd import ElasticDiffusion, ops
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)
    lat, counts = {}, {}
    for label, extra in (("omitted", {}), ("ddim", dict(sampler="ddim", solver_order=2)), ("dpm", dict(sampler="dpmsolver++"))):
        pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"]), vae=FakeVAE(),
                                text_encoder=embed_fn(False), **extra)
        pipe.seed_everything(c["seed"])
        ops.TIMER.start()
        try:
            lat[label] = pipe.generate_latents("p", "", **kw).cpu()
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert torch.equal(lat["omitted"], lat["ddim"]) and counts["omitted"] == counts["ddim"]
    phases = 2 * c["steps"] - 1
    glue = {k: v for k, v in counts["ddim"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k or "ddim" in k}
    assert glue == {"ed_assemble_rows": phases, "ed_phase_epilogue": phases, "ed_undo_step": c["steps"] - 1}, counts["ddim"]
    assert not any(k in counts["ddim"] for k in NEW_ENTRY_POINTS)
    assert rel_l2(lat["ddim"], torch.from_numpy(g[f"{name}/latent"])) < 1e-4
    # the multistep sampler: the same number of launches, one entry point exchanged
    swapped = {("ed_phase_epilogue_ms" if k == "ed_phase_epilogue" else k): v for k, v in counts["ddim"].items()}
    assert counts["dpm"] == swapped and rel_l2(lat["dpm"], lat["ddim"]) > 1e-3


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_sampler_flags(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    base = ["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "3", "--resampling_steps", "1", "--outdir",
            str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4"]
    d0 = main(base + ["--exp", "default"])
    d1 = main(base + ["--exp", "dpm", "--sampler", "dpmsolver++"])
    d2 = main(base + ["--exp", "dpm_v", "--sampler", "dpmsolver++", "--solver_order", "1", "--prediction_type", "v_prediction"])
    a0, a1, a2 = (np.asarray(Image.open(os.path.join(d, "0.png")), dtype=np.float32) for d in (d0, d1, d2))
    assert a0.shape == a1.shape == a2.shape == (512, 512, 3) and np.isfinite(a1).all()
    assert a1.std() > 0 and a2.std() > 0  # a NaN latent decodes to a constant image
    assert not np.array_equal(a0, a1) and not np.array_equal(a1, a2)
    args = open(os.path.join(d1, "args.txt")).read()
    assert "sampler: dpmsolver++" in args and "solver_order: 2" in args
    assert "sampler: ddim" in open(os.path.join(d0, "args.txt")).read()
    assert glob.glob(os.path.join(d1, "*.png"))
