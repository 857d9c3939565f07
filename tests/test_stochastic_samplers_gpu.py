"""-m gpu: the stochastic samplers through the HIP path -- DDIM with eta / "euler_a", SDE-DPM-Solver++(2M), LCM.

Bars (the project's existing ones):
  * kernels fed identical fp32 inputs and the same noise: BIT-EXACT against the specification's torch-CPU op sequence
    (tests/stochastic_cpu.py);
  * the fused epilogue with ``noise``: bit-identical to the chain of separate kernels with ``noise``;
  * end to end against the G18 fixture (the real reference's latents for the stateless steps) and ``StochasticOracle``: latent
    rel-L2 < 1e-4, host RNG stream in exactly the same end state; interleaved against alone 1e-5;
  * the toy-problem inequalities of tests/test_stochastic_samplers.py again, through the kernel loop, bit-equal to the restatement;
  * without the new keywords the loop launches exactly the entry points it launched before and gives the same bits.
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import dpm_solver_cpu as D
from tests import stochastic_cpu as S
from tests.ddim_variants import embed_fn
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE, synthetic_text_embeds
from tests.glue_geometries import FUSED_ROWS, misaligned
from tests.golden import cases
from tests.test_hip_parity import DEV, dev_i32, rel_l2

pytestmark = pytest.mark.gpu

NEW_ENTRY_POINTS = ("ed_cfg_ddim_step_sde", "ed_phase_epilogue_sde")
V_PRED = dict(prediction_type="v_prediction")
V_TRAILING_ZSNR = dict(prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True)
SAMPLER_KW = dict(S.STATELESS, eta03=dict(sampler="ddim", eta=0.3), euler_a=dict(sampler="euler_a"),
                  sde2=dict(sampler="dpmsolver++sde", solver_order=2))


def _mods():
    from elasticdiffusion_official_amd import geometry, ops, schedule
    return geometry, ops, schedule


def _schedules(key, kw, steps):
    """-> (the product's scheduler, the restatement's, the timesteps) of SAMPLER_KW[key] under the scheduler settings ``kw``"""
    from elasticdiffusion_official_amd.pipeline import make_scheduler
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    skw = SAMPLER_KW[key]
    prod = make_scheduler(DDIMSchedule(**kw), skw["sampler"], skw.get("solver_order", 2), skw.get("eta", 0.0))
    spec = S.StochasticCPU(**skw, **kw)
    ts = prod.set_timesteps(steps)
    spec.set_timesteps(steps)
    assert torch.equal(ts, spec.timesteps)
    return prod, spec, ts


def _step_args(prod, t, t_hist, is_last, hist):
    """-> (the four positional scalars, the keywords) of ops.cfg_ddim_step / the ``coef`` and keywords of ops.phase_epilogue"""
    from elasticdiffusion_official_amd.schedule import DPMSolverSchedule
    if isinstance(prod, DPMSolverSchedule):
        coef = prod.multistep_coefficients(t, t_hist, is_last)
        return coef[:2] + (0.0, 0.0), dict(multistep=coef[2:] + (hist if coef[5] != 0.0 else None,))
    return prod.step_coefficients(t), {}


# ---------------------------------------------------------------------------------------------------
# the flat step, bit-exact
# ---------------------------------------------------------------------------------------------------
# (sampler, scheduler settings, steps, timestep index, with a history): both forms, both prediction types, mid-schedule and the last
# step, the abar_t = 0 timestep of zero-SNR betas and the one after it (first order forced), LCM's last step (c_n = 0)
FLAT_CASES = [("eta1", {}, 20, 7, False), ("eta1", V_PRED, 20, 7, False), ("eta03", {}, 20, 19, False), ("eta1", V_TRAILING_ZSNR, 5, 0, False),
              ("sde2", {}, 20, 7, True), ("sde2", {}, 20, 7, False), ("sde2", V_PRED, 20, 19, True), ("sde2", V_TRAILING_ZSNR, 5, 0, False),
              ("sde2", V_TRAILING_ZSNR, 5, 1, True), ("sde2", V_TRAILING_ZSNR, 5, 2, True), ("lcm", {}, 4, 1, True), ("lcm", V_PRED, 4, 3, False)]


def _flat_case(key, kw, steps, ti, n, with_hist, with_ratio, B=1):
    prod, spec, ts = _schedules(key, kw, steps)
    g = torch.Generator().manual_seed(steps * 1000 + ti * 10 + n % 7)
    local, direction, x, x0h, noise = (torch.randn(n, generator=g) for _ in range(5))
    guidance = 10.0 / 3
    t = ts[ti]
    t_hist = ts[ti - 1] if with_hist and ti > 0 else None
    m = local + guidance * direction
    ratio = None
    if with_ratio:
        from tests.guidance_rescale_cpu import rescale_with_ratio
        ratio = torch.tensor([0.8, 1.1, 0.95, 1.3][:B])
        m = rescale_with_ratio(m.view(B, -1), ratio, 0.7).view(-1)
    want = spec.step(m, t, x, history=None if t_hist is None else (x0h, t_hist), is_last=ti == steps - 1, noise=noise)
    c_n = prod.noise_coefficient(t)
    assert c_n == float(spec.noise_coefficient(t))
    return prod, (t, t_hist, ti == steps - 1), (local, direction, x), x0h, noise, c_n, guidance, ratio, want


@pytest.mark.parametrize("with_ratio", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1028, 4 * 1025])
@pytest.mark.parametrize("key,kw,steps,ti,with_hist", FLAT_CASES)
def test_cfg_ddim_step_noise_bit_exact(key, kw, steps, ti, with_hist, n, with_ratio):
    _, ops, _ = _mods()
    B = 2 if with_ratio and n == 4 * 1025 else 1      # two samples of 2050 elements: no whole number of float4s, the scalar form
    prod, at, ins, x0h, noise, c_n, guidance, ratio, want = _flat_case(key, kw, steps, ti, n, with_hist, with_ratio, B)
    if kw.get("rescale_betas_zero_snr") and ti == 0:
        assert float(prod.alphas_cumprod[int(prod.timesteps[0])]) == 0.0
    kws = dict(prediction_type=kw.get("prediction_type", "epsilon"))
    if ratio is not None:
        kws.update(ratio=ratio.to(DEV), guidance_rescale=0.7)
    dev_ins = [t.to(DEV) for t in ins]
    scalars, ms_kw = _step_args(prod, *at, x0h.to(DEV))
    hist = ms_kw["multistep"][4] if ms_kw else None
    nz = noise.to(DEV)
    if c_n == 0.0:      # LCM's last step: not stochastic.  The noise is NOT READ -- a buffer of inf leaves the result the restatement's
        assert key == "lcm" and ti == steps - 1
        nz = torch.full((n,), float("inf"), device=DEV)
    prev, x0 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *scalars, noise=(c_n, nz), **ms_kw, **kws)
    assert bool(torch.isfinite(prev).all())
    assert torch.equal(x0.cpu(), want["pred_original_sample"])
    assert torch.equal(prev.cpu(), want["prev_sample"])
    # the scalar path: every operand in turn (the history and the noise among them) 4 bytes off a 16-byte boundary gives the same bits
    for k in range(7):
        args = dev_ins + [torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV), hist, nz]
        if args[k] is None:
            continue
        args[k] = misaligned(args[k])
        kw_k = dict(multistep=ms_kw["multistep"][:4] + (args[5],)) if ms_kw else {}
        ops.cfg_ddim_step(*args[:5], np.float32(guidance), *scalars, noise=(c_n, args[6]), **kw_k, **kws)
        assert torch.equal(args[3], prev) and torch.equal(args[4], x0), k


def test_zero_noise_coefficient_runs_the_deterministic_kernels_and_reads_no_noise():
    """c_n == 0 is not a stochastic step: with inf in ``noise`` the outputs are the deterministic launch's, bit for bit (the tensor is
    not read); a non-zero c_n with the same buffer does read it"""
    _, ops, _ = _mods()
    for key in ("eta1", "sde2"):
        prod, at, ins, x0h, noise, c_n, guidance, _, _ = _flat_case(key, {}, 20, 7, 1028, True, False)
        dev_ins = [t.to(DEV) for t in ins]
        scalars, ms_kw = _step_args(prod, *at, x0h.to(DEV))
        inf = torch.full((1028,), float("inf"), device=DEV)
        out = {}
        for label, kw in (("plain", {}), ("zero", dict(noise=(0.0, inf))), ("read", dict(noise=(c_n, inf)))):
            prev, x0 = torch.empty(1028, device=DEV), torch.empty(1028, device=DEV)
            ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *scalars, **ms_kw, **kw)
            out[label] = (prev, x0)
        assert torch.equal(out["zero"][0], out["plain"][0]) and torch.equal(out["zero"][1], out["plain"][1])
        assert bool(torch.isfinite(out["zero"][0]).all()) and bool(torch.isinf(out["read"][0]).all())
        assert torch.equal(out["read"][1], out["plain"][1])          # one x0 whatever the sample update


def test_cfg_ddim_step_noise_argument_errors():
    _, ops, _ = _mods()
    prod, at, ins, x0h, noise, c_n, guidance, _, _ = _flat_case("sde2", {}, 20, 7, 1028, True, False)
    dev_ins = [t.to(DEV) for t in ins]
    scalars, ms_kw = _step_args(prod, *at, x0h.to(DEV))
    nz = noise.to(DEV)
    prev, x0 = torch.full((1028,), 3.0, device=DEV), torch.full((1028,), 3.0, device=DEV)

    def call(noise, prev=prev, x0=x0, **kw):
        ops.cfg_ddim_step(*dev_ins, prev, x0, np.float32(guidance), *scalars, noise=noise, **dict(ms_kw, **kw))

    with pytest.raises(RuntimeError, match="overlaps an output"):      # in place
        call((c_n, x0))
    with pytest.raises(RuntimeError, match="overlaps an output"):
        call((c_n, prev))
    buf = torch.zeros(2 * 1028, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps an output"):      # a partial overlap
        call((c_n, buf[514:514 + 1028]), prev=buf[:1028])
    with pytest.raises(RuntimeError, match="noise must be"):
        call(nz)
    with pytest.raises(RuntimeError, match="noise must be"):
        call((c_n, None))
    with pytest.raises(RuntimeError, match="noise must be"):
        call((c_n, nz[:100]))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="finite"):
            call((bad, nz))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call((c_n, noise))
    with pytest.raises(RuntimeError, match="prediction_type"):
        call((c_n, nz), prediction_type="sample")
    assert float(prev.min()) == 3.0 and float(x0.min()) == 3.0     # nothing was launched
    assert ops._LAUNCH["device"] is None
    # the library refuses the same on its own (hipErrorInvalidValue = 1, before any launch)
    from elasticdiffusion_official_amd import _hip
    L = _hip.lib()
    p = [t.data_ptr() for t in dev_ins] + [prev.data_ptr(), x0.data_ptr()]
    st = torch.cuda.current_stream(DEV).cuda_stream
    coef = prod.multistep_coefficients(*at)

    def lib(form, c, noise_ptr, hist=None, pt=0):
        return L.ed_cfg_ddim_step_sde(*p, 1.0, *coef, 1028, pt, None, 0.0, 0.0, 0, hist, form, c, noise_ptr, st)

    assert lib(1, c_n, None) == 1                                   # a null noise
    assert lib(1, float("nan"), nz.data_ptr()) == 1 and lib(1, float("inf"), nz.data_ptr()) == 1
    assert lib(2, c_n, nz.data_ptr()) == 1 and lib(-1, c_n, nz.data_ptr()) == 1     # a bad form
    assert lib(1, c_n, nz.data_ptr(), pt=7) == 1                    # a bad prediction_type
    assert lib(0, c_n, nz.data_ptr(), hist=x0h.to(DEV).data_ptr()) == 1             # the DDIM form takes no history
    assert lib(1, c_n, x0.data_ptr()) == 1 and lib(1, c_n, prev.data_ptr() + 4) == 1    # a noise that shares an element with an output
    assert lib(0, 0.0, x0.data_ptr()) == 1                          # ... refused whatever c_n is
    torch.cuda.synchronize()
    assert float(prev.min()) == 3.0 and float(x0.min()) == 3.0
    assert lib(1, c_n, nz.data_ptr()) == 0                          # and the launch state is clean: the next call runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(prev).all()) and float(prev.min()) != 3.0


# ---------------------------------------------------------------------------------------------------
# the fused epilogue with noise == the chain of separate kernels with noise, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hl,Wl,h,w,d,patch", FUSED_ROWS)
@pytest.mark.parametrize("B,K,dtype", [(1, 4, torch.float32), (2, 1, torch.bfloat16), (1, 8, torch.float16)])
@pytest.mark.parametrize("key,kw,with_hist,rescale", [("eta1", {}, False, False), ("sde2", {}, True, False), ("sde2", {}, False, False),
                                                      ("sde2", V_PRED, True, True), ("eta1", V_PRED, False, True), ("lcm", {}, False, False)])
def test_fused_epilogue_noise_equals_separate_kernels(Hl, Wl, h, w, d, patch, B, K, dtype, key, kw, with_hist, rescale):
    geometry, ops, _ = _mods()
    from elasticdiffusion_official_amd import host_rng
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    gpad, vpad = geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)
    g = torch.Generator().manual_seed(Hl * 131 + Wl + K)
    x = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    x0h = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
    nz = torch.randn(B, 4, Hl, Wl, generator=g).to(DEV)
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
    prod, _, ts = _schedules(key, kw, 20)
    coef, ms_kw = _step_args(prod, ts[7], ts[6] if with_hist else None, False, x0h)
    assert (ms_kw.get("multistep", (None,) * 5)[4] is not None) == with_hist
    c_n = prod.noise_coefficient(ts[7])
    assert c_n != 0.0
    nz_kw = dict(noise=(c_n, nz))
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
    ops.cfg_ddim_step(local1, direction1, x, prev1, x01, guidance, *coef, **ms_kw, **nz_kw, **pt_kw, **flat_rs)
    ops.rrg_update(prev1, x01, low[K - 1], unc1, ldir1, T["up_row"], T["up_col"], nxt1, guidance, coef[0], coef[1], norm,
                   w_rrg, **pt_kw, **rrg_rs)
    assert bool(torch.isfinite(nxt1).all())
    # with x_next (fused RRG: formed from the prev that carries the noise) and every by-product
    out = {k: torch.full_like(x, 5.0) for k in ("prev", "x0", "x_next", "direction", "local")}
    unc2, ldir2 = torch.full_like(unc1, 5.0), torch.full_like(ldir1, 5.0)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, out["prev"], out["x0"], low_dir=ldir2, uncond_last=unc2, direction=out["direction"],
                       local=out["local"], x_next=out["x_next"], low_latent=low[K - 1], rrg_norm=norm, rrg_weight=w_rrg,
                       **ms_kw, **nz_kw, **pt_kw, **epi_rs)
    for name, want in (("prev", prev1), ("x0", x01), ("x_next", nxt1), ("direction", direction1), ("local", local1)):
        assert torch.equal(out[name], want), name
    assert torch.equal(unc2, unc1) and torch.equal(ldir2, ldir1)
    # without x_next and without the optional outputs
    p3, z3 = torch.empty_like(x), torch.empty_like(x)
    no_low = {k: v for k, v in epi_rs.items() if k != "ratio_low"}
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, p3, z3, **ms_kw, **nz_kw, **pt_kw, **no_low)
    assert torch.equal(p3, prev1) and torch.equal(z3, x01)
    # the noise launch is not the deterministic launch: one x0, another prev; at c_n = 0 it IS the deterministic launch (noise unread)
    p4, z4, p5, z5 = (torch.empty_like(x) for _ in range(4))
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, p4, z4, **ms_kw, **pt_kw, **no_low)
    ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                       coef, p5, z5, noise=(0.0, torch.full_like(x, float("inf"))), **ms_kw, **pt_kw, **no_low)
    assert torch.equal(z4, z3) and rel_l2(p4, p3) > 1e-3
    assert torch.equal(p5, p4) and torch.equal(z5, z4)
    # refused before any launch: a noise in place, on an optional output, of another shape; a non-finite coefficient
    keep = p4.clone()
    with pytest.raises(RuntimeError, match="overlaps an output"):
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                           coef, p4, z4, noise=(c_n, z4), **ms_kw, **pt_kw, **no_low)
    with pytest.raises(RuntimeError, match="overlaps an output"):
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                           coef, p4, z4, x_next=nz, low_latent=low[K - 1], noise=(c_n, nz), **ms_kw, **pt_kw, **epi_rs)
    with pytest.raises(RuntimeError, match="finite"):
        ops.phase_epilogue(g_out, v_out, x, stamp, pick, cover, vp.n_col_blocks, (gpad.top, gpad.left), K, h, w, guidance,
                           coef, p4, z4, noise=(float("nan"), nz), **ms_kw, **pt_kw, **no_low)
    assert torch.equal(p4, keep) and ops._LAUNCH["device"] is None


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _pipe(name, key, text_encoder=None, **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = D.SOLVER_CASES[name]
    if c.get("controlnet"):
        extra["controlnet"] = FakeControlNet()
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=D.VBS, unet=FakeUNet(c["sample"]), vae=FakeVAE(),
                            text_encoder=text_encoder or embed_fn(False), scheduler=_schedules(key, c["sched"], c["steps"])[0], **extra)


@pytest.mark.parametrize("key", ["eta1", "sde1", "lcm", "sde2"])
@pytest.mark.parametrize("name", list(D.SOLVER_CASES))
def test_end_to_end_vs_fixture(golden_dir, name, key):
    """the eta1 / sde1 / lcm rows of G18 are the REAL reference's latents with the stateless step injected; sde2 is StochasticOracle's"""
    from elasticdiffusion_official_amd import ops
    g = np.load(os.path.join(golden_dir, "g18_stochastic.npz"))
    pipe = _pipe(name, key)
    pipe.seed_everything(D.SEED)
    ops.TIMER.start()
    try:
        z = pipe.generate_latents("p", "", **D.case_kwargs(name), **D.condition_kwargs(name)).cpu()
        tail = torch.rand(4)
    finally:
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    want = torch.from_numpy(g[f"{name}/{key}/latent"])
    err = rel_l2(z, want)
    print(f"{name} {key}: rel-L2 vs G18 {err:.3e}")
    assert z.shape == want.shape and err < 1e-4, err
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/{key}/rng_tail"])
    c = D.SOLVER_CASES[name]
    repaint = D.case_kwargs(name)["repaint_sampling"]
    phases = 2 * c["steps"] - 1 if repaint else c["steps"]
    quiet = 1 if key == "lcm" else 0      # LCM's last timestep (one phase) is not stochastic: the deterministic entry point
    assert counts["ed_phase_epilogue_sde"] == phases - quiet and "ed_phase_epilogue" not in counts, counts
    assert counts.get("ed_phase_epilogue_ms", 0) == quiet, counts


@pytest.mark.parametrize("key", ["eta1", "sde1", "lcm", "sde2"])
def test_end_to_end_with_separate_glue_kernels(golden_dir, key):
    """FUSED_GLUE off: ed_cfg_ddim_step_sde carries the loop; same bar, and bit-identical to the fused path"""
    from elasticdiffusion_official_amd import ops, pipeline
    name = "eps_leading_repaint"
    g = np.load(os.path.join(golden_dir, "g18_stochastic.npz"))
    lat, tails, counts = {}, {}, {}
    for fused in (False, True):
        pipeline.FUSED_GLUE = fused
        ops.TIMER.start()
        try:
            pipe = _pipe(name, key)
            pipe.seed_everything(D.SEED)
            lat[fused] = pipe.generate_latents("p", "", **D.case_kwargs(name)).cpu()
            tails[fused] = torch.rand(4)
        finally:
            pipeline.FUSED_GLUE = True
            counts[fused] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert rel_l2(lat[False], torch.from_numpy(g[f"{name}/{key}/latent"])) < 1e-4
    np.testing.assert_array_equal(tails[False].numpy(), g[f"{name}/{key}/rng_tail"])
    assert torch.equal(lat[False], lat[True]) and torch.equal(tails[False], tails[True])
    phases = 2 * D.SOLVER_CASES[name]["steps"] - 1
    assert counts[False]["ed_cfg_ddim_step_sde"] == phases - (1 if key == "lcm" else 0) and "ed_phase_epilogue_sde" not in counts[False]


def _picture(H, W, seed=5):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H // 8, W // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 255
    return img, mask


def test_img2img_with_mask_under_euler_a_keeps_the_init_latent():
    from tests.img2img_cpu import latent_mask
    name = "eps_leading_repaint"
    c = D.SOLVER_CASES[name]
    img, mask = _picture(c["H"], c["W"])
    want, otail = S.run_oracle_case(name, dict(sampler="euler_a"), init_image=img, strength=0.75, mask_image=mask)
    pipe = _pipe(name, "euler_a")
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs(name), init_image=img, strength=0.75, mask_image=mask).cpu()
    tail = torch.rand(4)
    keep = (latent_mask(mask, 8) == 0).expand_as(z)
    assert bool(keep.any()) and not bool(keep.all())
    assert torch.equal(z[keep], pipe.last_init_latents.cpu()[keep])
    print(f"img2img + mask under euler_a, strength 0.75: rel-L2 {rel_l2(z, want):.3e}")
    assert rel_l2(z, want) < 1e-4 and torch.equal(tail, otail)


def test_guidance_rescale_with_v_prediction_under_sde():
    name = "v_trailing"
    kw = dict(sampler="dpmsolver++sde", solver_order=2)
    want, otail = S.run_oracle_case(name, kw, guidance_rescale=0.7)
    pipe = _pipe(name, "sde2")
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs(name), guidance_rescale=0.7).cpu()
    tail = torch.rand(4)
    print(f"guidance_rescale 0.7, v / trailing, 2M SDE: rel-L2 {rel_l2(z, want):.3e}")
    assert bool(torch.isfinite(z).all()) and rel_l2(z, want) < 1e-4 and torch.equal(tail, otail)


def test_interleaved_two_jobs_equal_each_alone(golden_dir):
    """the noise is drawn from each job's own RNG stream: two images in flight do not consume each other's draws"""
    name = "eps_leading_repaint"
    g = np.load(os.path.join(golden_dir, "g18_stochastic.npz"))
    kw = D.case_kwargs(name)
    seeds = [D.SEED, 11, 12]

    def embed(prompts):  # stateless (the programs' calls interleave); the values embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe(name, "sde2", text_encoder=embed)
    alone = []
    for s in seeds:
        pipe.seed_everything(s)
        alone.append(pipe.generate_latents("p", "", **kw).clone())
    got = pipe.generate_latents_interleaved([dict(prompts="p", negative_prompts="", seed=s) for s in seeds], in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], torch.from_numpy(g[f"{name}/sde2/latent"])) < 1e-4
    assert rel_l2(got[0], got[1]) > 1e-2


def test_sampler_keywords_build_the_schedule_and_regions_are_refused():
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule, DPMSolverSchedule, LCMSchedule
    kw = dict(view_batch_size=D.VBS, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=embed_fn(False))
    pipe = ElasticDiffusion(DEV, "1.5", sampler="euler_a", **kw)
    assert type(pipe.scheduler) is DDIMSchedule and pipe.scheduler.eta == 1.0
    assert ElasticDiffusion(DEV, "1.5", eta=0.25, **kw).scheduler.eta == 0.25
    sde = ElasticDiffusion(DEV, "1.5", sampler="dpmsolver++sde", solver_order=1, **kw).scheduler
    assert type(sde) is DPMSolverSchedule and sde.algorithm_type == "sde-dpmsolver++" and sde.solver_order == 1
    assert type(ElasticDiffusion(DEV, "1.5", sampler="lcm", **kw).scheduler) is LCMSchedule
    assert ElasticDiffusion(DEV, "1.5", **kw).scheduler.eta == 0.0
    with pytest.raises(ValueError, match="eta"):
        ElasticDiffusion(DEV, "1.5", eta=1.5, **kw)
    with pytest.raises(ValueError, match="eta"):
        ElasticDiffusion(DEV, "1.5", sampler="lcm", eta=0.5, **kw)
    # regions + a stochastic sampler: ValueError before anything launches
    from elasticdiffusion_official_amd import ops
    ops.TIMER.start()
    try:
        with pytest.raises(ValueError, match="stochastic"):
            pipe.generate_latents("p", "", height=256, width=512, num_inference_steps=2, resampling_steps=1,
                                  regions=[("a red door", (0, 0, 256, 256))])
        with pytest.raises(ValueError, match="stochastic"):
            pipe.generate_latents_interleaved([dict(prompts="p", seed=1, regions=[("a red door", (0, 0, 256, 256))])], height=256,
                                              width=512, num_inference_steps=2, resampling_steps=1)
    finally:
        assert ops.TIMER.stop() == {}
    with pytest.raises(RuntimeError, match="no noise variant"):
        x = torch.zeros(1, 4, 8, 8, device=DEV)
        ops.phase_epilogue(torch.zeros(2, 4, 8, 8, device=DEV), torch.zeros(1, 4, 8, 8, device=DEV), x, torch.zeros(64, 4, dtype=torch.int8, device=DEV),
                           tuple(torch.zeros(n, dtype=torch.int32, device=DEV) for n in (16, 16, 8, 8, 8, 8)),
                           tuple(torch.zeros(16, dtype=torch.int32, device=DEV) for _ in range(4)), 1, (0, 0), 1, 8, 8, 1.0,
                           (0.5, 0.5, 0.5, 0.5), torch.empty_like(x), torch.empty_like(x), region_w=torch.ones(1, 8, 8, device=DEV),
                           noise=(0.5, torch.zeros_like(x)))
    assert ops._LAUNCH["device"] is None


@pytest.mark.parametrize("key", ["eta1", "sde2", "lcm"])
def test_generate_vs_oracle(key):
    """``generate()``, the plain CFG loop: one draw per stochastic step where the reference calls scheduler.step (ED:776)"""
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.G11_CASES["gen_sd_pad_32x64"]
    (un, pun), (co, pco) = synthetic_text_embeds(1)
    text, pooled = torch.cat([un, co]), torch.cat([pun, pco])
    size = (4 * 8 * c["h"], 4 * 8 * c["w"])
    prod, spec, _ = _schedules(key, {}, c["steps"])
    pipe = ElasticDiffusion(DEV, c["sd"], log_freq=1, unet=FakeUNet(c["sample"]), vae=FakeVAE(), scheduler=prod)
    pipe.default_size = size
    pipe.seed_everything(c["seed"])
    z = torch.randn(1, 4, c["h"], c["w"])
    seen = {}
    dec = pipe.decode_latents
    pipe.decode_latents = lambda lat: (seen.__setitem__("z", lat.clone()), dec(lat))[1]
    _, info = pipe.generate(z, text, pooled, guidance_scale=c["guidance"])
    tail = torch.rand(4)
    orc = S.StochasticOracle(FakeUNet(c["sample"]), FakeVAE(), spec, sd_version=c["sd"])
    orc.default_size = size
    orc.seed_everything(c["seed"])
    latent, inter = orc.plain_cfg_generate(torch.randn(1, 4, c["h"], c["w"]), text, pooled, c["guidance"])
    otail = torch.rand(4)
    assert rel_l2(seen["z"], latent) < 1e-4, rel_l2(seen["z"], latent)
    assert rel_l2(torch.cat(info["inter_x0"]), torch.cat(inter)) < 1e-4
    assert torch.equal(tail, otail)


# ---------------------------------------------------------------------------------------------------
# the toy problem through the kernel loop: bit-equal to the restatement on the same noise
# ---------------------------------------------------------------------------------------------------
_TOY = {}


def _device_toy(name, steps):
    """-> (std error of the device chain's end latent, is it bit-equal to the restatement's?)  Computed once per process."""
    if (name, steps) in _TOY:
        return _TOY[name, steps]
    _, ops, _ = _mods()
    record = []
    spec, want = S.toy_chain(name, steps, record)
    prod, _, ts = _schedules(name, {}, steps)
    x = S.gauss_start(spec, S.TOY_N, S.TOY_SEED).to(DEV)
    zero = torch.zeros_like(x)
    predictor = S.gauss_predictor(spec)
    hist = None
    for (t, t_hist, is_last, noise) in record:
        local = predictor(x, t)                           # ONE product per element with a host scalar: the CPU's bits
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        scalars, ms_kw = _step_args(prod, t, t_hist, is_last, hist)
        ops.cfg_ddim_step(local, zero, x, prev, x0, np.float32(7.5), *scalars, noise=(prod.noise_coefficient(t), noise.to(DEV)), **ms_kw)
        hist, x = x0, prev
    got = x.cpu()
    _TOY[name, steps] = (S.gauss_std_error(spec, got), torch.equal(got, want))
    return _TOY[name, steps]


@pytest.mark.parametrize("steps", [20, 25, 50, 100])
@pytest.mark.parametrize("name", list(S.TOY_SAMPLERS))
def test_toy_problem_on_the_device_is_bit_equal_to_the_restatement(name, steps):
    err, equal = _device_toy(name, steps)
    print(f"toy problem on the device, {name}, {steps} steps: std error {err:.3e}")
    assert equal


def test_toy_problem_on_the_device_meets_the_cpu_assertions():
    err = {(name, k): _device_toy(name, k)[0] for name in S.TOY_SAMPLERS for k in (20, 25, 50, 100)}
    for k in (20, 25, 50):
        assert err["sde2", k] <= 0.75 * err["sde1", k], (k, err["sde2", k], err["sde1", k])
    for k in (20, 25, 50, 100):
        assert abs(err["eta1", k] - err["sde1", k]) <= 3e-3, (k, err["eta1", k], err["sde1", k])
    for name in S.TOY_SAMPLERS:
        assert err[name, 20] > err[name, 50] > err[name, 100], name


# ---------------------------------------------------------------------------------------------------
# opt-in: without the new keywords the loop is the loop as it was
# ---------------------------------------------------------------------------------------------------
def test_absent_keywords_launch_what_was_always_launched(golden_dir):
    from elasticdiffusion_official_amd import ElasticDiffusion, ops
    name = "cfg2_sd_512x1024"
    c = cases.E2E_CASES[name]
    g = np.load(os.path.join(golden_dir, "g8_end_to_end.npz"))
    g16 = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)
    lat, counts, tails = {}, {}, {}
    for label, extra in (("omitted", {}), ("eta0", dict(sampler="ddim", eta=0.0)), ("dpm", dict(sampler="dpmsolver++")),
                         ("euler_a", dict(sampler="euler_a"))):
        pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"]), vae=FakeVAE(),
                                text_encoder=embed_fn(False), **extra)
        pipe.seed_everything(c["seed"])
        ops.TIMER.start()
        try:
            lat[label] = pipe.generate_latents("p", "", **kw).cpu()
            tails[label] = torch.rand(4)
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert torch.equal(lat["omitted"], lat["eta0"]) and counts["omitted"] == counts["eta0"] and torch.equal(tails["omitted"], tails["eta0"])
    phases = 2 * c["steps"] - 1
    glue = {k: v for k, v in counts["eta0"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k or "ddim" in k}
    assert glue == {"ed_assemble_rows": phases, "ed_phase_epilogue": phases, "ed_undo_step": c["steps"] - 1}, counts["eta0"]
    assert rel_l2(lat["eta0"], torch.from_numpy(g[f"{name}/latent"])) < 1e-4
    # the deterministic multistep sampler still launches its own entry point and no other
    swapped = {("ed_phase_epilogue_ms" if k == "ed_phase_epilogue" else k): v for k, v in counts["eta0"].items()}
    assert counts["dpm"] == swapped
    for label in ("omitted", "eta0", "dpm"):
        assert not any(k in counts[label] for k in NEW_ENTRY_POINTS), label
    # a stochastic sampler: the same number of launches, one entry point exchanged
    swapped = {("ed_phase_epilogue_sde" if k == "ed_phase_epilogue" else k): v for k, v in counts["eta0"].items()}
    assert counts["euler_a"] == swapped and rel_l2(lat["euler_a"], lat["eta0"]) > 1e-3
    # and the existing DPM golden on its own geometry
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=D.VBS, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=embed_fn(False),
                            sampler="dpmsolver++")
    pipe.seed_everything(D.SEED)
    z = pipe.generate_latents("p", "", **D.case_kwargs("eps_norepaint")).cpu()
    assert rel_l2(z, torch.from_numpy(g16["eps_norepaint/order2/latent"])) < 1e-4
    np.testing.assert_array_equal(torch.rand(4).numpy(), g16["eps_norepaint/order2/rng_tail"])


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_sampler_flags(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    base = ["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "3", "--resampling_steps", "1", "--outdir",
            str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4"]
    runs = {"default": [], "eta": ["--eta", "1.0"], "sde": ["--sampler", "dpmsolver++sde"],
            "lcm_v": ["--sampler", "lcm", "--prediction_type", "v_prediction"]}
    dirs = {k: main(base + ["--exp", k] + v) for k, v in runs.items()}
    img = {k: np.asarray(Image.open(os.path.join(d, "0.png")), dtype=np.float32) for k, d in dirs.items()}
    for k, a in img.items():
        assert a.shape == (512, 512, 3) and np.isfinite(a).all() and a.std() > 0, k  # a NaN latent decodes to a constant image
    # (the command line builds randomly initialised models before it seeds, so no two runs share weights: that "euler_a" IS eta = 1
    # is asserted on the schedules, tests/test_stochastic_samplers.py::test_euler_a_is_eta_one)
    assert not np.array_equal(img["default"], img["eta"]) and not np.array_equal(img["eta"], img["sde"])
    assert not np.array_equal(img["sde"], img["lcm_v"])
    args = open(os.path.join(dirs["sde"], "args.txt")).read()
    assert "sampler: dpmsolver++sde" in args and "eta: 0.0" in args
    assert "eta: 1.0" in open(os.path.join(dirs["eta"], "args.txt")).read()
    assert glob.glob(os.path.join(dirs["lcm_v"], "*.png"))
    with pytest.raises(ValueError, match="eta"):
        main(base + ["--exp", "bad", "--sampler", "lcm", "--eta", "0.5"])
