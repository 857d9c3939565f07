"""CPU: DPM-Solver++(2M) -- the product's host scalars against the written-out specification
(tests/dpm_solver_cpu.py), the specification against the DDIM restatement and against an ODE with a known solution, and the
first-order cases against the real reference where its checkout exists."""
import math
import os

import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle
from tests import dpm_solver_cpu as D
from tests.golden.ref_loader import reference_available

SPACINGS = ("leading", "linspace", "trailing")


def _pair(k, order, **kw):
    from elasticdiffusion_official_amd.schedule import DPMSolverSchedule
    prod, spec = DPMSolverSchedule(solver_order=order, **kw), D.DPMSolverCPU(solver_order=order, **kw)
    ts = prod.set_timesteps(k)
    spec.set_timesteps(k)
    assert torch.equal(ts, spec.timesteps)
    return prod, spec, ts


# ---- host scalars == the restatement's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("zsnr", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("k", [4, 7, 14, 15, 20, 50])
def test_coefficients_equal_the_restatement(k, spacing, zsnr, order):
    prod, spec, ts = _pair(k, order, timestep_spacing=spacing, rescale_betas_zero_snr=zsnr, prediction_type="v_prediction")
    t_hist, n_second = None, 0
    for i, t in enumerate(ts):
        got = prod.multistep_coefficients(t, t_hist, i == k - 1)
        want = tuple(float(v) for v in spec.coefficients(t, t_hist, i == k - 1))
        assert got == want, (i, got, want)
        assert all(isinstance(v, float) and math.isfinite(v) for v in got), (i, got)
        assert got == tuple(float(np.float32(v)) for v in got)          # python floats holding fp32 values
        assert got[:2] == prod.step_coefficients(t)[:2]
        second = spec.second_order(t, t_hist, i == k - 1)
        if got[5] != 0.0:
            assert second
        elif second:    # linspace ends at t = 0, whose abar_prev is abar_t: h = 0, the step is the identity at either order
            assert spacing == "linspace" and i == k - 1 and got[2:5] == (1.0, 0.0, 0.0)
        n_second += got[5] != 0.0
        t_hist = t
    if order == 1:
        assert n_second == 0
    else:
        # first order: the first step, the last of a short run (or of a linspace grid: h = 0), the one after abar = 0
        forced = 1 + (k < 15 or spacing == "linspace") + (zsnr and float(spec.alphas_cumprod[int(ts[0])]) == 0.0)
        assert n_second == k - forced, (n_second, forced)


def test_forced_first_order_cases():
    # no history / solver_order 1
    prod, spec, ts = _pair(20, 2)
    assert prod.multistep_coefficients(ts[0], None, False)[5] == 0.0
    assert prod.multistep_coefficients(ts[1], ts[0], False)[5] != 0.0
    assert _pair(20, 1)[0].multistep_coefficients(ts[1], ts[0], False)[5] == 0.0
    # the last step of a short run, and lower_order_final switched off
    from elasticdiffusion_official_amd.schedule import DPMSolverSchedule
    for k, first in ((14, True), (15, False)):
        prod, spec, ts = _pair(k, 2)
        assert (prod.multistep_coefficients(ts[-1], ts[-2], True)[5] == 0.0) is first
        assert prod.multistep_coefficients(ts[-1], ts[-2], False)[5] != 0.0
    keep = DPMSolverSchedule(lower_order_final=False)
    keep.set_timesteps(4)
    assert keep.multistep_coefficients(keep.timesteps[-1], keep.timesteps[-2], True)[5] != 0.0
    # abar_prev == 1 (set_alpha_to_one): h is infinite, prev = x0 exactly
    prod, spec, ts = _pair(20, 2, set_alpha_to_one=True)
    c = prod.multistep_coefficients(ts[-1], ts[-2], True)
    assert c[2:] == (0.0, -1.0, -0.5, 0.0)
    # abar_{t_hist} == 0 (zero-SNR first timestep): h0 is infinite
    prod, spec, ts = _pair(5, 2, timestep_spacing="trailing", rescale_betas_zero_snr=True, prediction_type="v_prediction")
    assert float(prod.alphas_cumprod[int(ts[0])]) == 0.0
    assert prod.multistep_coefficients(ts[1], ts[0], False)[5] == 0.0
    assert prod.multistep_coefficients(ts[2], ts[1], False)[5] != 0.0


@pytest.mark.parametrize("k", [4, 20])
@pytest.mark.parametrize("kw", [dict(set_alpha_to_one=True), dict(set_alpha_to_one=True, timestep_spacing="trailing",
                                                                   rescale_betas_zero_snr=True, prediction_type="v_prediction")])
def test_set_alpha_to_one_stays_finite_to_the_end(k, kw):
    sched = D.DPMSolverCPU(**kw)
    sched.set_timesteps(k)
    g = torch.Generator().manual_seed(k)
    x = torch.randn(2, 4, 8, 8, generator=g)
    last = {}

    def model(x_, t):
        return 0.3 * x_ + 0.1 * torch.randn(x_.shape, generator=g)

    hist = None
    for t in sched.timesteps:
        out = sched.step(model(x, t), t, x, history=hist)
        hist, x, last = (out["pred_original_sample"], t), out["prev_sample"], out
    assert bool(torch.isfinite(x).all())
    assert torch.equal(x, last["pred_original_sample"])          # abar_prev = 1: the last step returns x0


# ---- order 1 is DDIM (the known identity) --------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_order_one_equals_ddim_in_fp64(prediction_type):
    spec, ddim = D.DPMSolverCPU(solver_order=1, prediction_type=prediction_type), DDIMOracle(prediction_type=prediction_type)
    for s in (spec, ddim):
        s.alphas_cumprod, s.final_alpha_cumprod = s.alphas_cumprod.double(), s.final_alpha_cumprod.double()
        s.set_timesteps(5)
    g = torch.Generator().manual_seed(1)
    x = y = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    for t in spec.timesteps:
        m = torch.randn(x.shape, generator=g, dtype=torch.float64)
        a, b = spec.step(m, t, x), ddim.step(m, t, y)
        x, y = a["prev_sample"], b["prev_sample"]
    rel = float((x - y).norm() / y.norm())
    print(f"order 1 vs DDIM, fp64, 5 steps, {prediction_type}: rel {rel:.2e}")
    assert rel < 1e-12, rel


# ---- convergence on the Gaussian ODE -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss_errors():
    return {(k, s): D.gauss_error(k, s) for k in (20, 25, 50, 100) for s in D.SAMPLERS}


@pytest.mark.parametrize("k", [20, 25, 50])
def test_gaussian_ode_2m_halves_ddim_error(gauss_errors, k):
    ddim, ms = gauss_errors[(k, "ddim")], gauss_errors[(k, "dpmsolver++")]
    print(f"Gaussian ODE, {k} steps: DDIM {ddim:.3e}, 2M {ms:.3e}, ratio {ms / ddim:.2f}")
    assert ms <= 0.5 * ddim, (ms, ddim)


def test_gaussian_ode_2m_at_25_beats_ddim_at_100(gauss_errors):
    assert gauss_errors[(25, "dpmsolver++")] < gauss_errors[(100, "ddim")], gauss_errors


def test_gaussian_ode_fp32_figures_hold_in_fp64(gauss_errors):
    for k in (20, 50):
        for s in D.SAMPLERS:
            assert abs(D.gauss_error(k, s, torch.float64) / gauss_errors[(k, s)] - 1) < 1e-3


# ---- the loop restatement ------------------------------------------------------------------------------------------------
def _oracle(cls, sched, name):
    from tests.ddim_variants import embed_fn
    from tests.fakes import FakeUNet, FakeVAE
    c = D.SOLVER_CASES[name]
    orc = cls(FakeUNet(c["sample"]), FakeVAE(), sched, embed_fn(False), sd_version=c["sd"], view_batch_size=D.VBS)
    orc.seed_everything(D.SEED)
    return orc


def test_solver_oracle_with_ddim_is_img2img_oracle_bit_for_bit():
    from tests.ddim_variants import DDIMVariants
    from tests.img2img_cpu import Img2ImgOracle
    name = "eps_leading_repaint"
    c = D.SOLVER_CASES[name]
    rng = np.random.RandomState(5)
    init = rng.randint(0, 256, (c["H"], c["W"], 3)).astype(np.uint8)
    mask = np.zeros((c["H"], c["W"]), np.uint8)
    mask[:, c["W"] // 2:] = 255
    kw = dict(D.case_kwargs(name), guidance_rescale=0.7, init_image=init, strength=0.75, mask_image=mask)
    want = _oracle(Img2ImgOracle, DDIMVariants(), name).generate_latent(["p"], "", **kw)
    wtail = torch.rand(4)
    got = _oracle(D.SolverOracle, D.DPMSolverCPU(sampler="ddim"), name).generate_latent(["p"], "", **kw)
    assert torch.equal(got, want) and torch.equal(torch.rand(4), wtail)
    # and the multistep sampler moves the result without moving a draw
    ms = _oracle(D.SolverOracle, D.DPMSolverCPU(), name).generate_latent(["p"], "", **kw)
    assert bool(torch.isfinite(ms).all()) and not torch.equal(ms, want) and torch.equal(torch.rand(4), wtail)


@pytest.mark.parametrize("name", list(D.SOLVER_CASES))
def test_oracle_equals_fixture(golden_dir, name):
    """SolverOracle reproduces G16 at both orders (the order-1 rows are the real reference's outputs): the same draws, and the
    latent to what another CPU's fp32 convolutions may differ by (bit for bit where the fixture was written: the test below)"""
    g = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    for order in (1, 2):
        z, tail = D.run_oracle_case(name, order)
        want = torch.from_numpy(g[f"{name}/order{order}/latent"])
        assert z.shape == want.shape and float((z - want).norm() / want.norm()) < 1e-5
        np.testing.assert_array_equal(tail.numpy(), g[f"{name}/order{order}/rng_tail"])


@pytest.mark.reference
@pytest.mark.parametrize("name", list(D.SOLVER_CASES))
def test_reference_first_order_equals_fixture(golden_dir, name):
    """Guards tests/golden/g16_dpm_solver.npz: the real reference with the first-order step injected, re-run here, gives exactly
    what is stored, and SolverOracle exactly that at order 1 and the stored latents at order 2."""
    if not reference_available():
        pytest.skip("reference checkout not present")
    g = np.load(os.path.join(golden_dir, "g16_dpm_solver.npz"))
    z, tail = D.run_reference_case(name)
    np.testing.assert_array_equal(z.numpy(), g[f"{name}/order1/latent"])
    np.testing.assert_array_equal(tail.numpy(), g[f"{name}/order1/rng_tail"])
    for order in (1, 2):
        oz, otail = D.run_oracle_case(name, order)
        np.testing.assert_array_equal(oz.numpy(), g[f"{name}/order{order}/latent"])
        np.testing.assert_array_equal(otail.numpy(), g[f"{name}/order{order}/rng_tail"])


# ---- argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors():
    from elasticdiffusion_official_amd.pipeline import check_sampler_arguments
    from elasticdiffusion_official_amd.schedule import DDIMSchedule, DPMSolverSchedule
    with pytest.raises(ValueError, match="solver_order"):
        DPMSolverSchedule(solver_order=3)
    with pytest.raises(NotImplementedError):            # it refuses what DDIMSchedule refuses
        DPMSolverSchedule(clip_sample=True)
    with pytest.raises(NotImplementedError):
        DPMSolverSchedule(prediction_type="sample")
    with pytest.raises(NotImplementedError):
        DPMSolverSchedule(timestep_spacing="karras")
    zs = DPMSolverSchedule(timestep_spacing="trailing", rescale_betas_zero_snr=True)      # epsilon at abar_t = 0, as the DDIM step
    zs.set_timesteps(5)
    with pytest.raises(ValueError, match="alpha_bar = 0"):
        zs.multistep_coefficients(zs.timesteps[0])
    with pytest.raises(ValueError, match="sampler"):
        check_sampler_arguments("euler")
    with pytest.raises(ValueError, match="solver_order"):
        check_sampler_arguments("dpmsolver++", 3)
    with pytest.raises(ValueError, match="scheduler object"):
        check_sampler_arguments("dpmsolver++", 2, DDIMSchedule())
    with pytest.raises(ValueError, match="scheduler object"):
        check_sampler_arguments("ddim", 2, DPMSolverSchedule())
    check_sampler_arguments(None, 2, DPMSolverSchedule())
    check_sampler_arguments("dpmsolver++", 1, DPMSolverSchedule(solver_order=1))
    with pytest.raises(ValueError):
        D.DPMSolverCPU(sampler="euler")
    with pytest.raises(ValueError):
        D.DPMSolverCPU(solver_order=3)


def test_from_config_dir_does_not_select_a_sampler(tmp_path):
    """a snapshot whose scheduler_config.json names a DPM scheduler class still loads as the DDIM schedule"""
    import json
    from elasticdiffusion_official_amd.schedule import DDIMSchedule, DPMSolverSchedule
    os.makedirs(tmp_path / "scheduler")
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        dict(_class_name="DPMSolverMultistepScheduler", prediction_type="v_prediction", solver_order=2)))
    s = DDIMSchedule.from_config_dir(str(tmp_path))
    assert type(s) is DDIMSchedule and s.config.prediction_type == "v_prediction"
    assert type(DPMSolverSchedule.from_config_dir(str(tmp_path))) is DPMSolverSchedule


def test_cli_flags_parse():
    from elasticdiffusion_official_amd.__main__ import build_parser
    opt = build_parser().parse_args(["--prompt", "p"])
    assert opt.sampler == "ddim" and opt.solver_order == 2
    opt = build_parser().parse_args(["--prompt", "p", "--sampler", "dpmsolver++", "--solver_order", "1"])
    assert opt.sampler == "dpmsolver++" and opt.solver_order == 1
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--prompt", "p", "--sampler", "euler"])
