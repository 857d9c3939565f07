"""CPU: ``DDIMSchedule`` with v-prediction, linspace / trailing timestep spacing and zero-terminal-SNR betas against the
test-side restatement (tests/ddim_variants.py), its config-file constructor, what it still refuses, and -- where the
reference checkout exists -- the g13 fixtures against a fresh run of the real reference."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ddim_variants as V

SPACINGS = ("leading", "linspace", "trailing")


def _pair(spacing, zsnr, prediction_type="v_prediction", k=None):
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    kw = dict(prediction_type=prediction_type, timestep_spacing=spacing, rescale_betas_zero_snr=zsnr)
    sch, orc = DDIMSchedule(**kw), V.DDIMVariants(**kw)
    if k is not None:
        sch.set_timesteps(k)
        orc.set_timesteps(k)
    return sch, orc


def _f32(v):
    return float(torch.as_tensor(v, dtype=torch.float32))


@pytest.mark.parametrize("zsnr", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("k", [4, 7, 20, 50])
def test_timesteps_and_scalars_equal_the_restatement(k, spacing, zsnr):
    """Every scalar the kernels consume, compared exactly (==) with the fp32 0-d tensors the restatement's step /
    add_noise / the reference's undo_step (ED:692-704) would use."""
    sch, orc = _pair(spacing, zsnr, k=k)
    assert sch.timesteps.dtype == torch.int64 and torch.equal(sch.timesteps, orc.timesteps)
    assert torch.equal(sch.betas, orc.betas) and torch.equal(sch.alphas_cumprod, orc.alphas_cumprod)
    assert torch.equal(sch.final_alpha_cumprod, orc.final_alpha_cumprod)
    n = orc.config.num_train_timesteps
    ts = [int(t) for t in orc.timesteps]
    for t in ts:
        prev_t = t - n // k
        a_t = orc.alphas_cumprod[t]
        a_prev = orc.alphas_cumprod[prev_t] if prev_t >= 0 else orc.final_alpha_cumprod
        want = ((1 - a_t) ** 0.5, a_t ** 0.5, a_prev ** 0.5, (1 - a_prev - 0.0 ** 2) ** 0.5)
        assert sch.step_coefficients(t) == tuple(_f32(v) for v in want), t
        assert sch.add_noise_coefficients(t) == (_f32(a_t ** 0.5), _f32((1 - a_t) ** 0.5)), t
    for t in ts[1:]:  # undo_step is only entered with timesteps[i + 1] (ED:1040)
        b = orc.betas[t: t + n // k]
        want = torch.stack([(1 - b) ** 0.5, b ** 0.5], dim=1)
        got = sch.undo_coefficients(t)
        assert got.dtype == torch.float32 and torch.equal(got, want), t
    if zsnr:
        assert float(sch.alphas_cumprod[-1]) == 0.0 and float(sch.betas[-1]) == 1.0


def test_fixture_case_timesteps():
    """The timesteps written into the issue's table, for the product schedule and the restatement alike."""
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    for name, c in V.VARIANT_CASES.items():
        assert DDIMSchedule(**c["sched"]).set_timesteps(c["steps"]).tolist() == c["timesteps"], name
        orc = V.DDIMVariants(**c["sched"])
        orc.set_timesteps(c["steps"])
        assert orc.timesteps.tolist() == c["timesteps"], name


def test_v_step_of_the_scalars_equals_the_restatement_step():
    """The scalars combined in the kernels' operation order on the CPU (separately rounded fp32 products) reproduce
    ``DDIMVariants.step`` bit for bit -- including the alpha_bar = 0 timestep of a zero-SNR schedule."""
    sch, orc = _pair("trailing", True, k=5)
    g = torch.Generator().manual_seed(5)
    v, x = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    for t in orc.timesteps:
        sb, sa, sp, sd = (torch.tensor(c, dtype=torch.float32) for c in sch.step_coefficients(t))
        x0 = sa * x - sb * v
        eps = sa * v + sb * x
        prev = sp * x0 + sd * eps
        out = orc.step(v, t, x)
        assert torch.equal(x0, out["pred_original_sample"]) and torch.equal(prev, out["prev_sample"])
        assert bool(torch.isfinite(prev).all())
    assert sch.step_coefficients(999)[1] == 0.0


def test_default_schedule_is_unchanged():
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    from oracle.ddim import DDIMOracle
    sch, orc = DDIMSchedule(), DDIMOracle()
    assert sch.config.prediction_type == "epsilon" and sch.config.timestep_spacing == "leading"
    assert sch.config.rescale_betas_zero_snr is False
    orc.set_timesteps(50)
    assert torch.equal(sch.set_timesteps(50), orc.timesteps) and torch.equal(sch.betas, orc.betas)


def test_from_config_dir_reads_v_trailing_zero_snr(tmp_path):
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    os.makedirs(tmp_path / "scheduler")
    cfg = dict(_class_name="DDIMScheduler", _diffusers_version="0.21.4", num_train_timesteps=1000, beta_start=0.00085,
               beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False, steps_offset=1,
               prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True,
               thresholding=False, trained_betas=None)
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    sch = DDIMSchedule.from_config_dir(str(tmp_path))
    assert sch.config.prediction_type == "v_prediction" and sch.config.timestep_spacing == "trailing"
    assert sch.config.rescale_betas_zero_snr is True
    orc = V.DDIMVariants(prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True)
    orc.set_timesteps(5)
    assert torch.equal(sch.set_timesteps(5), orc.timesteps) and torch.equal(sch.alphas_cumprod, orc.alphas_cumprod)
    # single keys overridden (the command line's flags); None = keep the file's value
    over = DDIMSchedule.from_config_dir(str(tmp_path), timestep_spacing="linspace", prediction_type=None)
    assert over.config.timestep_spacing == "linspace" and over.config.prediction_type == "v_prediction"
    assert over.config.rescale_betas_zero_snr is True
    # no snapshot: the defaults plus the overrides
    bare = DDIMSchedule.from_config_dir(None, prediction_type="v_prediction")
    assert bare.config.prediction_type == "v_prediction" and bare.config.timestep_spacing == "leading"


def test_zero_snr_with_epsilon_prediction_raises_at_the_zero_timestep():
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    sch = DDIMSchedule(timestep_spacing="trailing", rescale_betas_zero_snr=True)
    ts = sch.set_timesteps(4)
    assert int(ts[0]) == 999
    with pytest.raises(ValueError, match="alpha_bar = 0"):
        sch.step_coefficients(ts[0])
    assert all(np.isfinite(sch.step_coefficients(ts[1])))  # the other timesteps are fine
    # leading spacing never visits timestep 999: the same betas are usable with epsilon prediction
    lead = DDIMSchedule(rescale_betas_zero_snr=True)
    assert all(np.isfinite(c) for t in lead.set_timesteps(4) for c in lead.step_coefficients(t))


@pytest.mark.parametrize("kw", [dict(clip_sample=True), dict(prediction_type="sample"), dict(timestep_spacing="karras")])
def test_what_stays_refused(kw):
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    with pytest.raises(NotImplementedError):
        DDIMSchedule(**kw)


def test_ops_reject_an_unknown_prediction_type():
    from elasticdiffusion_official_amd import ops
    with pytest.raises(RuntimeError, match="prediction_type"):
        ops.cfg_ddim_step(*(torch.zeros(8) for _ in range(5)), 1.0, 1.0, 1.0, 1.0, 1.0, prediction_type="sample")


def test_command_line_has_the_scheduler_flags():
    import subprocess
    import sys
    from elasticdiffusion_official_amd import _hip
    out = subprocess.run([sys.executable, "-m", "elasticdiffusion_official_amd", "--help"], cwd=_hip.ROOT_DIR,
                         capture_output=True, text=True, timeout=300, check=True).stdout
    for flag in ("--prediction_type", "--timestep_spacing", "--rescale_betas_zero_snr"):
        assert flag in out


def test_abi_has_the_prediction_type_entry_points():
    from elasticdiffusion_official_amd import _hip
    assert _hip.ABI_VERSION >= 11
    for name in ("ed_cfg_ddim_step", "ed_rrg_update", "ed_phase_epilogue"):
        assert _hip.SIGNATURES[name + "_pt"][:-2] == _hip.SIGNATURES[name][:-1]  # + int prediction_type before the stream
        assert _hip.SIGNATURES[name + "_pt"][-2:] == [_hip._i, _hip._vp]


@pytest.mark.reference
@pytest.mark.parametrize("name", list(V.VARIANT_CASES))
def test_fixtures_equal_a_fresh_reference_run(golden_dir, name):
    """Guards tests/golden/g13_scheduler_variants.npz: the real reference, re-run here, gives exactly what is stored (and
    the oracle exactly what the reference gives)."""
    from tests.golden.ref_loader import reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    g = np.load(os.path.join(golden_dir, "g13_scheduler_variants.npz"))
    z, tail, ts = V.run_reference_case(name)
    assert ts == V.VARIANT_CASES[name]["timesteps"]
    assert np.array_equal(z.numpy(), g[f"{name}/latent"]) and np.array_equal(tail.numpy(), g[f"{name}/rng_tail"])
    want, otail = V.run_oracle_case(name)
    assert torch.equal(want, z) and torch.equal(otail, tail)
