"""CPU: guidance rescale -- the reference-held fixture g15, the torch restatement the GPU tests compare with
(tests/guidance_rescale_cpu.py), and the public surface (keyword, validation, command line, C ABI)."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle
from oracle.elastic_oracle import ElasticOracle
from tests import guidance_rescale_cpu as G
from tests.fakes import FakeUNet, FakeVAE
from tests.golden import cases

CASES = G.g15_cases()


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_guidance_rescale.npz"))


def test_fixture_holds_every_case_and_no_inputs(g15):
    want = {"torch_version"}
    for key, _, _, _ in CASES:
        want |= {f"{key}/seed", f"{key}/ratio_fp64"} | {f"{key}/gr{gr}/out" for gr in G.G15_RESCALES}
    assert set(g15.files) == want
    assert len(CASES) == 8 and sorted(G.G15_RESCALES) == [0.7, 1.0]


@pytest.mark.parametrize("key,shape,mean,seed", CASES)
def test_restatement_equals_reference_fixture_bit_for_bit(g15, key, shape, mean, seed):
    assert int(g15[f"{key}/seed"]) == seed
    local, direction, m_cfg, m_text = G.g15_inputs(seed, shape, mean)
    assert m_cfg.dtype == torch.float32 and abs(float(local.mean()) - mean) < 0.2
    for gr in G.G15_RESCALES:
        got = G.rescale_guided(m_cfg, m_text, gr)
        np.testing.assert_array_equal(G.g15_probe(got).numpy(), g15[f"{key}/gr{gr}/out"])
    # the stored fp64 ratios are those of the regenerated inputs, and torch's own fp32 ratio is well inside the 2-ulp bar
    r64 = G.ratio_fp64(m_cfg, m_text).numpy()
    np.testing.assert_allclose(r64, g15[f"{key}/ratio_fp64"], rtol=1e-13, atol=0)
    r32 = (G.sample_std(m_text) / G.sample_std(m_cfg)).flatten().double().numpy()
    assert np.abs(r32 - r64).max() / r64.min() < 2.4e-7
    # the split the kernels implement (ratio, then the elementwise part) is the same function
    ratio = (G.sample_std(m_text) / G.sample_std(m_cfg)).flatten()
    assert torch.equal(G.rescale_with_ratio(m_cfg, ratio, 0.7), G.rescale_guided(m_cfg, m_text, 0.7))


@pytest.mark.parametrize("key,shape,mean,seed", CASES)
def test_fixture_equals_a_fresh_reference_run(g15, key, shape, mean, seed):
    from tests.golden.ref_loader import load_reference, reference_available
    if not reference_available():
        pytest.skip("needs the reference checkout (builder container only)")
    ref = load_reference()
    _, _, m_cfg, m_text = G.g15_inputs(seed, shape, mean)
    for gr in G.G15_RESCALES:
        got = ref.ElasticDiffusion.rescale_noise_cfg(None, m_cfg, m_text, gr)
        np.testing.assert_array_equal(G.g15_probe(got).numpy(), g15[f"{key}/gr{gr}/out"])


def test_naive_fp32_sum_of_squares_misses_the_bar_on_large_means():
    """Why the accumulation is specified: the plain fp32 sum / sum of squares is ~1e-4 off at mean 50, std 1."""
    key, shape, mean, seed = next(c for c in CASES if c[2] == 50.0 and c[1] == (1, 4, 128, 256))
    _, _, m_cfg, m_text = G.g15_inputs(seed, shape, mean)

    def naive_std(x):
        x = x.flatten()
        s, ss, n = np.float32(0), np.float32(0), np.float32(x.numel())
        for chunk in x.numpy().reshape(-1, 256):  # sequential fp32 accumulation of 256-wide partial sums
            s = np.float32(s + chunk.sum(dtype=np.float32))
            ss = np.float32(ss + (chunk * chunk).sum(dtype=np.float32))
        return np.sqrt(np.float32((ss - s * s / n) / (n - np.float32(1))))

    naive = float(naive_std(m_text)) / float(naive_std(m_cfg))
    r64 = float(G.ratio_fp64(m_cfg, m_text)[0])
    assert abs(naive - r64) / r64 > 10 * 2.4e-7


def test_subclass_without_rescale_is_the_unmodified_oracle():
    c = cases.E2E_CASES["cfg2_sd_512x1024"]
    kw = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)

    def embed_fn():
        from tests.fakes import synthetic_text_embeds
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        st = {"n": 0}

        def fn(_):
            st["n"] += 1
            return (un, pun) if st["n"] % 2 == 1 else (co, pco)
        return fn

    out = {}
    for cls in (ElasticOracle, G.RescaleOracle):
        orc = cls(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), embed_fn(), sd_version=c["sd"], view_batch_size=c["vbs"])
        orc.seed_everything(c["seed"])
        extra = {} if cls is ElasticOracle else dict(guidance_rescale=0.0)
        out[cls] = (orc.generate_latent("p", "", **kw, **extra), torch.rand(4))
    assert torch.equal(out[ElasticOracle][0], out[G.RescaleOracle][0])
    assert torch.equal(out[ElasticOracle][1], out[G.RescaleOracle][1])
    # and the rescale changes the result (RRG is active in this case: both hooks are reached)
    orc = G.RescaleOracle(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), embed_fn(), sd_version=c["sd"], view_batch_size=c["vbs"])
    orc.seed_everything(c["seed"])
    z = orc.generate_latent("p", "", **kw, guidance_rescale=0.7)
    assert bool(torch.isfinite(z).all()) and float((z - out[ElasticOracle][0]).norm() / out[ElasticOracle][0].norm()) > 1e-3
    assert torch.equal(torch.rand(4), out[ElasticOracle][1])  # the rescale draws nothing from the host generators
    with pytest.raises(ValueError):
        orc.generate_latent("p", "", **kw, guidance_rescale=1.5)


# ---- public surface -------------------------------------------------------------------------------------------------
def test_keyword_on_every_public_method_defaults_to_zero():
    from elasticdiffusion_official_amd import ElasticDiffusion, ElasticDiffusionControlNet
    methods = [ElasticDiffusion.generate_image, ElasticDiffusionControlNet.generate_image, ElasticDiffusion.generate_latents,
               ElasticDiffusion.generate_latents_interleaved, ElasticDiffusion.generate]
    for m in methods:
        p = inspect.signature(m).parameters
        assert "guidance_rescale" in p and p["guidance_rescale"].default == 0.0, m.__qualname__
    # appended: the positional order the reference's callers rely on is unchanged
    base = list(inspect.signature(ElasticDiffusion.generate_image).parameters)
    assert base[:18] == ["self", "prompts", "negative_prompts", "height", "width", "num_inference_steps", "guidance_scale",
                         "resampling_steps", "new_p", "rrg_stop_t", "rrg_init_weight", "rrg_scherduler_cls", "cosine_scale",
                         "repaint_sampling", "progress", "tiled_decoder", "grid", "guidance_rescale"]
    cn = list(inspect.signature(ElasticDiffusionControlNet.generate_image).parameters)
    assert cn[:4] == ["self", "prompts", "negative_prompts", "condition_image"] and cn[7:9] == ["guidance_scale", "controlnet_conditioning_scale"]
    assert cn[17:20] == ["tiled_decoder", "grid", "guidance_rescale"]


@pytest.mark.parametrize("bad", [1.5, -0.1, float("nan")])
def test_values_outside_unit_interval_raise(bad):
    from elasticdiffusion_official_amd import ops
    with pytest.raises(ValueError, match="guidance_rescale"):
        ops.rescale_coefficients(bad)


def test_rescale_coefficients_are_the_fp32_scalars_torch_uses():
    from elasticdiffusion_official_amd import ops
    assert ops.rescale_coefficients(0.0) == (0.0, 1.0) and ops.rescale_coefficients(1.0) == (1.0, 0.0)
    gr, omgr = ops.rescale_coefficients(0.7)
    assert gr == float(np.float32(0.7)) and omgr == float(np.float32(1 - 0.7))
    x = torch.tensor([1.2345678, -3.25, 1e-3])
    assert torch.equal(0.7 * x, torch.tensor(gr) * x) and torch.equal((1 - 0.7) * x, torch.tensor(omgr) * x)


def test_cli_parses_the_flag():
    from elasticdiffusion_official_amd.__main__ import build_parser
    ap = build_parser()
    assert ap.parse_args([]).guidance_rescale == 0.0
    assert ap.parse_args(["--guidance_rescale", "0.7"]).guidance_rescale == 0.7


def test_abi_13_declares_the_rescale_entry_points():
    from elasticdiffusion_official_amd import _hip
    from tests.test_abi import header_functions
    new = {"ed_guidance_moments_workspace", "ed_guidance_moments", "ed_phase_moments", "ed_cfg_ddim_step_gr",
           "ed_rrg_update_gr", "ed_phase_epilogue_gr", "ed_cfg_ddim_step_width"}
    assert _hip.ABI_VERSION == 13 and new <= set(_hip.SIGNATURES) and new <= {n for n, _ in header_functions()}
    _hip.build_library()
    L = _hip.lib()
    assert L.ed_version() == 13
    # one partial (6 doubles) per block, a fixed number of blocks per sample: 1 below 1024 elements, at most 256
    assert L.ed_guidance_moments_workspace(1, 256, 0) == 48
    assert L.ed_guidance_moments_workspace(2, 4 * 33 * 47, 0) == 2 * 7 * 48
    assert L.ed_guidance_moments_workspace(1, 4 * 128 * 256, 4 * 64 * 128) == (128 + 32) * 48
    assert L.ed_guidance_moments_workspace(3, 1 << 30, 0) == 3 * 256 * 48


def test_plain_ddim_step_keeps_its_16_byte_path():
    """No GPU needed: ed_cfg_ddim_step_width launches nothing and only looks at the addresses.  Without a ratio the choice is
    the one the plain entry points always made (n % 4 and alignment); a ratio adds only the per-sample length condition."""
    import ctypes
    from elasticdiffusion_official_amd import _hip
    _hip.build_library()
    L = _hip.lib()
    a, m = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    ratio = ctypes.c_void_p(0x20000)
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 4 * 64 * 128, None, 0) == 4
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 2004, None, 0) == 4
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 2003, None, 0) == 1
    assert L.ed_cfg_ddim_step_width(a, a, a, m, a, 2004, None, 0) == 1
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 4 * 64 * 128, ratio, 1) == 4
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 2004, ratio, 2) == 1      # 1002 per sample
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 2004, ratio, 1) == 4
    assert L.ed_cfg_ddim_step_width(a, a, a, a, a, 2004, ratio, 5) == 0      # not 5 equal samples
