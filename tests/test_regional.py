"""CPU: regional prompts -- the specification tests/regional_cpu.py itself, the argument rules, the command
line, and the tie of the specification to the goldens of the real reference: one region with a full mask and prompt q IS the
unmodified oracle run with prompt q, bit for bit."""
import numpy as np
import pytest
import torch

from tests import regional_cpu as RG
from tests.golden import cases

NAME = "cfg2_sd_512x1024"


def _u8(*planes):
    return torch.tensor(np.stack([np.asarray(p, np.uint8) for p in planes]))


# ---- weights ------------------------------------------------------------------------------------------------------------------
def test_one_hot_coverage_gives_exact_one_and_zero():
    left = np.zeros((4, 6), np.uint8)
    left[:, :3] = 255
    right = 255 - left
    for weights in ([1.0, 1.0], [2.0, 1.5], [3.7, 1.0]):               # full weight: >= 1 (below it the base keeps the rest)
        w = RG.region_weights(_u8(left, right), weights)
        assert w.dtype == torch.float32 and tuple(w.shape) == (3, 4, 6)
        assert torch.equal(w[0], torch.zeros(4, 6))                       # the base prompt is covered everywhere
        assert torch.equal(w[1], torch.from_numpy(left / 255).float()) and torch.equal(w[2], torch.from_numpy(right / 255).float())


def test_weights_lie_in_unit_interval_and_sum_to_one():
    g = torch.Generator().manual_seed(3)
    for n in (1, 3, 7):
        masks = torch.randint(0, 256, (n, 9, 13), generator=g, dtype=torch.uint8)
        masks[:, 0, 0] = 0
        masks[:, 0, 1] = 255
        wts = [float(v) for v in torch.rand(n, generator=g) * 3 + 0.05]
        w = RG.region_weights(masks, wts)
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0 and float(w.max()) <= 1.0
        assert float((w.sum(0) - 1).abs().max()) < 1e-6
        assert float(w[0, 0, 0]) == 1.0 and float(w[1:, 0, 0].abs().max()) == 0.0     # no coverage: the base gets exactly 1


def test_no_coverage_and_equal_overlaps():
    zero, full = np.zeros((3, 5), np.uint8), np.full((3, 5), 255, np.uint8)
    w = RG.region_weights(_u8(zero, zero), [1.0, 4.0])
    assert torch.equal(w[0], torch.ones(3, 5)) and float(w[1:].abs().max()) == 0.0
    w = RG.region_weights(_u8(full, full), [1.0, 1.0])
    assert torch.equal(w[1], torch.full((3, 5), 0.5)) and torch.equal(w[2], w[1]) and float(w[0].abs().max()) == 0.0
    w = RG.region_weights(_u8(full, full, full, full), [2.0] * 4)
    assert torch.equal(w[1:], torch.full((4, 3, 5), 0.25))
    w = RG.region_weights(_u8(full, full), [3.0, 1.0])                                 # the weight decides an overlap
    assert torch.equal(w[1], torch.full((3, 5), 0.75)) and torch.equal(w[2], torch.full((3, 5), 0.25))
    half = np.full((3, 5), 51, np.uint8)                                               # 51 / 255 = 0.2: the base keeps the rest
    w = RG.region_weights(_u8(half), [1.0])
    assert float((w[1] - 0.2).abs().max()) < 1e-7 and float((w[0] - 0.8).abs().max()) < 1e-7


def test_box_mask_is_the_drawn_rectangle():
    from PIL import Image, ImageDraw
    for box in ((0, 0, 64, 32), (8, 16, 40, 24), (63, 31, 64, 32)):
        img = Image.new("L", (64, 32), 0)
        ImageDraw.Draw(img).rectangle([box[0], box[1], box[2] - 1, box[3] - 1], fill=255)
        assert np.array_equal(RG.box_mask(box, 32, 64), np.array(img))
    # the reduction (Pillow's BILINEAR, a triangle two latent cells wide) keeps the box's area, is 255 a cell inside the edge and
    # 0 two cells outside it
    low = RG.latent_mask((32, 16, 96, 48), 64, 128)
    assert low.shape == (8, 16) and low.dtype == np.uint8
    assert (low[3:5, 5:11] == 255).all() and low[0].max() == 0 and low[:, :2].max() == 0 and low[:, 14:].max() == 0
    assert abs(float(low.sum()) / 255 - 4 * 8) < 0.5
    assert np.array_equal(low, low[::-1]) and np.array_equal(low, low[:, ::-1])
    # a latent-size mask is used as is, a blurred one is feathered
    given = np.arange(32, dtype=np.uint8).reshape(4, 8)
    assert RG.latent_mask(given, 32, 64) is not None and np.array_equal(RG.latent_mask(given, 32, 64), given)
    soft = RG.latent_mask((16, 8, 48, 24), 32, 64, region_blur=6.0)
    assert 0 < soft[1, 1] < 255 and soft.max() < 255
    with pytest.raises(ValueError):
        RG.latent_mask(np.zeros((5, 5), np.uint8), 32, 64)


def test_blend_skips_zero_weights_and_keeps_one_hot_bits():
    g = torch.Generator().manual_seed(1)
    dirs = torch.randn(3, 2, 4, 5, 7, generator=g)
    dirs[0, :, :, 0, 0] = -0.0                                        # a signed zero survives a one-hot weight
    w = torch.zeros(3, 5, 7)
    w[0, :, :3], w[2, :, 3:] = 1.0, 1.0
    dirs[1] = float("nan")                                            # never read: its weight is 0 everywhere
    d = RG.blend(dirs, w)
    assert torch.equal(d[..., :3].view(torch.int32), dirs[0][..., :3].view(torch.int32))
    assert torch.equal(d[..., 3:], dirs[2][..., 3:])
    assert float(RG.blend(dirs, torch.zeros(3, 5, 7)).abs().max()) == 0.0
    dirs[1] = torch.randn(2, 4, 5, 7, generator=g)
    w = torch.rand(3, 5, 7, generator=g)
    assert torch.equal(RG.blend(dirs, w), (w[0] * dirs[0] + w[1] * dirs[1]) + w[2] * dirs[2])


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def test_check_region_arguments():
    from elasticdiffusion_official_amd.pipeline import check_region_arguments as chk
    from PIL import Image
    H, W = 64, 128
    pix, lat = np.zeros((H, W), np.uint8), torch.zeros(H // 8, W // 8, dtype=torch.uint8)
    assert chk(None, H, W) == (None, 0.0)
    out, blur = chk([("a", pix), ("b", lat, 2), ("c", (0, 0, 64, 32)), ("d", Image.new("L", (W, H))), ("e", pix[:, :, None], 0.5)],
                    H, W, region_blur=3)
    assert blur == 3.0 and [r[0] for r in out] == list("abcde") and [r[2] for r in out] == [1.0, 2.0, 1.0, 1.0, 0.5]
    assert [r[1][0] for r in out] == ["pixel", "latent", "box", "pixel", "pixel"] and out[2][1][1] == (0, 0, 64, 32)
    assert len(chk([("a", pix)] * 7, H, W)[0]) == 7
    bad = [[], [("a", pix)] * 8, [("a",)], ["a"], [(3, pix)], [("a", pix, 0)], [("a", pix, -1.0)], [("a", pix, float("nan"))],
           [("a", pix, float("inf"))], [("a", pix, "x")], [("a", np.zeros((H, W + 8), np.uint8))], [("a", pix.astype(np.float32))],
           [("a", np.zeros((H // 4, W // 4), np.uint8))], [("a", Image.new("L", (W // 8, H // 8)))], [("a", (0, 0, 0, 8))],
           [("a", (0, 0, W + 1, 8))], [("a", (-1, 0, 8, 8))], [("a", (0, 8, 8, 8))], [("a", (0, 0, 8))], [("a", (0, 0, 8.5, 8))],
           [("a", None)]]
    for regions in bad:
        with pytest.raises(ValueError):
            chk(regions, H, W)
    for blur in (-1.0, float("nan"), 1e9, "x"):
        with pytest.raises(ValueError, match="region_blur"):
            chk([("a", pix)], H, W, region_blur=blur)
    with pytest.raises(ValueError, match="needs regions"):
        chk(None, H, W, region_blur=2.0)
    with pytest.raises(ValueError, match="9-channel"):
        chk([("a", pix)], H, W, in_channels=9)
    assert chk(None, H, W, in_channels=9) == (None, 0.0)


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_pair(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import build_parser, parse_regions
    ap = build_parser()
    assert parse_regions(ap.parse_args([])) is None
    path = str(tmp_path / "m.png")
    Image.new("L", (64, 32), 255).save(path)
    opt = ap.parse_args(["--region_prompt", "mountains", "--region_mask", "0,0,32,32", "--region_prompt", "a harbour",
                         "--region_mask", "16,0,64,32:2", "--region_prompt", "sky", "--region_mask", path + ":0.5",
                         "--region_blur", "4"])
    regions = parse_regions(opt)
    assert opt.region_blur == 4.0 and [r[0] for r in regions] == ["mountains", "a harbour", "sky"]
    assert regions[0][1:] == ((0, 0, 32, 32), 1.0) and regions[1][1:] == ((16, 0, 64, 32), 2.0)
    assert regions[2][1].mode == "L" and regions[2][1].size == (64, 32) and regions[2][2] == 0.5
    from elasticdiffusion_official_amd.pipeline import check_region_arguments
    assert len(check_region_arguments(regions, 32, 64, 8, opt.region_blur)[0]) == 3
    for argv in (["--region_prompt", "a"], ["--region_mask", "0,0,8,8"], ["--region_prompt", "a", "--region_prompt", "b",
                                                                            "--region_mask", "0,0,8,8"],
                 ["--region_blur", "2"], ["--region_prompt", "a", "--region_mask", "/no/such/file.png"]):
        with pytest.raises(SystemExit):
            parse_regions(ap.parse_args(argv))


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def _loop_kw(name):
    c = cases.E2E_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **cases.E2E_KW)


def _regional_oracle(name):
    from tests.dpm_solver_cpu import DPMSolverCPU
    from tests.fakes import FakeUNet, FakeVAE
    c = cases.E2E_CASES[name]
    return RG.RegionalOracle(FakeUNet(c["sample"]), FakeVAE(), DPMSolverCPU(sampler="ddim"), RG.prompt_embeds(False),
                             sd_version=c["sd"], view_batch_size=c["vbs"])


def test_one_full_region_is_the_plain_oracle_with_that_prompt_bit_for_bit():
    """ties the specification to the goldens of the real reference (which pin ElasticOracle): base weight 0 everywhere, the
    region's 1, so d = 1 * (c_q - u) with the base row never entering -- latents and RNG tail"""
    from oracle import elastic_oracle as eo
    from oracle.ddim import DDIMOracle
    from tests.fakes import FakeUNet, FakeVAE
    c = cases.E2E_CASES[NAME]
    q = "a harbour at dusk"
    plain = eo.ElasticOracle(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), RG.prompt_embeds(False), sd_version=c["sd"],
                             view_batch_size=c["vbs"])
    plain.seed_everything(c["seed"])
    want = plain.generate_latent(q, "", **_loop_kw(NAME))
    wtail = torch.rand(4)
    orc = _regional_oracle(NAME)
    orc.seed_everything(c["seed"])
    full = np.full((c["H"], c["W"]), 255, np.uint8)
    got = orc.generate_latent("p", "", regions=[(q, full)], **_loop_kw(NAME))
    tail = torch.rand(4)
    assert torch.equal(orc.last_region_weights[0], torch.zeros(c["H"] // 8, c["W"] // 8))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert torch.equal(tail, wtail)
    # and the prompt matters: the same run with the base prompt's own embedding is another latent
    plain.seed_everything(c["seed"])
    other = plain.generate_latent("p", "", **_loop_kw(NAME))
    assert not torch.equal(other, want)


def test_regions_change_the_picture_where_they_apply_and_not_the_rng_stream():
    c = cases.E2E_CASES[NAME]
    kw = dict(_loop_kw(NAME), num_inference_steps=2, resampling_steps=1)
    orc = _regional_oracle(NAME)
    orc.seed_everything(c["seed"])
    base = orc.generate_latent("p", "", **kw)
    btail = torch.rand(4)
    orc.seed_everything(c["seed"])
    half = np.zeros((c["H"], c["W"]), np.uint8)
    half[:, c["W"] // 2:] = 255
    got = orc.generate_latent("p", "", regions=[("q", half), ("r", (256, 128, 768, 384), 2.0)], **kw)
    assert torch.equal(torch.rand(4), btail)
    assert not torch.equal(got, base) and bool(torch.isfinite(got).all())
