"""CPU: the specification of soft-edged inpainting (tests/soft_inpaint_cpu.py) held to Pillow and numpy, the
graded rule, the restated loop against ``Img2ImgOracle``, and the product's pure host parts (box parameters, argument rules,
command-line flags).  The kernels and the loop are tested in tests/test_soft_inpaint_gpu.py."""
import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle
from tests import ddim_variants as V
from tests import img2img_cpu as I
from tests import soft_inpaint_cpu as S
from tests.fakes import FakeUNet, FakeVAE
from tests.golden import cases
from tests.test_img2img import half_mask, synthetic_image

NAME = "cfg2_sd_512x1024"
BLUR_SHAPES = [(64, 128), (37, 53), (5, 300), (256, 256)]
BLUR_RADII = [0.5, 1, 2, 3.3, 4, 8, 16, 33, 70]


def noise_mask(H, W, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H, W), dtype=np.uint8)


def block_mask(H, W):
    """0 / 255 with a white block that touches neither edge where the image is large enough, and one that touches the corner"""
    m = np.zeros((H, W), np.uint8)
    m[H // 4:H // 4 * 3 + 1, W // 3:W // 3 * 2 + 1] = 255
    m[: max(1, H // 8), : max(1, W // 8)] = 255
    return m


def ramp_mask(H, W, s=8):
    """uint8 [H,W]: black left quarter, white right quarter, a ramp through every grey level in between (constant per s-cell)"""
    x = np.arange(W) // s * s
    g = np.clip((x - W // 4) * 255.0 / (W // 2 - s), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(g, (H, W)))


def _loop_kw(name=NAME):
    c = cases.E2E_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"],
                **dict(cases.E2E_KW, **c.get("kw", {})))


def _oracle(cls, name=NAME):
    c = cases.E2E_CASES[name]
    return cls(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), V.embed_fn(False), sd_version=c["sd"], view_batch_size=c["vbs"])


# ---- the blur ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", BLUR_SHAPES)
def test_blur_restatement_equals_pillow(H, W):
    """includes r = 0 (radius 0.5) and lines shorter than 2r + 1 (5 x 300 from radius 4 up), Pillow's other branch"""
    from PIL import Image, ImageFilter
    for img in (noise_mask(H, W), block_mask(H, W)):
        for radius in BLUR_RADII:
            want = np.array(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))
            assert np.array_equal(S.gaussian_blur(img, radius), want), (H, W, radius, S.box_parameters(radius))
    assert S.box_parameters(0.5)[0] == 0 and 2 * S.box_parameters(4)[0] + 1 > 5


def test_product_box_parameters_equal_the_restatement():
    from elasticdiffusion_official_amd import ops
    for radius in BLUR_RADII + [0.0, 0.1, 1.7320508, 100, 255.5, ops.MASK_BLUR_MAX]:
        r, ww, fw = ops.gaussian_box_parameters(radius)
        assert (r, ww, fw) == S.box_parameters(radius), radius
        assert r >= 0 and ww > 0 and fw >= 0 and (2 * r + 1) * ww + 2 * fw <= 1 << 24     # the result of a pass is a byte
    assert ops.gaussian_box_parameters(0.0) == (0, 1 << 24, 0)                            # the identity
    for bad in (-1.0, float("nan"), float("inf"), ops.MASK_BLUR_MAX + 1, "x"):
        with pytest.raises(ValueError):
            ops.gaussian_box_parameters(bad)


# ---- the composite ----------------------------------------------------------------------------------------------------
def test_composite_restatement_equals_pillow_on_every_byte_triple():
    from PIL import Image
    init_v, m_v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    init_i, m_i = Image.fromarray(init_v), Image.fromarray(m_v)
    for u in range(256):
        u_v = np.full((256, 256), u, np.uint8)
        want = np.array(Image.composite(Image.fromarray(u_v), init_i, m_i))
        assert np.array_equal(S.composite_bytes(u_v, init_v, m_v), want), u
    assert np.array_equal(S.composite_bytes(u_v, init_v, np.zeros_like(m_v)), init_v)       # m = 0: the init picture
    assert np.array_equal(S.composite_bytes(u_v, init_v, np.full_like(m_v, 255)), u_v)      # m = 255: the decoded one


def test_to_bytes_truncates_the_fp32_product():
    k = torch.arange(256, dtype=torch.float32)
    exact = k / 255
    below = torch.nextafter(exact, torch.tensor(-1.0))
    got, got_below = S.to_bytes(exact), S.to_bytes(below)
    assert torch.equal(got, (exact * 255).byte())
    # k / 255 * 255 rounds to k or just below it: the byte is k or k - 1, never k + 1; just below k / 255 it is at most k
    assert bool(((got.int() - k.int()).abs() <= 1).all()) and bool((got.int() <= k.int()).all())
    assert bool((got_below.int() <= got.int()).all()) and int(S.to_bytes(torch.tensor([1.0]))) == 255


def test_canvas_pad_equals_numpy_edge_padding():
    img = synthetic_image(13, 19, seed=2)
    for left, top, right, bottom in ((0, 0, 0, 0), (3, 0, 0, 0), (0, 5, 0, 2), (4, 1, 7, 9)):
        canvas, mask = S.canvas_pad(img, left, top, right, bottom)
        assert np.array_equal(canvas, np.pad(img, ((top, bottom), (left, right), (0, 0)), mode="edge"))
        want = np.pad(np.zeros((13, 19), np.uint8), ((top, bottom), (left, right)), constant_values=255)
        assert np.array_equal(mask, want)


# ---- the graded rule --------------------------------------------------------------------------------------------------
def test_thr_table_monotone_and_binary_on_0_255():
    assert [S.thr(j, 4) for j in (1, 2, 3, 4)] == [191, 127, 63, 0]
    for T in (4, 7, 20, 50):
        ts = [S.thr(j, T) for j in range(1, T + 1)]
        assert all(a >= b for a, b in zip(ts, ts[1:])) and ts[-1] == 0 and ts[0] < 255
        for j in range(1, T + 1):
            # on 0 / 255 levels the test is the binary rule at every j: 0 is held (kept), 255 never
            level = torch.tensor([0, 255], dtype=torch.uint8)
            held = level <= S.thr(j, T)
            assert held.tolist() == [True, False] == (I.latent_mask(level.numpy()[None], 1)[0] == 0).tolist()


def test_level_map_samples_the_top_left_pixel():
    m = noise_mask(16, 24)
    lv = S.level_map(m, 8)
    assert lv.dtype == torch.uint8 and lv.tolist() == [[int(m[0, 0]), int(m[0, 8]), int(m[0, 16])], [int(m[8, 0]), int(m[8, 8]), int(m[8, 16])]]
    assert torch.equal((lv >= 128).to(torch.uint8), I.latent_mask(m, 8))


# ---- the loop ---------------------------------------------------------------------------------------------------------
def test_graded_on_a_0_255_mask_is_the_img2img_oracle_bit_for_bit():
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"]), half_mask(c["H"], c["W"])
    ref = _oracle(I.Img2ImgOracle)
    ref.seed_everything(1)
    want = ref.generate_latent("p", "", **_loop_kw(), init_image=img, strength=0.5, mask_image=mask)
    want_tail = torch.rand(4)
    for mode in ("graded", "binary"):
        orc = _oracle(S.SoftInpaintOracle)
        orc.seed_everything(1)
        got = orc.generate_latent("p", "", **_loop_kw(), init_image=img, strength=0.5, mask_image=mask, mask_mode=mode)
        assert torch.equal(got, want), mode
        assert torch.equal(torch.rand(4), want_tail), mode
        assert torch.equal(orc.last_init_latents, ref.last_init_latents)
    # a bool mask at latent resolution is 0 / 255
    orc.seed_everything(1)
    got = orc.generate_latent("p", "", **_loop_kw(), init_image=img, strength=0.5, mask_image=I.latent_mask(mask, 8).bool(),
                              mask_mode="graded")
    assert torch.equal(got, want)


def test_grey_ramp_keeps_level_0_exactly_and_differs_from_binary_below_128():
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"]), ramp_mask(c["H"], c["W"])
    out = {}
    for mode in ("graded", "binary"):
        orc = _oracle(S.SoftInpaintOracle)
        orc.seed_everything(1)
        out[mode] = orc.generate_latent("p", "", **_loop_kw(), init_image=img, mask_image=mask, mask_mode=mode)
        if mode == "graded":
            z0, level = orc.last_init_latents, orc.last_levels
    lv = level.expand_as(z0)
    assert int((level == 0).sum()) > 0 and int(((level > 0) & (level < 128)).sum()) > 0 and int((level == 255).sum()) > 0
    assert torch.equal(out["graded"][lv == 0], z0[lv == 0])
    # T = 4: levels 1..63 are released after j = 3 only (the last blend holds level 0 alone), so they end repainted where the
    # binary run keeps them
    mid = (lv > 0) & (lv < 128)
    assert torch.equal(out["binary"][mid], z0[mid])
    assert bool((out["graded"][mid] != out["binary"][mid]).any())
    assert bool((out["graded"][lv == 255] != z0[lv == 255]).all())


def test_blurred_mask_reaches_the_loop():
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"]), half_mask(c["H"], c["W"])
    orc = _oracle(S.SoftInpaintOracle)
    orc.seed_everything(1)
    orc.generate_latent("p", "", **_loop_kw(), init_image=img, mask_image=mask, mask_blur=8, mask_mode="graded")
    assert np.array_equal(orc.last_pixel_mask, S.gaussian_blur(mask, 8))
    assert torch.equal(orc.last_levels, S.level_map(S.gaussian_blur(mask, 8), 8))
    assert 2 < len(orc.last_levels.unique()) <= 256


# ---- argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules_of_the_soft_inpaint_keywords():
    from elasticdiffusion_official_amd import ops
    from elasticdiffusion_official_amd.pipeline import check_soft_inpaint_arguments as chk
    img, mask = synthetic_image(16, 16), np.zeros((16, 16), np.uint8)
    lat = torch.zeros(2, 2, dtype=torch.uint8)
    assert chk() == 0.0 and chk(img, mask, 4, "graded", True) == 4.0 and chk(img, lat, 0, "graded", latent_size=(2, 2)) == 0.0
    assert chk(img, mask, ops.MASK_BLUR_MAX) == ops.MASK_BLUR_MAX
    for kw in (dict(mask_blur=2.0), dict(mask_mode="graded"), dict(composite=True)):
        with pytest.raises(ValueError, match="mask_image"):
            chk(img, None, **kw)
    for bad in (-1.0, float("nan"), float("inf"), ops.MASK_BLUR_MAX + 0.5, "much"):
        with pytest.raises(ValueError, match="mask_blur"):
            chk(img, mask, bad)
    with pytest.raises(ValueError, match="mask_mode"):
        chk(img, mask, 0.0, "soft")
    with pytest.raises(ValueError, match="8-bit picture mask"):
        chk(img, lat, 2.0, latent_size=(2, 2))
    with pytest.raises(ValueError, match="8-bit picture mask"):
        chk(img, lat.bool(), 2.0, latent_size=(2, 2))
    with pytest.raises(ValueError, match="8-bit init_image"):
        chk(torch.zeros(1, 3, 16, 16), mask, composite=True)
    with pytest.raises(ValueError, match="output_type"):
        chk(img, mask, composite=True, output_type="pt")
    with pytest.raises(ValueError, match="grid"):
        chk(img, mask, composite=True, grid=True)
    with pytest.raises(ValueError, match="8-bit picture mask"):
        chk(img, lat, composite=True, latent_size=(2, 2))


def test_command_line_has_the_flags():
    from elasticdiffusion_official_amd.__main__ import build_parser, main
    opt = build_parser().parse_args(["--mask_blur", "6.5", "--mask_mode", "graded", "--composite", "--outpaint", "8,0,16,0"])
    assert (opt.mask_blur, opt.mask_mode, opt.composite, opt.outpaint) == (6.5, "graded", True, "8,0,16,0")
    opt = build_parser().parse_args([])
    assert (opt.mask_blur, opt.mask_mode, opt.composite, opt.outpaint) == (0.0, "binary", False, None)
    for argv in (["--mask_blur", "4"], ["--mask_mode", "graded"], ["--composite"],               # no mask
                 ["--init_image", "a.png", "--mask_blur", "4"],
                 ["--outpaint", "8,8,8,8"],                                                        # no init image
                 ["--init_image", "a.png", "--mask_image", "m.png", "--outpaint", "8,8,8,8"],      # exclusive
                 ["--init_image", "a.png", "--outpaint", "8,8,8"], ["--init_image", "a.png", "--outpaint", "0,0,0,0"],
                 ["--init_image", "a.png", "--outpaint", "8,-1,0,0"]):
        with pytest.raises(SystemExit):
            main(argv)
