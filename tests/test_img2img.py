"""CPU: the specification of image-to-image / inpainting (tests/img2img_cpu.py) and the product's pure
host parts: the timestep window and the argument rules.  The kernels and the loop are tested in tests/test_img2img_gpu.py."""
import numpy as np
import pytest
import torch

from oracle.ddim import DDIMOracle
from oracle.elastic_oracle import ElasticOracle
from tests import ddim_variants as V
from tests import img2img_cpu as I
from tests.fakes import FakeUNet, FakeVAE
from tests.golden import cases

NAME = "cfg2_sd_512x1024"


def synthetic_image(H, W, seed=0):
    """uint8 [H,W,3]: a smooth gradient plus seeded noise (every byte value occurs at the sizes the tests use)"""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.linspace(0, 1, H).view(H, 1, 1), torch.linspace(0, 1, W).view(1, W, 1)
    base = torch.cat([ys.expand(H, W, 1), xs.expand(H, W, 1), (0.5 + 0.5 * torch.sin(6 * (ys + xs)))], dim=2)
    img = (base * 200 + torch.randint(0, 56, (H, W, 3), generator=g)).clamp(0, 255)
    return img.to(torch.uint8).numpy()


def half_mask(H, W, s=8):
    """uint8 [H,W] mask, 255 = repaint: the left half is kept, plus ONE isolated kept latent cell in the repainted half whose
    top-left pixel alone is black; a white pixel sits off the sampled position inside the kept half."""
    m = np.full((H, W), 255, np.uint8)
    m[:, : W // 2] = 0
    y, x = isolated_cell(W, s)
    m[s * y, s * x] = 0
    m[s * 2 + s // 2, s * 2 + s // 2] = 255
    return m


def isolated_cell(W, s=8):
    """(latent row, latent column) of the kept cell ``half_mask`` puts into the repainted half"""
    return 3, (W // 2) // s + 6


def _loop_kw(name=NAME):
    c = cases.E2E_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"],
                **dict(cases.E2E_KW, **c.get("kw", {})))


def _oracle(cls, name=NAME):
    c = cases.E2E_CASES[name]
    return cls(FakeUNet(c["sample"]), FakeVAE(), DDIMOracle(), V.embed_fn(False), sd_version=c["sd"], view_batch_size=c["vbs"])


def test_window_table():
    """values written by hand from diffusers' get_timesteps: init_timestep = min(int(T * strength), T), t_start = T - it"""
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    for fn in (I.window, DDIMSchedule.img2img_window):
        assert fn(50, 1.0) == 0
        assert fn(50, 0.8) == 10
        assert fn(50, 0.3) == 35
        assert fn(4, 0.5) == 2
        with pytest.raises(ValueError):
            fn(10, 0.05)
        for bad in (0.0, -0.5, 1.01, float("nan")):
            with pytest.raises(ValueError):
                fn(50, bad)


def test_window_function_equals_the_specification_on_a_sweep():
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    n = 0
    for T in (1, 2, 3, 4, 7, 10, 20, 25, 30, 50, 100, 1000):
        for k in range(1, 201):
            strength = k / 200
            try:
                want = I.window(T, strength)
            except ValueError:
                with pytest.raises(ValueError):
                    DDIMSchedule.img2img_window(T, strength)
                continue
            assert DDIMSchedule.img2img_window(T, strength) == want, (T, strength)
            assert 0 <= want < T
            n += 1
    assert n > 1500


def test_no_init_image_is_the_oracle_loop_bit_for_bit():
    want_orc = _oracle(ElasticOracle)
    want_orc.seed_everything(cases.E2E_CASES[NAME]["seed"])
    want = want_orc.generate_latent("p", "", **_loop_kw())
    want_tail = torch.rand(4)
    orc = _oracle(I.Img2ImgOracle)
    orc.seed_everything(cases.E2E_CASES[NAME]["seed"])
    got = orc.generate_latent("p", "", **_loop_kw())
    assert torch.equal(got, want)
    assert torch.equal(torch.rand(4), want_tail)
    assert orc.last_init_latents is None


def test_masked_run_keeps_the_init_latent_exactly_and_repaints_the_rest():
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"]), half_mask(c["H"], c["W"])
    orc = _oracle(I.Img2ImgOracle)
    orc.seed_everything(1)
    z = orc.generate_latent("p", "", **_loop_kw(), init_image=img, strength=0.5, mask_image=mask)
    z0, m = orc.last_init_latents, orc.last_mask
    assert tuple(m.shape) == (c["H"] // 8, c["W"] // 8)
    y, x = isolated_cell(c["W"])
    assert int(m[y, x]) == 0 and int(m[y, x - 1]) == 1 and int(m[y + 1, x]) == 1 and int(m[2, 2]) == 0   # the isolated cell; the off-sample pixel
    assert int((m == 0).sum()) == (c["H"] // 8) * (c["W"] // 16) + 1
    keep = (m == 0).expand_as(z)
    assert torch.equal(z[keep], z0[keep])
    assert bool((z[~keep] != z0[~keep]).all())
    # and the unmasked image-to-image run starts where it should: strength 0.5 of 4 steps = the last two
    orc.seed_everything(1)
    trace = []
    orc.generate_latent("p", "", **_loop_kw(), init_image=img, strength=0.5, trace=trace)
    assert len(trace) == 2


def test_specification_pieces():
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    x = I.to_vae_input(u8)
    assert tuple(x.shape) == (1, 3, 16, 16) and float(x.min()) == -1.0 and float(x.max()) == 1.0
    m = np.zeros((16, 24), np.uint8)
    m[0, 0], m[8, 8], m[8, 16], m[4, 4] = 128, 127, 255, 255
    assert I.latent_mask(m, 8).tolist() == [[1, 0, 0], [0, 0, 1]]
    assert I.latent_mask(np.array([[0, 3], [255, 0]], np.uint8), 1).tolist() == [[0, 1], [1, 0]]
    z0, noise, xx = torch.full((1, 1, 2, 2), 2.0), torch.full((1, 1, 2, 2), float("inf")), torch.ones(1, 1, 2, 2)
    out = I.blend(xx, torch.tensor([[1, 0], [0, 1]], dtype=torch.uint8), z0, noise, 1.0, 0.0, clean=True)
    assert out.flatten().tolist() == [1.0, 2.0, 2.0, 1.0]


def test_argument_rules_of_the_pipeline_keywords():
    from elasticdiffusion_official_amd.pipeline import check_img2img_arguments
    img = synthetic_image(8, 8)
    assert check_img2img_arguments(50) == 0
    assert check_img2img_arguments(50, img, 0.8) == 10
    assert check_img2img_arguments(50, img, 1.0, np.zeros((8, 8), np.uint8)) == 0
    with pytest.raises(ValueError, match="init_image"):
        check_img2img_arguments(50, None, 0.5)
    with pytest.raises(ValueError, match="init_image"):
        check_img2img_arguments(50, None, 1.0, np.zeros((8, 8), np.uint8))
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="strength"):
            check_img2img_arguments(50, img, bad)
    with pytest.raises(ValueError, match="strength"):
        check_img2img_arguments(10, img, 0.05)


def test_command_line_has_the_flags():
    from elasticdiffusion_official_amd.__main__ import build_parser, main
    opt = build_parser().parse_args(["--init_image", "a.png", "--strength", "0.5", "--mask_image", "m.png"])
    assert (opt.init_image, opt.strength, opt.mask_image) == ("a.png", 0.5, "m.png")
    opt = build_parser().parse_args([])
    assert (opt.init_image, opt.strength, opt.mask_image) == (None, 1.0, None)
    with pytest.raises(SystemExit):
        main(["--strength", "0.5"])                       # no init image
    with pytest.raises(SystemExit):
        main(["--init_image", "a.png", "--strength", "1.5"])
