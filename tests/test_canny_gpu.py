"""-m gpu: the HIP Canny kernels (csrc/canny_kernels.hip) and everything built on them -- ``ops.canny``,
``process_condition_image`` / ``prepare_condition_image``, the command line -- against the numpy restatement of the
specification (tests/canny_cpu.py).  All arithmetic is integer: every comparison is exact, no tolerance anywhere."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import canny_cpu as cc
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
from tests.test_hip_parity import _embed_fn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1, 1), (3, 5), (17, 33), (64, 96), (1000, 1000), (1024, 512), (2048, 2048)]
THRESHOLDS = [(100, 200), (50, 150), (0, 0), (200, 100), (300, 300)]
PHOTO_SIZES = [(512, 512), (1024, 1024), (1024, 512)]          # (width, height) as PIL takes them


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _gpu_canny(img, low=100, high=200):
    e = _ops().canny(torch.from_numpy(np.array(img)).to(DEV), low, high).cpu().numpy()
    assert e.shape == img.shape[:2] + (3,) and e.dtype == np.uint8
    assert np.array_equal(e[:, :, 0], e[:, :, 1]) and np.array_equal(e[:, :, 0], e[:, :, 2])
    return e[:, :, 0]


def _photo(golden_dir, size):
    from PIL import Image
    return Image.open(os.path.join(golden_dir, "canny_input_yoga.jpeg")).resize(size).convert("RGB")


def _image(kind, H, W, C, seed):
    img = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
    if kind != "noise":
        img = cc.box_blur(img, int(kind[-1]))
    return img


# ---------------------------------------------------------------------------------------------------
# ops.canny == the restatement
# ---------------------------------------------------------------------------------------------------
def test_anchors():
    a = np.zeros((16, 16), np.uint8)
    a[:, 8:] = 255
    want = np.zeros((16, 16), np.uint8)
    want[:, 7] = 255
    assert np.array_equal(_gpu_canny(a), want)
    assert np.array_equal(_gpu_canny(a.T.copy()), want.T)
    a[:, 8:] = 40
    assert not _gpu_canny(a).any()
    cmap = _ops().canny_map(torch.from_numpy(a).to(DEV)).cpu().numpy()
    assert np.array_equal(cmap, cc.canny_map(a)) and (cmap[:, 7] == 0).all()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_canny_matches_restatement(H, W, C):
    """Uniform noise (dense: about 36 % edges) and box-blurred noise (long chains), every threshold pair; the map stage is
    compared as well, so that a miss names its stage."""
    ops = _ops()
    for kind in ("noise", "blur3", "blur5"):
        img = _image(kind, H, W, C, seed=H * 7 + W * 3 + C)
        dev = torch.from_numpy(img).to(DEV)
        for lo, hi in THRESHOLDS:
            want_map = cc.canny_map(img, lo, hi)
            assert np.array_equal(ops.canny_map(dev, lo, hi).cpu().numpy(), want_map), (kind, lo, hi, "map")
            flood, _ = cc.hysteresis(want_map)
            want = np.where(flood == 2, 255, 0).astype(np.uint8)
            got = ops.canny(dev, lo, hi).cpu().numpy()
            assert np.array_equal(got, np.repeat(want[:, :, None], 3, axis=2)), (kind, lo, hi)


def test_canny_single_channel_layouts_and_float_thresholds():
    """[H,W] and [H,W,1] are the same image; thresholds are floored."""
    ops = _ops()
    img = _image("blur3", 120, 75, 1, seed=1)
    a = ops.canny(torch.from_numpy(img).to(DEV), 50.9, 150.5)
    b = ops.canny(torch.from_numpy(img[:, :, 0].copy()).to(DEV), 50, 150)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy()[:, :, 0], cc.canny(img, 50, 150))


def test_canny_cond_output_is_the_condition_tensor():
    ops = _ops()
    for H, W in ((64, 96), (33, 17), (5, 3)):        # H W % 4 == 0, and the scalar-store tails
        dev = torch.from_numpy(_image("noise", H, W, 3, seed=2)).to(DEV)
        u8 = ops.canny(dev)
        cond = ops.canny(dev, out="cond")
        assert cond.shape == (1, 3, H, W) and cond.dtype == torch.float32
        assert torch.equal(cond, u8.permute(2, 0, 1)[None].float() / 255.0)


def test_wrappers_reject_bad_arguments():
    ops = _ops()
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    for bad in (ok.float(), ok[:, :, :2].contiguous(), ok.permute(2, 0, 1), torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV),
                torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV), ok.cpu()):
        with pytest.raises(RuntimeError):
            ops.canny(bad)
    with pytest.raises(RuntimeError):
        ops.canny_hysteresis(torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.canny(ok, out="pil")
    assert torch.equal(ops.canny(ok), torch.zeros_like(ok))     # the launch state is clean after the rejections


@pytest.mark.parametrize("size", PHOTO_SIZES)
def test_sample_photo(golden_dir, size):
    """The reference's sample input (imgs/input/yoga.jpeg) resized as its command line does (PIL default filter, RGB).  The
    restatement gives 2.58 % edges at 512 x 512, 1.69 % at 1024 x 1024 and 2.16 % at 1024 x 512 (width x height); the
    assertion is equality with the restatement."""
    img = np.asarray(_photo(golden_dir, size))
    want = cc.canny(img)
    frac = float((want == 255).mean())
    print(f"photo {size}: restatement edge fraction {100 * frac:.2f} %")
    assert 0.01 < frac < 0.04
    assert np.array_equal(_gpu_canny(img), want)


# ---------------------------------------------------------------------------------------------------
# ed_canny_hysteresis on synthetic maps
# ---------------------------------------------------------------------------------------------------
def _flood(cmap):
    out, passes = _ops().canny_hysteresis(torch.from_numpy(cmap).to(DEV))
    return out.cpu().numpy(), passes


def test_hysteresis_spiral_through_every_tile():
    pts = cc.spiral_path(1024)
    cmap = np.ones((1024, 1024), np.uint8)
    cmap[pts[:, 0], pts[:, 1]] = 0
    assert (cmap.reshape(32, 32, 32, 32) == 0).any(axis=(1, 3)).all()       # every 32 x 32 block holds a piece of it
    assert len(pts) > 60000 and int((cmap == 0).sum()) == len(pts)              # one pixel wide, never crosses itself
    idle, passes = _flood(cmap)                                                 # no strong pixel: nothing happens
    assert np.array_equal(idle, cmap) and passes == 1
    cmap[pts[0, 0], pts[0, 1]] = 2                                              # strong pixel at the outer end
    want = np.where(cmap == 0, 2, cmap).astype(np.uint8)
    got, passes = _flood(cmap)
    # A pass floods at least the run of the chain up to the next tile boundary (the tile sees the pixel promoted by the pass
    # before in its halo and floods to stability in LDS), and the last pass is the empty one.  The kernel's tile is 64 x 32:
    # crossings of the 32-pixel grid bound the number of runs from above, whatever multiple of 32 a tile side is.
    step = np.abs(np.diff(pts // 32, axis=0)).sum(axis=1)
    runs = int((step != 0).sum()) + 1
    print(f"spiral: {len(pts)} pixels promoted in {passes} global passes ({runs} runs between 32-pixel grid lines)")
    assert np.array_equal(got, want)
    assert 1 < passes <= runs + 1 < len(pts) // 8                               # tiles flood in LDS, not pixel by pixel


def test_hysteresis_diagonals_cross_tile_corners():
    n = 256
    i = np.arange(n)
    for chain in ((i, i), (i, n - 1 - i)):
        for strong_end in (0, n - 1):
            cmap = np.ones((n, n), np.uint8)
            cmap[chain] = 0
            cmap[chain[0][strong_end], chain[1][strong_end]] = 2
            got, _ = _flood(cmap)
            assert np.array_equal(got, np.where(cmap == 0, 2, cmap))


def test_hysteresis_does_not_wrap_at_the_border():
    """Pixels that are neighbours only in flat memory (end of one row / start of the next) or across the image (first / last
    row or column) are not neighbours."""
    for H, W in ((64, 100), (37, 64), (96, 128)):
        cmap = np.ones((H, W), np.uint8)
        cmap[10, W - 1] = 0
        cmap[11, 0] = 2            # next byte in memory
        cmap[0, 20] = 0
        cmap[H - 1, 20] = 2        # same column, opposite border
        cmap[H - 1, W - 1] = 0
        cmap[0, 0] = 2             # opposite corner
        cmap[20, 0] = 0
        cmap[20, W - 1] = 2        # same row, opposite border
        got, passes = _flood(cmap)
        assert np.array_equal(got, cmap) and passes == 1


def test_hysteresis_random_maps_match_connected_components():
    rng = np.random.default_rng(11)
    for H, W in ((77, 131), (32, 64), (200, 333), (1, 50), (50, 1)):
        for p_cand, p_strong in ((0.45, 0.002), (0.3, 0.05), (0.6, 0.0005)):
            r = rng.random((H, W))
            cmap = np.where(r < p_strong, 2, np.where(r < p_strong + p_cand, 0, 1)).astype(np.uint8)
            got, _ = _flood(cmap)
            assert np.array_equal(got, cc.hysteresis_by_labels(cmap)), (H, W, p_cand)


def test_photo_needs_fewer_global_passes_than_dilation(golden_dir):
    """The flood inside LDS does the work: on the 1024 x 1024 photo the number of global passes is strictly below the number
    of one-pixel dilation passes the restatement needs on the same map (91 when this was written; computed here)."""
    img = np.asarray(_photo(golden_dir, (1024, 1024)))
    cmap = cc.canny_map(img)
    want, cpu_passes = cc.hysteresis(cmap)
    got, gpu_passes = _flood(cmap)
    print(f"photo 1024 x 1024: {gpu_passes} global passes on the GPU, {cpu_passes} dilation passes in the restatement")
    assert np.array_equal(got, want)
    assert 1 <= gpu_passes < cpu_passes


# ---------------------------------------------------------------------------------------------------
# process_condition_image / prepare_condition_image / end to end / command line
# ---------------------------------------------------------------------------------------------------
def _pipe(model="canny", **kw):
    from elasticdiffusion_official_amd import ElasticDiffusionControlNet
    return ElasticDiffusionControlNet(DEV, "1.5", model, view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(),
                                      text_encoder=_embed_fn(False), controlnet=FakeControlNet(), **kw)


def test_process_condition_image_canny(golden_dir):
    """Raises NotImplementedError without the feature."""
    pipe = _pipe()
    photo = _photo(golden_dir, (512, 384))
    want = cc.canny(np.asarray(photo))
    out = pipe.process_condition_image(photo, "canny")
    assert out.mode == "RGB" and out.size == (512, 384)
    arr = np.asarray(out)
    for c in range(3):
        assert np.array_equal(arr[:, :, c], want)
    assert np.array_equal(np.asarray(pipe.process_condition_image(np.asarray(photo), "canny")), arr)    # HWC uint8 array input
    pt = pipe.process_condition_image(photo, "canny", output_type="pt")
    assert pt.is_cuda and torch.equal(pt.cpu(), pipe._to_condition_tensor(out, 384, 512))
    grey = photo.convert("L")                                                                           # one channel
    assert np.array_equal(np.asarray(pipe.process_condition_image(grey, "canny"))[:, :, 0], cc.canny(np.asarray(grey)))


def test_process_condition_image_depth_and_unknown_models(golden_dir):
    from PIL import Image
    photo = _photo(golden_dir, (96, 64))
    depth = photo.convert("L")
    calls = []

    def estimator(image):
        calls.append(image)
        return {"depth": depth, "predicted_depth": None}

    out = _pipe("depth", depth_estimator=estimator).process_condition_image(photo, "depth")
    assert calls == [photo] and isinstance(out, Image.Image) and out.mode == "RGB"
    assert np.array_equal(np.asarray(out), np.repeat(np.asarray(depth)[:, :, None], 3, axis=2))
    pipe = _pipe("depth")
    with pytest.raises(NotImplementedError, match="depth_estimator"):
        pipe.process_condition_image(photo, "depth")
    with pytest.raises(AssertionError):
        pipe.process_condition_image(photo, "seg")


def test_end_to_end_from_a_raw_photo(golden_dir):
    """generate_image on prepare_condition_image(photo) == generate_image on the restatement's edge image built by the same
    three host lines (EDC:1391-1393), same seed: identical final images."""
    from PIL import Image
    photo = Image.open(os.path.join(golden_dir, "canny_input_yoga.jpeg"))
    H, W = 512, 1024
    kw = dict(height=H, width=W, num_inference_steps=3, resampling_steps=2, controlnet_conditioning_scale=0.2, output_type="pt",
              progress=lambda it: it)
    pipe = _pipe()
    cond = pipe.prepare_condition_image(photo, H, W)
    ds = pipe.get_downsample_size(H, W)
    resized = photo.resize((ds[1] * pipe.vae_scale_factor, ds[0] * pipe.vae_scale_factor)).convert("RGB")
    edges = cc.canny(np.asarray(resized))
    assert edges.any() and cond.size == resized.size
    want_cond = Image.fromarray(np.repeat(edges[:, :, None], 3, axis=2))
    assert np.array_equal(np.asarray(cond), np.asarray(want_cond))
    pipe.seed_everything(7)
    got, _ = pipe.generate_image("p", "", cond, **kw)
    pipe = _pipe()
    pipe.seed_everything(7)
    want, _ = pipe.generate_image("p", "", want_cond, **kw)
    assert got.shape == (1, 3, H, W) and torch.equal(got, want)


def _cli(tmp_path, photo_path, process):
    from elasticdiffusion_official_amd.__main__ import main
    return main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1",
                 "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4",
                 "--controlnet_model", "canny", "--condition_image", photo_path, "--process_condition", process])


def test_cli_process_condition(tmp_path, golden_dir):
    """--process_condition true: the file is a raw photo (the reference command line's meaning); false (the default): it is
    the already extracted condition, as before."""
    from PIL import Image
    photo_path = os.path.join(golden_dir, "canny_input_yoga.jpeg")
    save_dir = _cli(tmp_path / "a", photo_path, "true")
    files = {os.path.basename(f) for f in glob.glob(os.path.join(save_dir, "*"))}
    assert {"0.png", "condition.png", "args.txt"} <= files, files
    assert "process_condition: True" in open(os.path.join(save_dir, "args.txt")).read()
    assert Image.open(os.path.join(save_dir, "0.png")).size == (512, 512)
    want = cc.canny(np.asarray(Image.open(photo_path).resize((512, 512)).convert("RGB")))
    cond = np.asarray(Image.open(os.path.join(save_dir, "condition.png")))
    assert cond.shape == (512, 512, 3) and all(np.array_equal(cond[:, :, c], want) for c in range(3))
    processed = np.asarray(Image.open(os.path.join(save_dir, "0.png")))

    save_dir = _cli(tmp_path / "b", photo_path, "false")
    files = {os.path.basename(f) for f in glob.glob(os.path.join(save_dir, "*"))}
    assert "0.png" in files and "condition.png" not in files, files
    assert "process_condition: False" in open(os.path.join(save_dir, "args.txt")).read()
    raw = np.asarray(Image.open(os.path.join(save_dir, "0.png")))
    assert raw.shape == processed.shape and not np.array_equal(raw, processed)      # the photo itself was the condition
