"""-m gpu: the HIP resize kernels (csrc/resize_kernels.hip), ``ops.resize_u8`` and the condition-image methods built on them
against ``PIL.Image.resize`` itself, against the recorded Pillow outputs of tests/golden/g14_resize.npz and against the numpy
restatement (tests/resize_cpu.py).  All arithmetic is integer: every comparison is equality, no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import canny_cpu as cc
from tests import resize_cpu as rc
from tests.fakes import FakeControlNet, FakeUNet, FakeVAE
from tests.test_hip_parity import _embed_fn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


def _pil(img, size, filter):
    return np.asarray(Image.fromarray(img).resize((size[1], size[0]), FILTERS[filter]))


def _gpu(img, size, filter, out="u8"):
    return _ops().resize_u8(torch.from_numpy(img).to(DEV), size, filter, out=out).cpu()


def _cond_of(u8):
    u8 = u8 if u8.ndim == 3 else np.repeat(u8[:, :, None], 3, axis=2)
    return torch.from_numpy(u8).float().div(255).permute(2, 0, 1)[None]


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(14).integers(0, 256, (37, 53, 3), dtype=np.uint8)      # rows of 159 bytes: no row but the first is aligned


@pytest.fixture(scope="module")
def photo(golden_dir):
    return Image.open(os.path.join(golden_dir, "canny_input_yoga.jpeg")).convert("RGB")


# ---------------------------------------------------------------------------------------------------
# ops.resize_u8 == Pillow
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
@pytest.mark.parametrize("size", [(17, 53), (37, 96), (129, 7), (1, 1), (300, 517)])    # columns only, rows only, both
def test_noise_matches_pillow(noise, size, filter):
    got = _gpu(noise, size, filter)
    assert got.dtype == torch.uint8 and tuple(got.shape) == size + (3,)
    assert np.array_equal(got.numpy(), _pil(noise, size, filter))
    assert torch.equal(_gpu(noise, size, filter, out="cond"), _cond_of(got.numpy()))


@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
def test_single_channel_layouts(noise, filter):
    grey = noise[:, :, 0].copy()
    for size in ((17, 53), (37, 96), (129, 7), (1, 1), (300, 517)):
        want = _pil(grey, size, filter)
        flat = _gpu(grey, size, filter)
        assert tuple(flat.shape) == size and np.array_equal(flat.numpy(), want)
        hwc = _gpu(grey[:, :, None].copy(), size, filter)
        assert tuple(hwc.shape) == size + (1,) and np.array_equal(hwc.numpy()[:, :, 0], want)
        assert torch.equal(_gpu(grey, size, filter, out="cond"), _cond_of(want))             # one channel replicated to three planes


def test_recorded_pillow_outputs(golden_dir):
    """The reference does not depend on the Pillow installed here: inputs and outputs recorded by tests/golden/make_resize.py."""
    z = np.load(os.path.join(golden_dir, "g14_resize.npz"))
    outs = [k for k in z.files if k.startswith("out_")]
    assert len(outs) >= 12
    for key in outs:
        _, name, hw, filter = key.split("_")
        H, W = (int(v) for v in hw.split("x"))
        assert np.array_equal(_gpu(z[f"in_{name}"], (H, W), filter).numpy(), z[key]), key


def test_large_reduction_and_the_bounds():
    """200 x 313 -> 5 x 3: ksize far beyond the tile.  8192 taps per output along either axis, and the widest output row."""
    rng = np.random.default_rng(3)
    cases = [(rng.integers(0, 256, (200, 313, 3), dtype=np.uint8), (5, 3)),
             (rng.integers(0, 256, (8192, 1, 1), dtype=np.uint8), (1, 1)),
             (rng.integers(0, 256, (1, 8192, 3), dtype=np.uint8), (1, 1)),
             (rng.integers(0, 256, (2, 2, 3), dtype=np.uint8), (1, 8192))]
    for img, size in cases:
        for filter in FILTERS:
            want = _pil(img[:, :, 0] if img.shape[2] == 1 else img, size, filter).reshape(size + (img.shape[2],))
            assert np.array_equal(rc.resize(img, size, filter), want)
            assert np.array_equal(_gpu(img, size, filter).numpy(), want), (img.shape, size, filter)


def test_clamp_is_exercised():
    img = (np.random.default_rng(0).integers(0, 2, (40, 41, 3)) * 255).astype(np.uint8)
    for size in ((64, 128), (17, 41)):
        want, raws = rc.resize(img, size, "lanczos", unclamped=True)
        assert min(int(r.min()) for _, r in raws) < 0 and max(int(r.max()) for _, r in raws) > 255   # both sides leave [0, 255]
        assert np.array_equal(want, _pil(img, size, "lanczos"))
        assert np.array_equal(_gpu(img, size, "lanczos").numpy(), want)


def test_every_byte_value_as_condition():
    """byte / 255 is the correctly rounded division for all 256 bytes (a multiply by the reciprocal is not)."""
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([ramp, ramp.T, ramp[::-1]], axis=2).copy()
    cond = _gpu(img, (16, 16), "bicubic", out="cond")                                        # same size: a copy into the tensor
    assert torch.equal(cond, _cond_of(img))
    assert torch.equal(_gpu(img, (16, 16), "lanczos"), torch.from_numpy(img))


@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
def test_sample_photo(photo, filter):
    arr = np.array(photo)
    assert arr.shape == (1000, 1000, 3)
    dev = torch.from_numpy(arr).to(DEV)
    ops = _ops()
    for size in ((512, 512), (512, 1024)):
        want = _pil(arr, size, filter)
        got = ops.resize_u8(dev, size, filter)
        assert np.array_equal(got.cpu().numpy(), want), size
        cond = ops.resize_u8(dev, size, filter, out="cond")
        assert cond.is_cuda and torch.equal(cond.cpu(), torch.from_numpy(want).float().div(255).permute(2, 0, 1)[None])
        assert torch.equal(ops.resize_u8(dev, size, filter), got)                            # two launches: bit-identical
    if filter == "bicubic":
        assert np.array_equal(np.asarray(photo.resize((1024, 512))), _pil(arr, (512, 1024), "bicubic"))   # PIL's default filter


def test_rejections_launch_nothing():
    ops = _ops()
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    ops.TIMER.start()
    try:
        for bad in (ok.cpu(), ok.permute(1, 0, 2), ok.float(), ok[:, :, :2].contiguous(),
                    torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV), torch.zeros(0, 8, 3, dtype=torch.uint8, device=DEV),
                    torch.zeros(8193, 1, 1, dtype=torch.uint8, device=DEV), torch.zeros(1, 8193, dtype=torch.uint8, device=DEV)):
            with pytest.raises(RuntimeError):
                ops.resize_u8(bad, (4, 4))
        for size in ((0, 4), (4, 0), (8193, 4), (4, 8193), (4,), 4):
            with pytest.raises(RuntimeError):
                ops.resize_u8(ok, size)
        with pytest.raises(ValueError):
            ops.resize_u8(ok, (4, 4), filter="nearest")
        with pytest.raises(ValueError):
            ops.resize_u8(ok, (4, 4), out="pil")
    finally:
        events = ops.TIMER.stop()
    assert not any(name.startswith("ed_resize") for name in events), events
    assert torch.equal(ops.resize_u8(ok, (4, 5)), torch.zeros(4, 5, 3, dtype=torch.uint8, device=DEV))   # the launch state is clean


def test_entry_points_reject_without_a_launch():
    """The C ABI's own bounds: hipErrorInvalidValue (1) for C outside {1, 3}, an extent outside 1..8192, a destination pitch that is
    not a multiple of 4 or too short, two NULL destinations."""
    from elasticdiffusion_official_amd import _hip, resample
    L = _hip.lib()
    src = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(8, 16, dtype=torch.uint8, device=DEV)
    cond = torch.zeros(1, 3, 4, 8, dtype=torch.float32, device=DEV)
    k, b = (torch.from_numpy(t.copy()).to(DEV) for t in resample.coefficients(8, 4, "bicubic"))
    ks = k.shape[1]
    p = [t.data_ptr() for t in (src, k, b, dst, cond)]
    rows = lambda H=8, W=8, C=3, sp=24, Wo=4, dp=16: L.ed_resize_rows_u8(p[0], H, W, C, sp, p[1], p[2], ks, Wo, p[3], dp, None)  # noqa: E731
    cols = lambda H=8, WC=24, sp=24, Ho=4, C=3, u8=p[3], cd=None: L.ed_resize_cols_u8(p[0], H, WC, sp, p[1], p[2], ks, Ho, C, u8, cd, None)  # noqa: E731
    assert rows() == 0 and cols() == 0 and cols(u8=None, cd=p[4]) == 0
    for bad in (rows(C=2), rows(C=4), rows(H=0), rows(H=8193), rows(W=0), rows(Wo=0), rows(Wo=8193), rows(sp=23), rows(dp=15),
                rows(dp=8), cols(C=2), cols(H=0), cols(Ho=0), cols(Ho=8193), cols(WC=0), cols(WC=25), cols(WC=3 * 8193, sp=3 * 8193),
                cols(sp=23), cols(u8=None, cd=None)):
        assert bad == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# prepare_condition_image / _to_condition_tensor / generate_image
# ---------------------------------------------------------------------------------------------------
def _pipe(model="canny", **kw):
    from elasticdiffusion_official_amd import ElasticDiffusionControlNet
    return ElasticDiffusionControlNet(DEV, "1.5", model, view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(),
                                      text_encoder=_embed_fn(False), controlnet=FakeControlNet(), **kw)


def _no_host_resize(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("PIL.Image.resize called: the resize must run on the device")
    monkeypatch.setattr(Image.Image, "resize", boom)


def test_prepare_condition_image_resizes_on_the_device(photo, monkeypatch):
    """Fails without the feature: the parent resizes with PIL on the host."""
    H, W = 512, 1024
    pipe = _pipe()
    ds = pipe.get_downsample_size(H, W)
    h_px, w_px = ds[0] * pipe.vae_scale_factor, ds[1] * pipe.vae_scale_factor
    host = photo.resize((w_px, h_px)).convert("RGB")                       # the parent's three lines, recorded before the patch
    want = np.repeat(cc.canny(np.asarray(host))[:, :, None], 3, axis=2)
    want_grey = cc.canny(np.asarray(photo.convert("L").resize((w_px, h_px)).convert("RGB")))
    assert want.any()
    _no_host_resize(monkeypatch)
    out = pipe.prepare_condition_image(photo, H, W)
    assert out.mode == "RGB" and out.size == (w_px, h_px) and np.array_equal(np.asarray(out), want)
    pt = pipe.prepare_condition_image(photo, H, W, output_type="pt")
    assert pt.is_cuda and pt.dtype == torch.float32 and torch.equal(pt.cpu(), pipe._to_condition_tensor(out, h_px, w_px))
    for same in (np.asarray(photo), torch.from_numpy(np.asarray(photo).copy()), torch.from_numpy(np.asarray(photo).copy()).to(DEV)):
        assert np.array_equal(np.asarray(pipe.prepare_condition_image(same, H, W)), want)    # array / host tensor / device tensor
    assert np.array_equal(np.asarray(pipe.prepare_condition_image(photo.convert("L"), H, W))[:, :, 0], want_grey)
    with pytest.raises(ValueError):
        pipe.prepare_condition_image(photo, H, W, output_type="np")


def test_depth_estimator_still_receives_a_pil_image(photo, monkeypatch):
    small = photo.crop((0, 0, 200, 120))
    pipe = _pipe("depth", depth_estimator=lambda image: calls.append(image) or {"depth": image.convert("L")})
    calls = []
    ds = pipe.get_downsample_size(512, 512)
    size = (ds[1] * pipe.vae_scale_factor, ds[0] * pipe.vae_scale_factor)
    host = small.resize(size).convert("RGB")
    _no_host_resize(monkeypatch)
    out = pipe.prepare_condition_image(small, 512, 512)
    assert len(calls) == 1 and isinstance(calls[0], Image.Image) and calls[0].mode == "RGB"
    assert np.array_equal(np.asarray(calls[0]), np.asarray(host))
    assert np.array_equal(np.asarray(out), np.repeat(np.asarray(host.convert("L"))[:, :, None], 3, axis=2))


def test_wrong_sized_condition_is_resized_on_the_device(photo, monkeypatch):
    """generate_image(condition_image=<PIL of the photo's size>) == generate_image on the PIL-Lanczos-resized image."""
    H, W = 512, 512
    kw = dict(height=H, width=W, num_inference_steps=2, resampling_steps=1, controlnet_conditioning_scale=0.2, output_type="pt",
              progress=lambda it: it)
    pipe = _pipe()
    ds = pipe.get_downsample_size(H, W)
    h_px, w_px = ds[0] * pipe.vae_scale_factor, ds[1] * pipe.vae_scale_factor
    assert photo.size != (w_px, h_px)
    resized = photo.resize((w_px, h_px), resample=Image.LANCZOS)
    want_cond = pipe._to_condition_tensor(resized, h_px, w_px)                 # right size: today's host conversion
    pipe.seed_everything(5)
    want, _ = pipe.generate_image("p", "", resized, **kw)
    grey_want = pipe._to_condition_tensor(photo.convert("L").resize((w_px, h_px), resample=Image.LANCZOS).convert("RGB"), h_px, w_px)
    _no_host_resize(monkeypatch)
    got_cond = pipe._to_condition_tensor(photo, h_px, w_px)
    assert got_cond.is_cuda and torch.equal(got_cond.cpu(), want_cond)
    assert torch.equal(pipe._to_condition_tensor(np.asarray(photo), h_px, w_px).cpu(), want_cond)       # HWC uint8 array
    assert torch.equal(pipe._to_condition_tensor(photo.convert("L"), h_px, w_px).cpu(), grey_want)
    pipe = _pipe()
    pipe.seed_everything(5)
    got, _ = pipe.generate_image("p", "", photo, **kw)
    assert got.shape == (1, 3, H, W) and torch.equal(got, want)


def test_other_modes_stay_on_the_host_path(photo, monkeypatch):
    """RGBA (resampled premultiplied by Pillow) and P (nearest) are outside the kernels' scope: today's code, today's results."""
    ops = _ops()
    small = photo.crop((300, 200, 620, 440))
    rgba = small.copy()
    rgba.putalpha(small.convert("L"))
    pal = small.convert("P")
    pipe = _pipe()
    H, W = 512, 512
    ds = pipe.get_downsample_size(H, W)
    h_px, w_px = ds[0] * pipe.vae_scale_factor, ds[1] * pipe.vae_scale_factor

    def boom(*a, **k):
        raise AssertionError("ops.resize_u8 called for a mode Pillow does not resample per channel")
    monkeypatch.setattr(ops, "resize_u8", boom)
    for img in (rgba, pal):
        want = cc.canny(np.asarray(img.resize((w_px, h_px)).convert("RGB")))
        assert np.array_equal(np.asarray(pipe.prepare_condition_image(img, H, W))[:, :, 0], want), img.mode
        host = np.asarray(img.convert("RGB").resize((w_px, h_px), resample=Image.LANCZOS))
        want_t = torch.from_numpy(host.copy()).float().div(255.0).permute(2, 0, 1)[None]
        assert torch.equal(pipe._to_condition_tensor(img, h_px, w_px), want_t), img.mode
    right = small.resize((w_px, h_px))                                          # the right size already: no resize of either kind
    assert torch.equal(pipe._to_condition_tensor(right, h_px, w_px),
                       torch.from_numpy(np.asarray(right).copy()).float().div(255.0).permute(2, 0, 1)[None])
