"""-m gpu: soft-edged inpainting through the HIP path.

Bars:
  * every kernel against the restatement of tests/soft_inpaint_cpu.py (itself held to Pillow / numpy in tests/test_soft_inpaint.py):
    BIT-EXACT, wide and scalar paths alike; the blur also against Pillow directly;
  * end-to-end latents against ``SoftInpaintOracle``: the project's rel-L2 < 1e-4 and an identical host RNG end state;
  * the level-0 region of a graded run equals ``pipe.last_init_latents`` bit for bit; a 0 / 255 mask in graded mode is the binary
    run bit for bit; a graded image costs the launches of a binary one;
  * interleaved vs alone 1e-5; without the keywords the loop launches and computes what it did;
  * ``composite=True`` gives the bytes of ``Image.composite`` on the same call's decode.
"""
import os

import numpy as np
import pytest
import torch

from tests import ddim_variants as V
from tests import img2img_cpu as I
from tests import soft_inpaint_cpu as S
from tests.fakes import synthetic_text_embeds
from tests.golden import cases
from tests.test_hip_parity import DEV, rel_l2
from tests.test_img2img import half_mask, synthetic_image
from tests.test_img2img_gpu import EPS, LATENT_SHAPES, _inputs, _loop_kw, _misaligned, _oracle_run, _pipe
from tests.test_scheduler_variants_gpu import V_TRAILING_ZSNR, _schedules
from tests.test_soft_inpaint import block_mask, noise_mask, ramp_mask

pytestmark = pytest.mark.gpu

NAME = "cfg2_sd_512x1024"
NEW_ENTRY_POINTS = ("ed_box_blur3_rows_u8", "ed_box_blur3_cols_u8", "ed_mask_levels_to_latent", "ed_inpaint_blend_level",
                    "ed_composite_u8", "ed_canvas_pad_u8")


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------
# the blur
# ---------------------------------------------------------------------------------------------------
BLUR_SHAPES = [(1, 1), (5, 300), (300, 5), (37, 53), (64, 128)]
BLUR_RADII = [0.5, 3.3, 8, 33]


@pytest.mark.parametrize("H,W", BLUR_SHAPES)
def test_gaussian_blur_bit_exact(H, W):
    """widths that are no multiple of 4 (byte staging), lines shorter than the window in either direction (5 x 300, 300 x 5 from
    radius 3.3 up; 1 x 1), more than one column strip (37 x 53: 7 strips, the last one partial; 64 x 128: 16), r = 0."""
    from PIL import Image, ImageFilter
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    strip = _hip.lib().ed_box_blur3_cols_strip(H, W)
    assert strip == 8 and ((W + strip - 1) // strip > 1) == (W > 8)
    for img in (noise_mask(H, W), block_mask(H, W)):
        dev = torch.from_numpy(img).to(DEV)
        for radius in BLUR_RADII:
            want = S.gaussian_blur(img, radius)
            got = ops.gaussian_blur_u8(dev, radius)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (H, W, radius)
            assert np.array_equal(got.cpu().numpy(), np.array(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius))))
        assert torch.equal(dev.cpu(), torch.from_numpy(img))                                   # the source is left alone
        # [H,W,1], and a view that starts one byte past a 16-byte boundary: byte staging, the same bytes
        assert torch.equal(ops.gaussian_blur_u8(dev.view(H, W, 1), 3.3).view(H, W).cpu(), torch.from_numpy(S.gaussian_blur(img, 3.3)))
        assert torch.equal(ops.gaussian_blur_u8(_misaligned(torch.from_numpy(img)), 8).cpu(), torch.from_numpy(S.gaussian_blur(img, 8)))
    assert torch.equal(ops.gaussian_blur_u8(dev, 0.0), dev)                                    # radius 0: the identity


@pytest.mark.parametrize("H,W,strip,radius", [(16, 12, 8, 3.3), (8, 4096, 16, 8), (4, 8192, 32, 33), (8192, 8, 4, 8)])
def test_gaussian_blur_every_strip_width(H, W, strip, radius):
    """the sizes at which the column launch takes another strip width: 8 (a partial last strip on a width that is a multiple
    of 4), 16 and 32 (wide images), and 4 at the largest height, where the two buffers of a strip fill the 64 KiB of LDS"""
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    assert _hip.lib().ed_box_blur3_cols_strip(H, W) == strip
    img = noise_mask(H, W)
    assert torch.equal(ops.gaussian_blur_u8(torch.from_numpy(img).to(DEV), radius).cpu(), torch.from_numpy(S.gaussian_blur(img, radius)))


# ---------------------------------------------------------------------------------------------------
# the level map and the graded blend
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(104, 152), (64, 64)])
def test_mask_levels_to_latent_exact(H, W):
    ops = _ops()
    m = noise_mask(H, W)
    want = S.level_map(m, 8)
    assert not torch.equal(want, S.level_map(np.roll(m, (-4, -4), (0, 1)), 8)) and len(want.unique()) > 30
    t = torch.from_numpy(m)
    got = ops.mask_levels_to_latent(t.to(DEV), 8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H // 8, W // 8)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.mask_levels_to_latent(t.view(H, W, 1).to(DEV), 8).cpu(), want)
    assert torch.equal(ops.mask_levels_to_latent(_misaligned(t), 8).cpu(), want)
    # a map that is already at latent resolution is copied; a bool one is 0 / 255
    lat = want.to(DEV)
    assert torch.equal(ops.mask_levels_to_latent(lat, 1), lat)
    assert torch.equal(ops.mask_levels_to_latent(lat >= 128, 1).cpu(), (want >= 128).to(torch.uint8) * 255)


def _levels(Hl, Wl, thr, seed):
    """the four levels 0, thr, thr + 1, 255 in random places, each present (also in every byte lane of the 4-wide kernel)"""
    vals = torch.tensor([0, thr, thr + 1, 255], dtype=torch.uint8)
    g = torch.Generator().manual_seed(seed)
    lv = vals[torch.randint(0, 4, (Hl, Wl), generator=g)]
    lv.view(-1)[:16] = vals.repeat_interleave(4)[torch.tensor([0, 4, 8, 12, 13, 1, 5, 9, 10, 14, 2, 6, 7, 11, 15, 3])]
    assert set(vals.tolist()) <= set(lv.unique().tolist())
    return lv


@pytest.mark.parametrize("thr", [0, 63, 254])
@pytest.mark.parametrize("shape", LATENT_SHAPES)
def test_inpaint_blend_level_bit_exact(shape, thr):
    ops = _ops()
    sch, _, ts = _schedules(EPS, 50)
    a, b = sch.add_noise_coefficients(ts[17])
    g = torch.Generator().manual_seed(sum(shape) + thr)
    x, z0, noise = (torch.randn(shape, generator=g) for _ in range(3))
    x_d, z0_d, n_d = x.to(DEV), z0.to(DEV), noise.to(DEV)
    lv = _levels(shape[2], shape[3], thr, sum(shape))
    lv_d = lv.to(DEV)
    want = S.blend_level(x, lv, thr, z0, noise, torch.tensor(a), torch.tensor(b), clean=False)
    held = (lv <= thr).expand(shape)
    assert torch.equal(want[~held], x[~held]) and 0 < int(held.sum()) < held.numel()
    out = torch.empty(shape, device=DEV)
    ops.inpaint_blend_level(x_d, lv_d, thr, z0_d, n_d, a, b, out=out)                      # out of place
    assert torch.equal(out.cpu(), want)
    inplace = x_d.clone()
    assert ops.inpaint_blend_level(inplace, lv_d, thr, z0_d, n_d, a, b) is inplace         # in place
    assert torch.equal(inplace, out)
    # the binary kernel on the thresholded map: the same bits (the rule is the binary one with level > thr as the mask)
    assert torch.equal(ops.inpaint_blend(x_d, (lv_d > thr).to(torch.uint8), z0_d, n_d, a, b, out=torch.empty_like(out)), out)
    # the scalar kernel (misaligned buffers / a misaligned level map): the same bits, out of place and in place
    xm, om = _misaligned(x), _misaligned(torch.zeros(shape))
    ops.inpaint_blend_level(xm, lv_d, thr, _misaligned(z0), _misaligned(noise), a, b, out=om)
    assert torch.equal(om, out)
    ops.inpaint_blend_level(xm, _misaligned(lv), thr, z0_d, n_d, a, b)
    assert torch.equal(xm, out)
    # clean: z0 itself where held, also when the noise holds inf (a select); the noise may be absent
    inf_noise = torch.full(shape, float("inf"))
    want_c = S.blend_level(x, lv, thr, z0, inf_noise, 1.0, 0.0, clean=True)
    assert bool(torch.isfinite(want_c).all()) and torch.equal(want_c[held], z0[held])
    for nz in (inf_noise.to(DEV), None):
        oc = torch.empty(shape, device=DEV)
        ops.inpaint_blend_level(x_d, lv_d, thr, z0_d, nz, 1.0, 0.0, out=oc, clean=True)
        assert torch.equal(oc.cpu(), want_c)
    # ... and an inf on the side that is not taken does not leak in the noised blend either
    nz = n_d.clone()
    nz[(lv_d > thr).expand(shape)] = float("inf")
    o2 = torch.empty(shape, device=DEV)
    ops.inpaint_blend_level(x_d, lv_d, thr, z0_d, nz, a, b, out=o2)
    assert torch.equal(o2, out)


# ---------------------------------------------------------------------------------------------------
# the composite and the canvas
# ---------------------------------------------------------------------------------------------------
def test_composite_every_byte_triple():
    """all 256^3 (decoded byte, init byte, mask byte) triples on a 4096 x 1368 RGB picture (the 4-pixel kernel): the mask byte is
    the pixel index mod 256, (decoded byte, init byte) count through the 65536 pairs over the pixels of one mask value and the
    three channels.  The decoded value of byte u is (u + 0.5) / 255, whose product with 255 truncates to u."""
    ops = _ops()
    H, W = 4096, 1368
    p = torch.arange(H * W, dtype=torch.int64)
    m = (p % 256).to(torch.uint8).view(H, W)
    q = (p // 256)[:, None] * 3 + torch.arange(3)[None]                    # [HW, 3]
    assert int(q.max()) >= 65535
    u, init = (q % 256).to(torch.uint8), ((q // 256) % 256).to(torch.uint8).view(H, W, 3).contiguous()
    decoded = ((u.float() + 0.5) / 255).t().contiguous().view(1, 3, H, W)
    assert torch.equal(S.to_bytes(decoded).view(3, -1).t(), u)
    want = S.composite(decoded, init.numpy(), m.numpy())
    got = ops.composite_u8(decoded.to(DEV), init.to(DEV), m.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("H,W", [(13, 19), (64, 128)])
def test_composite_rgb_and_the_truncation(H, W):
    """13 x 19: the scalar kernel; 64 x 128: four pixels per thread.  Decoded values that are exactly k / 255 and the float just
    below pin the conversion to the truncated fp32 product (a rounding conversion, or a division-free k, gives other bytes)."""
    from PIL import Image
    ops = _ops()
    g = torch.Generator().manual_seed(H)
    k = torch.randint(0, 256, (1, 3, H, W), generator=g)
    k.view(-1)[:256] = torch.arange(256)
    exact = k.float() / 255
    below = torch.nextafter(exact, torch.tensor(-1.0)).clamp(min=0)
    init, m = synthetic_image(H, W, seed=H), noise_mask(H, W)
    m[0, :4] = (0, 255, 1, 254)
    init_d, m_d = torch.from_numpy(init).to(DEV), torch.from_numpy(m).to(DEV)
    for decoded in (exact, below, torch.rand(1, 3, H, W, generator=g)):
        want = S.composite(decoded, init, m)
        got = ops.composite_u8(decoded.to(DEV), init_d, m_d)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        pil = Image.composite(Image.fromarray(S.to_bytes(decoded)[0].permute(1, 2, 0).numpy()), Image.fromarray(init), Image.fromarray(m))
        assert np.array_equal(got.cpu().numpy(), np.array(pil))
        # misaligned buffers: the scalar kernel, the same bytes; a [H,W,1] mask
        got2 = ops.composite_u8(_misaligned(decoded), _misaligned(torch.from_numpy(init)), _misaligned(torch.from_numpy(m)))
        assert torch.equal(got2, got)
        assert torch.equal(ops.composite_u8(decoded.to(DEV), init_d, m_d.view(H, W, 1)), got)
    assert not torch.equal(S.to_bytes(exact), S.to_bytes(below))
    keep = torch.from_numpy(m == 0)
    assert torch.equal(got.cpu()[keep], torch.from_numpy(init)[keep])


def test_canvas_pad_exact():
    ops = _ops()
    img = synthetic_image(13, 19, seed=2)
    for pads in ((0, 0, 0, 0), (3, 0, 0, 0), (0, 5, 0, 2), (4, 1, 7, 9)):
        want_c, want_m = S.canvas_pad(img, *pads)
        for src in (torch.from_numpy(img).to(DEV), _misaligned(torch.from_numpy(img))):
            canvas, mask = ops.canvas_pad_u8(src, *pads)
            assert canvas.dtype == mask.dtype == torch.uint8
            assert torch.equal(canvas.cpu(), torch.from_numpy(np.ascontiguousarray(want_c))) and torch.equal(mask.cpu(), torch.from_numpy(want_m))


def test_rejections_leave_the_launch_state_clean():
    ops = _ops()
    a = torch.zeros(1, 4, 8, 8, device=DEV)
    lv = torch.zeros(8, 8, dtype=torch.uint8, device=DEV)
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    dec = torch.zeros(1, 3, 8, 8, device=DEV)
    for call in (lambda: ops.gaussian_blur_u8(lv.cpu(), 2.0), lambda: ops.mask_levels_to_latent(lv.cpu(), 1),
                 lambda: ops.inpaint_blend_level(a.cpu(), lv, 0, a, a, 1.0, 0.0), lambda: ops.composite_u8(dec.cpu(), img, lv),
                 lambda: ops.composite_u8(dec, img.cpu(), lv), lambda: ops.canvas_pad_u8(img.cpu(), 1, 1, 1, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="uint8"):
        ops.gaussian_blur_u8(lv.float(), 2.0)
    with pytest.raises(RuntimeError, match=r"\[H,W\]"):
        ops.gaussian_blur_u8(img, 2.0)
    for bad in (ops.MASK_BLUR_MAX + 1, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="radius"):
            ops.gaussian_blur_u8(lv, bad)
    with pytest.raises(RuntimeError, match="multiple of scale"):
        ops.mask_levels_to_latent(torch.ones(12, 16, dtype=torch.uint8, device=DEV), 8)
    with pytest.raises(RuntimeError, match="uint8 or bool"):
        ops.mask_levels_to_latent(lv.float(), 1)
    with pytest.raises(RuntimeError, match="level must be uint8"):
        ops.inpaint_blend_level(a, lv.bool(), 0, a, a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="level must be"):
        ops.inpaint_blend_level(a, lv[:4].contiguous(), 0, a, a, 1.0, 0.0)
    for bad in (-1, 256, 1.5):
        with pytest.raises(RuntimeError, match="thr"):
            ops.inpaint_blend_level(a, lv, bad, a, a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="shape"):
        ops.inpaint_blend_level(a, lv, 0, a[:, :2].contiguous(), a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="noise is required"):
        ops.inpaint_blend_level(a, lv, 0, a, None, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.composite_u8(dec.half(), img, lv)
    with pytest.raises(RuntimeError, match=r"\[1,3,H,W\]"):
        ops.composite_u8(a, img, lv)
    with pytest.raises(RuntimeError, match="init must be"):
        ops.composite_u8(dec, img[:4].contiguous(), lv)
    with pytest.raises(RuntimeError, match="mask must be"):
        ops.composite_u8(dec, img, lv[:4].contiguous())
    with pytest.raises(RuntimeError, match=r"\[H,W,3\]"):
        ops.canvas_pad_u8(lv, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="borders"):
        ops.canvas_pad_u8(img, 1, -1, 1, 1)
    with pytest.raises(RuntimeError, match="sides"):
        ops.canvas_pad_u8(img, ops.RESIZE_MAX_DIM, 0, 0, 0)
    assert ops._LAUNCH["device"] is None
    out = torch.empty_like(a)
    ops.inpaint_blend_level(a + 1, lv + 1, 0, a, a, 1.0, 0.0, out=out)      # the launch state is clean again
    assert torch.equal(out, a + 1)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
BLUR = 12.0


def soft_block_mask(H, W):
    """0 / 255: a white block in the right half, the left third black far beyond the reach of the blur (level 0 survives)"""
    m = np.zeros((H, W), np.uint8)
    m[H // 4: 3 * H // 4, W // 2: 7 * W // 8] = 255
    return m


_ORACLE = {}


def _soft_oracle_run(name, sched_kw, strength, gr, mask_blur=BLUR, mask_mode="graded"):
    """The CPU restatement's (latent, RNG tail, z0, level map, pixel mask) for one case, computed once and shared."""
    from tests import ddim_variants as V
    from tests.fakes import FakeUNet, FakeVAE
    key = (name, tuple(sorted(sched_kw.items())), strength, gr, mask_blur, mask_mode)
    if key not in _ORACLE:
        c = cases.E2E_CASES[name]
        orc = S.SoftInpaintOracle(FakeUNet(c["sample"]), FakeVAE(), V.DDIMVariants(**sched_kw), V.embed_fn(False), sd_version=c["sd"],
                                  view_batch_size=c["vbs"])
        img = synthetic_image(c["H"], c["W"], seed=c["seed"])
        orc.seed_everything(c["seed"])
        z = orc.generate_latent("p", "", **_loop_kw(name), guidance_rescale=gr, init_image=img, strength=strength,
                                mask_image=soft_block_mask(c["H"], c["W"]), mask_blur=mask_blur, mask_mode=mask_mode)
        _ORACLE[key] = (z, torch.rand(4), orc.last_init_latents, orc.last_levels, orc.last_pixel_mask)
    return _ORACLE[key]


E2E = [
    (NAME, EPS, 1.0, 0.0),                        # 64x128 latent, padded global pass, RePaint on
    (NAME, EPS, 0.5, 0.0),                        # the last 2 of 4 steps: the absolute j in thr(j)
    (NAME, V_TRAILING_ZSNR, 1.0, 0.7),            # a = 0 at the first timestep, guidance rescale on
]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,sched_kw,strength,gr", E2E)
def test_end_to_end_graded_vs_cpu_restatement(name, sched_kw, strength, gr, fused):
    from elasticdiffusion_official_amd import ops, pipeline
    want, otail, oz0, olevel, opix = _soft_oracle_run(name, sched_kw, strength, gr)
    c = cases.E2E_CASES[name]
    img, mask = synthetic_image(c["H"], c["W"], seed=c["seed"]), soft_block_mask(c["H"], c["W"])
    assert int((olevel == 0).sum()) > 0 and int((olevel == 255).sum()) > 0 and len(olevel.unique()) > 8
    pipeline.FUSED_GLUE = fused
    counts = {}
    try:
        for mode in ("graded", "binary"):
            pipe = _pipe(name, sched_kw)
            pipe.seed_everything(c["seed"])
            ops.TIMER.start()
            try:
                z_mode = pipe.generate_latents("p", "", **_loop_kw(name), guidance_rescale=gr, init_image=img, strength=strength,
                                               mask_image=mask, mask_blur=BLUR, mask_mode=mode).cpu()
            finally:
                counts[mode] = {k: v[0] for k, v in ops.TIMER.stop().items()}
            if mode == "graded":
                z, tail, z0 = z_mode, torch.rand(4), pipe.last_init_latents.cpu()
                assert torch.equal(pipe.last_pixel_mask.cpu(), torch.from_numpy(opix))          # the blurred bytes, Pillow's
                assert torch.equal(pipe.last_init_pixels.cpu(), torch.from_numpy(img))
    finally:
        pipeline.FUSED_GLUE = True
    err = rel_l2(z, want)
    print(f"{name} {sorted(sched_kw)} strength={strength} gr={gr} fused={fused}: rel-L2 {err:.3e}, z0 rel-L2 {rel_l2(z0, oz0):.3e}")
    assert bool(torch.isfinite(z).all())
    assert err < 1e-4, err
    assert torch.equal(tail, otail)
    assert rel_l2(z0, oz0) < 1e-5
    keep = (olevel == 0).expand_as(z)
    assert torch.equal(z[keep], z0[keep])                                     # level 0: the init latent bit for bit
    assert bool((z[~keep] != z0[~keep]).any()) and rel_l2(z, z_mode) > 1e-3   # and the grey levels are not the binary run
    # one blend per phase in either mode: a graded image costs the launches of a binary one
    T = c["steps"]
    n = T - I.window(T, strength)
    two_phase = sum(1 for i in range(T - n, T) if i < T - 1)
    g, b = counts["graded"], counts["binary"]
    assert g["ed_inpaint_blend_level"] == n + two_phase == b["ed_inpaint_blend"]
    assert "ed_inpaint_blend" not in g and "ed_inpaint_blend_level" not in b
    assert g["ed_mask_levels_to_latent"] == 1 == b["ed_mask_to_latent"] and "ed_mask_to_latent" not in g
    assert g["ed_box_blur3_rows_u8"] == g["ed_box_blur3_cols_u8"] == 1 == b["ed_box_blur3_rows_u8"] == b["ed_box_blur3_cols_u8"]
    rename = {"ed_inpaint_blend_level": "ed_inpaint_blend", "ed_mask_levels_to_latent": "ed_mask_to_latent"}
    assert {rename.get(k, k): v for k, v in g.items()} == b


def test_binary_mode_on_the_blurred_mask_vs_cpu_restatement():
    """``mask_blur`` with the default mode: the existing rule (>= 128) on the blurred bytes"""
    want, otail, _, _, opix = _soft_oracle_run(NAME, EPS, 1.0, 0.0, mask_mode="binary")
    c = cases.E2E_CASES[NAME]
    pipe = _pipe(NAME)
    pipe.seed_everything(c["seed"])
    z = pipe.generate_latents("p", "", **_loop_kw(NAME), init_image=synthetic_image(c["H"], c["W"], seed=c["seed"]),
                              mask_image=soft_block_mask(c["H"], c["W"]), mask_blur=BLUR).cpu()
    assert rel_l2(z, want) < 1e-4 and torch.equal(torch.rand(4), otail)
    keep = torch.from_numpy(opix[::8, ::8] < 128).expand_as(z)
    assert torch.equal(z[keep], pipe.last_init_latents.cpu()[keep])


def test_graded_on_a_0_255_mask_is_binary_bit_for_bit():
    img, mask = _inputs(NAME, True)
    lat = {}
    for label, extra in (("binary", {}), ("graded", dict(mask_mode="graded")),
                         ("graded_bool", dict(mask_mode="graded", mask_image=I.latent_mask(mask, 8).bool())),
                         ("graded_levels", dict(mask_mode="graded", mask_image=I.latent_mask(mask, 8) * 255))):
        pipe = _pipe(NAME)
        pipe.seed_everything(cases.E2E_CASES[NAME]["seed"])
        lat[label] = pipe.generate_latents("p", "", **_loop_kw(NAME), **dict(dict(init_image=img, strength=0.5, mask_image=mask), **extra))
        lat[label + "_tail"] = torch.rand(4)
    for label in ("graded", "graded_bool", "graded_levels"):
        assert torch.equal(lat[label], lat["binary"]), label
        assert torch.equal(lat[label + "_tail"], lat["binary_tail"])
    assert rel_l2(lat["binary"], _oracle_run(NAME, EPS, 0.5, True, 0.0)[0]) < 1e-4


def test_absent_keywords_are_the_loop_as_it_was_and_the_keywords_are_not_ignored():
    from elasticdiffusion_official_amd import ops
    seed, steps = cases.E2E_CASES[NAME]["seed"], cases.E2E_CASES[NAME]["steps"]
    img, mask = _inputs(NAME, True)
    lat, counts = {}, {}
    runs = (("omitted", {}), ("defaults", dict(mask_blur=0.0, mask_mode="binary")),
            ("masked", dict(init_image=img, mask_image=mask)),
            ("masked_defaults", dict(init_image=img, mask_image=mask, mask_blur=0.0, mask_mode="binary")),
            ("on", dict(init_image=img, mask_image=mask, mask_blur=BLUR, mask_mode="graded")))
    for label, extra in runs:
        pipe = _pipe(NAME)
        pipe.seed_everything(seed)
        ops.TIMER.start()
        try:
            lat[label] = pipe.generate_latents("p", "", **_loop_kw(NAME), **extra).cpu()
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
        if label in ("omitted", "defaults"):
            assert pipe.last_pixel_mask is None and pipe.last_init_pixels is None
    assert torch.equal(lat["omitted"], lat["defaults"]) and counts["omitted"] == counts["defaults"]
    assert torch.equal(lat["masked"], lat["masked_defaults"]) and counts["masked"] == counts["masked_defaults"]
    phases = 2 * steps - 1
    glue = {k: v for k, v in counts["omitted"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k}
    assert glue == {"ed_assemble_rows": phases, "ed_phase_epilogue": phases, "ed_undo_step": steps - 1}, counts["omitted"]
    # the masked run of the parent commit: its launches and, against its restatement, its latents
    assert rel_l2(lat["masked"], _oracle_run(NAME, EPS, 1.0, True, 0.0)[0]) < 1e-4
    assert counts["masked"]["ed_inpaint_blend"] == phases and counts["masked"]["ed_mask_to_latent"] == 1
    added = {k: v for k, v in counts["masked"].items() if k not in counts["omitted"]}
    assert added == {"ed_u8_to_vae_input": 1, "ed_img2img_init": 1, "ed_mask_to_latent": 1, "ed_inpaint_blend": phases}, added
    for label in ("omitted", "masked"):
        assert not any(k in counts[label] for k in NEW_ENTRY_POINTS)
    assert rel_l2(lat["on"], lat["masked"]) > 1e-3
    assert counts["on"]["ed_inpaint_blend_level"] == phases and "ed_inpaint_blend" not in counts["on"]


def test_interleaved_two_jobs_match_each_alone():
    kw = _loop_kw(NAME)
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"], seed=c["seed"]), soft_block_mask(c["H"], c["W"])

    def embed(prompts):  # stateless (the programs' calls interleave); the values V.embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe(NAME, text_encoder=embed)
    jobs = [dict(prompts="p", negative_prompts="", seed=c["seed"], init_image=img, mask_image=mask, mask_blur=BLUR, mask_mode="graded"),
            dict(prompts="p", negative_prompts="", seed=11, init_image=img, mask_image=half_mask(c["H"], c["W"])),
            dict(prompts="p", negative_prompts="", seed=12)]
    alone = []
    for job in jobs:
        pipe.seed_everything(job["seed"])
        extra = {k: v for k, v in job.items() if k not in ("prompts", "negative_prompts", "seed")}
        alone.append(pipe.generate_latents("p", "", **kw, **extra).clone())
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], _soft_oracle_run(NAME, EPS, 1.0, 0.0)[0]) < 1e-4
    with pytest.raises(ValueError, match="mask_image"):
        pipe.generate_latents_interleaved([dict(prompts="p", seed=1, init_image=img, mask_mode="graded")], in_flight=1, **kw)


def test_pipeline_rejects_bad_arguments_before_any_launch():
    from elasticdiffusion_official_amd import ops
    pipe = _pipe(NAME)
    kw = _loop_kw(NAME)
    img, mask = _inputs(NAME, True)
    ops.TIMER.start()
    try:
        for call in (pipe.generate_latents, pipe.generate_image):
            with pytest.raises(ValueError, match="mask_image"):
                call("p", "", **kw, init_image=img, mask_blur=4.0)
            with pytest.raises(ValueError, match="mask_image"):
                call("p", "", **kw, init_image=img, mask_mode="graded")
            with pytest.raises(ValueError, match="mask_blur"):
                call("p", "", **kw, init_image=img, mask_image=mask, mask_blur=ops.MASK_BLUR_MAX + 1)
            with pytest.raises(ValueError, match="mask_mode"):
                call("p", "", **kw, init_image=img, mask_image=mask, mask_mode="soft")
            with pytest.raises(ValueError, match="8-bit picture mask"):
                call("p", "", **kw, init_image=img, mask_image=I.latent_mask(mask, 8), mask_blur=4.0)
        with pytest.raises(ValueError, match="mask_image"):
            pipe.generate_image("p", "", **kw, init_image=img, composite=True)
        with pytest.raises(ValueError, match="output_type"):
            pipe.generate_image("p", "", **kw, init_image=img, mask_image=mask, composite=True, output_type="pt")
        with pytest.raises(ValueError, match="grid"):
            pipe.generate_image("p", "", **kw, init_image=img, mask_image=mask, composite=True, grid=True)
        with pytest.raises(ValueError, match="8-bit init_image"):
            pipe.generate_image("p", "", **kw, init_image=torch.zeros(1, 3, 512, 1024), mask_image=mask, composite=True)
    finally:
        assert ops.TIMER.stop() == {}


# ---------------------------------------------------------------------------------------------------
# generate_image(composite=True), the canvas helper, the command line
# ---------------------------------------------------------------------------------------------------
def test_generate_image_composite_is_pillows_composite_of_the_same_decode():
    from PIL import Image
    from elasticdiffusion_official_amd import ops
    c = cases.E2E_CASES[NAME]
    img, mask = synthetic_image(c["H"], c["W"], seed=c["seed"]), soft_block_mask(c["H"], c["W"])
    kw = dict(_loop_kw(NAME), init_image=img, mask_image=mask, mask_blur=BLUR, mask_mode="graded", progress=lambda it: it)
    pipe = _pipe(NAME, text_encoder=V.embed_fn(False, B=2))       # two prompts: one composited image per prompt
    pipe.seed_everything(4)
    decoded, _ = pipe.generate_image(["p", "q"], "", **kw, output_type="pt")
    assert tuple(decoded.shape) == (2, 3, c["H"], c["W"])
    pipe.seed_everything(4)
    ops.TIMER.start()
    try:
        pils, _ = pipe.generate_image(["p", "q"], "", **kw, composite=True)
    finally:
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    assert counts["ed_composite_u8"] == 2 and len(pils) == 2
    init, m = pipe.last_init_pixels.cpu().numpy(), pipe.last_pixel_mask.cpu().numpy()
    assert np.array_equal(init, img) and np.array_equal(m, S.gaussian_blur(mask, BLUR))
    assert int((m == 0).sum()) > 0 and int((m == 255).sum()) > 0 and len(np.unique(m)) > 100
    for i, pil in enumerate(pils):
        u = decoded[i].float().mul(255).byte().permute(1, 2, 0).cpu().numpy()
        want = np.array(Image.composite(Image.fromarray(u), Image.fromarray(init), Image.fromarray(m)))
        got = np.array(pil)
        assert got.shape == (c["H"], c["W"], 3) and np.array_equal(got, want)
        assert np.array_equal(got[m == 0], img[m == 0])                  # the kept pixels are the init picture's, byte for byte
        assert not np.array_equal(got[m == 255], img[m == 255])
    # without composite the output path is untouched: the plain conversion of the same decode
    pipe.seed_everything(4)
    plain, _ = pipe.generate_image(["p", "q"], "", **kw)
    assert np.array_equal(np.array(plain[0]), decoded[0].float().mul(255).byte().permute(1, 2, 0).cpu().numpy())


def test_outpaint_canvas_feeds_an_inpainting_run():
    from PIL import Image
    c = cases.E2E_CASES[NAME]
    small = synthetic_image(c["H"], c["W"] - 256, seed=7)
    pipe = _pipe(NAME)
    want_c, want_m = S.canvas_pad(small, 128, 0, 128, 0)
    for src in (small, Image.fromarray(small), torch.from_numpy(small).to(DEV)):
        canvas, mask = pipe.outpaint_canvas(src, 128, 0, 128, 0)
        assert canvas.is_cuda and torch.equal(canvas.cpu(), torch.from_numpy(np.ascontiguousarray(want_c)))
        assert torch.equal(mask.cpu(), torch.from_numpy(want_m))
    pipe.seed_everything(2)
    z = pipe.generate_latents("p", "", **_loop_kw(NAME), init_image=canvas, mask_image=mask, strength=0.5)
    keep = torch.from_numpy(want_m[::8, ::8] == 0).expand_as(z).to(DEV)
    assert torch.equal(z[keep], pipe.last_init_latents[keep]) and bool((z[~keep] != pipe.last_init_latents[~keep]).any())
    with pytest.raises(ValueError, match="borders"):
        pipe.outpaint_canvas(small, -1, 0, 0, 0)
    with pytest.raises(ValueError, match="RGB"):
        pipe.outpaint_canvas(torch.zeros(1, 3, 8, 8), 1, 0, 0, 0)


CLI_RUNS = {
    "mask_blur": ["--mask_blur", "6"],
    "mask_mode": ["--mask_mode", "graded"],
    "composite": ["--composite", "--mask_blur", "0"],
    "outpaint": ["--outpaint", "16,0,16,8"],
}


@pytest.mark.parametrize("flag", sorted(CLI_RUNS))
def test_cli_flags(flag, tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    p, q = str(tmp_path / "init.png"), str(tmp_path / "mask.png")
    init, mask = synthetic_image(96, 128, seed=1), half_mask(96, 128, s=1)
    Image.fromarray(init).save(p)
    Image.fromarray(mask).save(q)
    argv = ["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1", "--outdir",
            str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4", "--exp", "soft",
            "--init_image", p, "--strength", "0.5"] + ([] if flag == "outpaint" else ["--mask_image", q]) + CLI_RUNS[flag]
    d = main(argv)
    a = np.asarray(Image.open(os.path.join(d, "0.png")))
    assert a.shape == (512, 512, 3) and a.std() > 0
    txt = open(os.path.join(d, "args.txt")).read()
    assert {"mask_blur": "mask_blur: 6.0", "mask_mode": "mask_mode: graded", "composite": "composite: True",
            "outpaint": "outpaint: 16,0,16,8"}[flag] in txt
    if flag == "composite":   # the kept pixels are the Lanczos-resized init picture's, the mask resized with NEAREST
        big = np.array(Image.fromarray(init).resize((512, 512), resample=Image.LANCZOS))
        m = np.array(Image.fromarray(mask).resize((512, 512), resample=Image.NEAREST))
        assert np.array_equal(a[m == 0], big[m == 0]) and not np.array_equal(a[m == 255], big[m == 255])
