"""-m gpu: image-to-image and masked inpainting through the HIP path.

Bars:
  * the four kernels against the torch-CPU op sequences of tests/img2img_cpu.py: BIT-EXACT, 16-byte and scalar paths alike;
  * end-to-end latents against ``Img2ImgOracle``: the project's rel-L2 < 1e-4 and an identical host RNG end state (the fake VAE's
    ``exp`` runs on the device in the product and on the CPU in the restatement, so z0 itself is not bit-equal);
  * the kept region of a masked run equals ``pipe.last_init_latents`` bit for bit;
  * interleaved vs alone 1e-5; without the keywords the loop launches and computes what it always did;
  * the real (reduced-width) VAE encoder through the init path against the CPU VAE: twice the error the GPU encoder has
    against the CPU one WITHOUT the new kernels, measured in the same test.
"""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ddim_variants as V
from tests import img2img_cpu as I
from tests.fakes import FakeUNet, FakeVAE, synthetic_text_embeds
from tests.glue_geometries import misaligned as _misaligned
from tests.golden import cases
from tests.test_hip_parity import DEV, rel_l2
from tests.test_img2img import half_mask, synthetic_image
from tests.test_scheduler_variants_gpu import V_TRAILING_ZSNR, _schedules

pytestmark = pytest.mark.gpu

EPS = dict()
LATENT_SHAPES = [(1, 4, 8, 8), (3, 4, 13, 19), (2, 4, 67, 97), (1, 4, 64, 128)]
NEW_ENTRY_POINTS = ("ed_u8_to_vae_input", "ed_img2img_init", "ed_mask_to_latent", "ed_inpaint_blend")


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------
# ed_u8_to_vae_input
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("H,W", [(8, 8), (13, 19), (67, 97), (64, 128)])
def test_u8_to_vae_input_bit_exact(H, W, dtype):
    """8x8 and 64x128 take the 4-pixel path, 13x19 and 67x97 (odd pixel counts: colour planes that do not start on 16 bytes)
    the scalar one; all 256 byte values occur."""
    ops = _ops()
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    flat = img.view(-1)
    n = min(256, flat.numel())
    flat[:n] = torch.arange(n, dtype=torch.uint8)
    if flat.numel() >= 256:
        assert len(set(flat.tolist())) == 256
    want = I.to_vae_input(img.numpy(), dtype)
    got = ops.u8_to_vae_input(img.to(DEV), dtype)
    assert got.dtype == dtype and tuple(got.shape) == (1, 3, H, W)
    assert torch.equal(got.cpu(), want)
    # a source that is not 4-byte aligned: the scalar kernel, the same bits
    got2 = ops.u8_to_vae_input(_misaligned(img), dtype)
    assert torch.equal(got2.cpu(), want)


def test_u8_to_vae_input_every_byte_value_in_every_lane():
    """every byte value at every one of the 12 byte positions of the 4-pixel kernel's three dwords"""
    ops = _ops()
    img = torch.stack([torch.roll(torch.arange(256, dtype=torch.uint8), k) for k in range(12)]).t().contiguous().view(32, 32, 3)
    for dtype in (torch.float32, torch.float16):
        assert torch.equal(ops.u8_to_vae_input(img.to(DEV), dtype).cpu(), I.to_vae_input(img.numpy(), dtype))


# ---------------------------------------------------------------------------------------------------
# ed_img2img_init
# ---------------------------------------------------------------------------------------------------
COEF_ROWS = [(EPS, 50, 0), (EPS, 50, 49), (V_TRAILING_ZSNR, 50, 0)]


@pytest.mark.parametrize("mdtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kw,steps,ti", COEF_ROWS)
@pytest.mark.parametrize("shape", LATENT_SHAPES)
def test_img2img_init_bit_exact(shape, kw, steps, ti, mdtype):
    ops = _ops()
    sch, _, ts = _schedules(kw, steps)
    a, b = sch.add_noise_coefficients(ts[ti])
    if kw.get("rescale_betas_zero_snr") and ti == 0:
        assert a == 0.0 and b == 1.0
    g = torch.Generator().manual_seed(sum(shape) + ti)
    mean = (torch.randn(shape, generator=g) * 3).to(mdtype)
    std = torch.exp(0.5 * torch.randn(shape, generator=g) - 2).to(mdtype)
    eps_p, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    sf = 0.18215
    want_z0, want_x = I.init_latent(mean, std, eps_p, noise, sf, torch.tensor(a), torch.tensor(b))
    z0, x = ops.img2img_init(mean.to(DEV), std.to(DEV), eps_p.to(DEV), noise.to(DEV), sf, a, b)
    assert z0.dtype == torch.float32 and x.dtype == torch.float32
    assert torch.equal(z0.cpu(), want_z0) and torch.equal(x.cpu(), want_x)
    if a == 0.0:
        assert torch.equal(x.cpu(), (0.0 * want_z0) + noise)
    # misaligned views (offset by one element): the scalar kernels, the same bits, into misaligned outputs too
    z0m, xm = _misaligned(torch.zeros(shape)), _misaligned(torch.zeros(shape))
    ops.img2img_init(_misaligned(mean), _misaligned(std), _misaligned(eps_p), _misaligned(noise), sf, a, b, z0=z0m, x=xm)
    assert torch.equal(z0m, z0) and torch.equal(xm, x)


# ---------------------------------------------------------------------------------------------------
# ed_mask_to_latent
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(104, 152), (64, 64)])
def test_mask_to_latent_exact(H, W):
    """bytes 0 / 127 / 128 / 255 at the sampled positions (8y, 8x) and, differently, off them: a kernel that averages the cell
    or samples its centre 8y + 4 gives another mask"""
    ops = _ops()
    g = torch.Generator().manual_seed(H)
    vals = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    m = vals[torch.randint(0, 4, (H, W), generator=g)]
    want = I.latent_mask(m.numpy(), 8)
    centre = I.latent_mask(np.roll(m.numpy(), (-4, -4), (0, 1)), 8)
    assert not torch.equal(want, centre) and 0 < int(want.sum()) < want.numel()
    got = ops.mask_to_latent(m.to(DEV), 8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H // 8, W // 8)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.mask_to_latent(m.view(H, W, 1).to(DEV), 8).cpu(), want)
    assert torch.equal(ops.mask_to_latent(_misaligned(m), 8).cpu(), want)
    # the direct (Hl, Wl) pass-through: non-zero = repaint, bool or uint8
    lat = m[: H // 8, : W // 8].contiguous()
    direct = I.latent_mask(lat.numpy(), 1)
    assert torch.equal(ops.mask_to_latent(lat.to(DEV), 1).cpu(), direct)
    assert torch.equal(ops.mask_to_latent((lat != 0).to(DEV), 1).cpu(), direct)
    assert set(direct.unique().tolist()) == {0, 1}


# ---------------------------------------------------------------------------------------------------
# ed_inpaint_blend
# ---------------------------------------------------------------------------------------------------
def _masks(Hl, Wl):
    chk = ((torch.arange(Hl).view(-1, 1) + torch.arange(Wl).view(1, -1)) % 2).to(torch.uint8)
    one_kept = torch.ones(Hl, Wl, dtype=torch.uint8)
    one_kept[Hl - 1, Wl - 1] = 0
    return {"all0": torch.zeros(Hl, Wl, dtype=torch.uint8), "all1": torch.ones(Hl, Wl, dtype=torch.uint8), "checker": chk,
            "one_kept_last": one_kept}


@pytest.mark.parametrize("shape", LATENT_SHAPES)
def test_inpaint_blend_bit_exact(shape):
    ops = _ops()
    sch, _, ts = _schedules(EPS, 50)
    a, b = sch.add_noise_coefficients(ts[17])
    g = torch.Generator().manual_seed(sum(shape))
    x, z0, noise = (torch.randn(shape, generator=g) for _ in range(3))
    x_d, z0_d, n_d = x.to(DEV), z0.to(DEV), noise.to(DEV)
    inf_noise = torch.full(shape, float("inf"))
    for name, m in _masks(*shape[2:]).items():
        m_d = m.to(DEV)
        want = I.blend(x, m, z0, noise, torch.tensor(a), torch.tensor(b), clean=False)
        out = torch.empty(shape, device=DEV)
        ops.inpaint_blend(x_d, m_d, z0_d, n_d, a, b, out=out)
        assert torch.equal(out.cpu(), want), name
        if name == "all1":
            assert torch.equal(out, x_d)
        if name == "all0":
            assert torch.equal(out.cpu(), torch.tensor(a) * z0 + torch.tensor(b) * noise)
        inplace = x_d.clone()
        assert ops.inpaint_blend(inplace, m_d, z0_d, n_d, a, b) is inplace         # in place
        assert torch.equal(inplace, out), name
        # the scalar kernel (misaligned buffers): the same bits, out of place and in place
        xm = _misaligned(x)
        om = _misaligned(torch.zeros(shape))
        ops.inpaint_blend(xm, m_d, _misaligned(z0), _misaligned(noise), a, b, out=om)
        assert torch.equal(om, out), name
        ops.inpaint_blend(xm, _misaligned(m), z0_d, n_d, a, b)
        assert torch.equal(xm, out), name
        # clean: z0 itself where kept, also when the noise holds inf (a select, not 1 * z0 + 0 * noise); noise may be absent
        want_c = I.blend(x, m, z0, inf_noise, 1.0, 0.0, clean=True)
        assert bool(torch.isfinite(want_c).all())
        for nz in (inf_noise.to(DEV), None):
            oc = torch.empty(shape, device=DEV)
            ops.inpaint_blend(x_d, m_d, z0_d, nz, 1.0, 0.0, out=oc, clean=True)
            assert torch.equal(oc.cpu(), want_c), name
        keep = (m == 0).expand(shape)
        assert torch.equal(oc.cpu()[keep], z0[keep])
        # ... and an inf on the side that is not taken does not leak in the noised blend either
        if name != "all0":
            nz = n_d.clone()
            nz[(m_d != 0).expand(shape)] = float("inf")
            o2 = torch.empty(shape, device=DEV)
            ops.inpaint_blend(x_d, m_d, z0_d, nz, a, b, out=o2)
            assert torch.equal(o2, out), name


def test_rejections_leave_the_launch_state_clean():
    ops = _ops()
    a = torch.zeros(1, 4, 8, 8, device=DEV)
    m = torch.ones(8, 8, dtype=torch.uint8, device=DEV)
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.u8_to_vae_input(img.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.img2img_init(a.cpu(), a, a, a, 1.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_to_latent(m.cpu(), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.inpaint_blend(a.cpu(), m, a, a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match=r"\[H,W,3\]"):
        ops.u8_to_vae_input(img[:, :, :2].contiguous())
    with pytest.raises(RuntimeError, match="uint8"):
        ops.u8_to_vae_input(img.float())
    with pytest.raises(RuntimeError, match="shape"):
        ops.img2img_init(a, a[:, :2].contiguous(), a, a, 1.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.img2img_init(a, a, a.half(), a, 1.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.img2img_init(a, a.half(), a, a, 1.0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="multiple of scale"):
        ops.mask_to_latent(torch.ones(12, 16, dtype=torch.uint8, device=DEV), 8)
    with pytest.raises(RuntimeError, match="uint8 or bool"):
        ops.mask_to_latent(m.float(), 1)
    with pytest.raises(RuntimeError, match="mask must be uint8"):
        ops.inpaint_blend(a, m.bool(), a, a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="mask must be"):
        ops.inpaint_blend(a, m[:4].contiguous(), a, a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="shape"):
        ops.inpaint_blend(a, m, a[:, :2].contiguous(), a, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="noise is required"):
        ops.inpaint_blend(a, m, a, None, 1.0, 0.0)
    assert ops._LAUNCH["device"] is None
    out = torch.empty_like(a)
    ops.inpaint_blend(a + 1, m, a, a, 1.0, 0.0, out=out)      # the launch state is clean again
    assert torch.equal(out, a + 1)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _pipe(name, sched_kw=EPS, text_encoder=None, **extra):
    from elasticdiffusion_official_amd import ElasticDiffusion
    from elasticdiffusion_official_amd.schedule import DDIMSchedule
    c = cases.E2E_CASES[name]
    return ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=FakeUNet(c["sample"]), vae=FakeVAE(),
                            text_encoder=text_encoder or V.embed_fn(False), scheduler=DDIMSchedule(**sched_kw), **extra)


def _loop_kw(name):
    c = cases.E2E_CASES[name]
    return dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"],
                **dict(cases.E2E_KW, **c.get("kw", {})))


def _inputs(name, masked):
    c = cases.E2E_CASES[name]
    return synthetic_image(c["H"], c["W"], seed=c["seed"]), (half_mask(c["H"], c["W"]) if masked else None)


_ORACLE = {}


def _oracle_run(name, sched_kw, strength, masked, gr):
    """The CPU restatement's (latent, RNG tail, z0, latent mask) for one case, computed once and shared."""
    key = (name, tuple(sorted(sched_kw.items())), strength, masked, gr)
    if key not in _ORACLE:
        c = cases.E2E_CASES[name]
        orc = I.Img2ImgOracle(FakeUNet(c["sample"]), FakeVAE(), V.DDIMVariants(**sched_kw), V.embed_fn(False), sd_version=c["sd"],
                              view_batch_size=c["vbs"])
        img, mask = _inputs(name, masked)
        orc.seed_everything(c["seed"])
        z = orc.generate_latent("p", "", **_loop_kw(name), guidance_rescale=gr, init_image=img, strength=strength, mask_image=mask)
        _ORACLE[key] = (z, torch.rand(4), orc.last_init_latents, orc.last_mask)
    return _ORACLE[key]


E2E = [
    ("cfg2_sd_512x1024", EPS, 0.5, False, 0.0),             # 64x128 latent, padded global pass, RePaint on; the last 2 of 4 steps
    ("cfg2_sd_512x1024", EPS, 1.0, False, 0.0),
    ("cfg2_sd_512x1024", EPS, 0.5, True, 0.0),              # kept: the left half + one isolated latent pixel
    ("cfg2_sd_512x1024", EPS, 1.0, True, 0.0),
    ("overlap_536x776", EPS, 0.75, True, 0.0),              # 67x97 latent, overlapping view centres; scalar blend
    ("tall_1024x512_norepaint", EPS, 1.0, True, 0.0),       # one blend per iteration, no phase-1 blend
    ("cfg2_sd_512x1024", V_TRAILING_ZSNR, 1.0, True, 0.7),  # a = 0 at the first timestep, guidance rescale on
]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,sched_kw,strength,masked,gr", E2E)
def test_end_to_end_vs_cpu_restatement(name, sched_kw, strength, masked, gr, fused):
    from elasticdiffusion_official_amd import ops, pipeline
    want, otail, oz0, om = _oracle_run(name, sched_kw, strength, masked, gr)
    img, mask = _inputs(name, masked)
    c = cases.E2E_CASES[name]
    pipeline.FUSED_GLUE = fused
    ops.TIMER.start()
    try:
        pipe = _pipe(name, sched_kw)
        pipe.seed_everything(c["seed"])
        z = pipe.generate_latents("p", "", **_loop_kw(name), guidance_rescale=gr, init_image=img, strength=strength,
                                  mask_image=mask).cpu()
        tail = torch.rand(4)
    finally:
        pipeline.FUSED_GLUE = True
        counts = {k: v[0] for k, v in ops.TIMER.stop().items()}
    err = rel_l2(z, want)
    print(f"{name} {sorted(sched_kw)} strength={strength} masked={masked} gr={gr} fused={fused}: rel-L2 {err:.3e}, "
          f"z0 rel-L2 {rel_l2(pipe.last_init_latents, oz0):.3e}")
    assert bool(torch.isfinite(z).all())
    assert err < 1e-4, err
    assert torch.equal(tail, otail)
    assert rel_l2(pipe.last_init_latents, oz0) < 1e-5
    # the loop ran the window's steps only, and blended where the specification says
    T = c["steps"]
    n = T - I.window(T, strength)
    two_phase = sum(1 for i in range(T - n, T) if _loop_kw(name)["repaint_sampling"] and c["R"] > 0 and i < T - 1)
    assert counts["ed_u8_to_vae_input"] == 1 and counts["ed_img2img_init"] == 1
    assert counts.get("ed_undo_step", 0) == two_phase
    assert counts.get("ed_mask_to_latent", 0) == (1 if masked else 0)
    assert counts.get("ed_inpaint_blend", 0) == ((n + two_phase) if masked else 0)
    if masked:
        keep = (om == 0).expand_as(z)
        assert torch.equal(z[keep], pipe.last_init_latents.cpu()[keep])


def test_kept_region_is_the_init_latent_bit_for_bit():
    name = "cfg2_sd_512x1024"
    img, mask = _inputs(name, True)
    pipe = _pipe(name)
    pipe.seed_everything(9)
    z = pipe.generate_latents("p", "", **_loop_kw(name), init_image=img, strength=0.5, mask_image=mask)
    m = I.latent_mask(mask, 8).to(DEV)
    z0 = pipe.last_init_latents
    assert z0 is not None and z0.shape == z.shape
    keep = (m == 0).expand_as(z)
    assert int(keep.sum()) == 4 * (64 * 64 + 1)
    assert torch.equal(z[keep], z0[keep])
    assert bool((z[~keep] != z0[~keep]).any())
    # the same mask given at latent resolution (bool, repaint = True) and as an L PIL image: the same latents
    from PIL import Image
    for alt in ((m != 0).cpu(), Image.fromarray(mask), torch.from_numpy(mask)[:, :, None].to(DEV)):
        pipe.seed_everything(9)
        z2 = pipe.generate_latents("p", "", **_loop_kw(name), init_image=Image.fromarray(img), strength=0.5, mask_image=alt)
        assert torch.equal(z2, z)


def test_absent_keywords_are_the_loop_as_it_was_and_the_keywords_are_not_ignored():
    from elasticdiffusion_official_amd import ops
    name = "cfg2_sd_512x1024"
    seed, steps = cases.E2E_CASES[name]["seed"], cases.E2E_CASES[name]["steps"]
    img, _ = _inputs(name, False)
    lat, counts = {}, {}
    for label, extra in (("omitted", {}), ("defaults", dict(init_image=None, strength=1.0, mask_image=None)),
                         ("on", dict(init_image=img, strength=0.5))):
        pipe = _pipe(name)
        pipe.seed_everything(seed)
        ops.TIMER.start()
        try:
            lat[label] = pipe.generate_latents("p", "", **_loop_kw(name), **extra).cpu()
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
        if label != "on":
            assert pipe.last_init_latents is None
    assert torch.equal(lat["omitted"], lat["defaults"])
    assert counts["omitted"] == counts["defaults"]
    phases = 2 * steps - 1
    glue = {k: v for k, v in counts["omitted"].items() if k in ("ed_assemble_rows", "ed_undo_step") or "epilogue" in k}
    assert glue == {"ed_assemble_rows": phases, "ed_phase_epilogue": phases, "ed_undo_step": steps - 1}, counts["omitted"]
    assert not any(k in counts["omitted"] for k in NEW_ENTRY_POINTS)
    assert rel_l2(lat["on"], lat["omitted"]) > 1e-3
    assert counts["on"]["ed_u8_to_vae_input"] == 1 and counts["on"]["ed_img2img_init"] == 1
    assert counts["on"]["ed_assemble_rows"] == 2 * 2 - 1      # the last two of the four steps


def test_interleaved_two_jobs_match_each_alone():
    name = "cfg2_sd_512x1024"
    kw = _loop_kw(name)
    img, mask = _inputs(name, True)

    def embed(prompts):  # stateless (the programs' calls interleave); the values V.embed_fn alternates between
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    pipe = _pipe(name, text_encoder=embed)
    jobs = [dict(prompts="p", negative_prompts="", seed=cases.E2E_CASES[name]["seed"], init_image=img, mask_image=mask),
            dict(prompts="p", negative_prompts="", seed=11)]
    alone = []
    for job in jobs:
        pipe.seed_everything(job["seed"])
        alone.append(pipe.generate_latents("p", "", **kw, init_image=job.get("init_image"), mask_image=job.get("mask_image")).clone())
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    for z, want in zip(got, alone):
        assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    assert rel_l2(got[0], _oracle_run(name, EPS, 1.0, True, 0.0)[0]) < 1e-4
    assert not torch.equal(got[0], got[1])
    with pytest.raises(ValueError, match="init_image"):      # below strength 1 every job needs an init image
        pipe.generate_latents_interleaved(jobs, in_flight=2, **kw, strength=0.5)


def test_resize_path_is_the_lanczos_resize_on_the_device():
    ops = _ops()
    name = "cfg2_sd_512x1024"
    small = synthetic_image(100, 150, seed=4)
    resized = ops.resize_u8(torch.from_numpy(small).to(DEV), (512, 1024), "lanczos")
    lat = []
    mask_small = half_mask(100, 150, s=1)
    for img, mask in ((small, None), (resized, None), (small, mask_small)):
        pipe = _pipe(name)
        pipe.seed_everything(2)
        lat.append(pipe.generate_latents("p", "", **_loop_kw(name), init_image=img, strength=0.5, mask_image=mask))
    assert torch.equal(lat[0], lat[1])
    assert not torch.equal(lat[0], lat[2])       # a mask of the unresized image's size is resized with it (host, NEAREST)


def test_pipeline_rejects_bad_arguments():
    name = "cfg2_sd_512x1024"
    pipe = _pipe(name)
    kw = _loop_kw(name)
    img, mask = _inputs(name, True)
    for call in (pipe.generate_latents, pipe.generate_image):
        with pytest.raises(ValueError, match="strength"):
            call("p", "", **kw, init_image=img, strength=0.0)
        with pytest.raises(ValueError, match="strength"):
            call("p", "", **kw, init_image=img, strength=0.2)          # int(4 * 0.2) = 0 steps
        with pytest.raises(ValueError, match="init_image"):
            call("p", "", **kw, strength=0.5)
        with pytest.raises(ValueError, match="init_image"):
            call("p", "", **kw, mask_image=mask)
    with pytest.raises(ValueError, match="float init_image"):
        pipe.generate_latents("p", "", **kw, init_image=torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="mask_image"):
        pipe.generate_latents("p", "", **kw, init_image=img, mask_image=mask[:100])
    # a float image of the right size in [0, 1] is the same picture
    pipe.seed_everything(1)
    z1 = pipe.generate_latents("p", "", **kw, init_image=img, strength=0.5)
    pipe.seed_everything(1)
    flt = torch.from_numpy(np.float32(img) / 255).permute(2, 0, 1)[None]
    z2 = pipe.generate_latents("p", "", **kw, init_image=flt, strength=0.5)
    assert torch.equal(z1, z2)


# ---------------------------------------------------------------------------------------------------
# the real VAE encoder
# ---------------------------------------------------------------------------------------------------
def test_real_vae_init_latent_vs_cpu_vae():
    """The reduced-width real ``AutoencoderKL`` (fp32, split-fp16 MFMA convolutions on the device) through the pipeline's init
    path on a 64x128-pixel image, against the same weights on the CPU with the same draws.  The bar is twice the rel-L2 the
    GPU encoder has against the CPU encoder WITHOUT the new kernels (the same posterior sample formed by torch ops from the
    specification's VAE input), measured here; the kernels themselves are bit-exact, so both figures are the encoder's.
    One run on the MI355X: GPU-vs-CPU encode without the new kernels 4.8e-7 (so the bar was 9.6e-7); the init path z0 4.8e-7,
    x 7.2e-8."""
    from elasticdiffusion_official_amd import ElasticDiffusion, pipeline
    from elasticdiffusion_official_amd.models import build_models
    _, vae = build_models("1.5", device="cpu", dtype=torch.float32, small=True, seed=0)
    pipe = ElasticDiffusion(DEV, "1.5", unet=FakeUNet(64), vae=copy.deepcopy(vae), text_encoder=V.embed_fn(False))
    H, W = 64, 128
    img = synthetic_image(H, W, seed=3)
    S = pipeline._Plan()
    S.P = pipeline._Plan()
    S.P.Hl, S.P.Wl, S.C, S.t_start = H // 8, W // 8, 4, 1
    pipe._timesteps = list(pipe.scheduler.set_timesteps(4))
    pipe.host_s = {"noise": 0.0}
    pipe.seed_everything(5)
    with torch.no_grad():
        x, z0, noise, m = pipe._img2img_start(S, 1, img, None)
    tail = torch.rand(2)
    # the CPU VAE on the same draws
    sf = vae.config.scaling_factor
    a, b = pipe.scheduler.add_noise_coefficients(pipe._timesteps[1])
    with torch.no_grad():
        dist = vae.encode(I.to_vae_input(img)).latent_dist
    torch.manual_seed(5)
    eps_p, nz = torch.randn(1, 4, H // 8, W // 8), torch.randn(1, 4, H // 8, W // 8)
    assert torch.equal(tail, torch.rand(2))
    want_z0, want_x = I.init_latent(dist.mean, dist.std, eps_p, nz, sf, torch.tensor(a), torch.tensor(b))
    assert torch.equal(noise.cpu(), nz)
    # the bar: this repository's GPU encode against its CPU encode, without the new kernels
    with torch.no_grad():
        gd = pipe.vae.encode(I.to_vae_input(img).to(DEV)).latent_dist
    base_z0 = (gd.mean.float() + gd.std.float() * eps_p.to(DEV)) * sf
    base = rel_l2(base_z0, want_z0)
    err_z0, err_x = rel_l2(z0, want_z0), rel_l2(x, want_x)
    print(f"real VAE 64x128: GPU-vs-CPU encode without the new kernels {base:.3e}; init path z0 {err_z0:.3e}, x {err_x:.3e} "
          f"(bar {2 * base:.3e})")
    assert 0 < base < 1e-3          # fp32 accuracy on the 16-bit MFMA pipe: a few 1e-7 per convolution
    assert err_z0 <= 2 * base and err_x <= 2 * base


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_init_image_strength_and_mask_flags(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    p, q = str(tmp_path / "init.png"), str(tmp_path / "mask.png")
    Image.fromarray(synthetic_image(96, 128, seed=1)).save(p)
    Image.fromarray(half_mask(96, 128, s=1)).save(q)
    d = main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2", "--resampling_steps", "1", "--outdir",
              str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4", "--exp", "i2i",
              "--init_image", p, "--strength", "0.5", "--mask_image", q])
    a = np.asarray(Image.open(os.path.join(d, "0.png")), dtype=np.float32)
    assert a.shape == (512, 512, 3) and np.isfinite(a).all() and a.std() > 0
    txt = open(os.path.join(d, "args.txt")).read()
    assert "strength: 0.5" in txt and f"init_image: {p}" in txt and f"mask_image: {q}" in txt
    with pytest.raises(SystemExit):
        main(["--strength", "0.5", "--outdir", str(tmp_path)])
