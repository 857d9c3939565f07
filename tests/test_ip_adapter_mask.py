"""IP-Adapter attention masks on the CPU: the fp64 modules against the fp64 specification, the deliberate
defects the inputs must notice, the fp32 restatement of the mask rows against the spec's rule, the argument rules with no
device, and the index replay of the masked one-launch kernel."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from elasticdiffusion_official_amd import models as M
from elasticdiffusion_official_amd import ops
from elasticdiffusion_official_amd import pipeline as P
from tests import ip_adapter_mask_spec as KS
from tests import ip_adapter_multi_spec as MS
from tests import ip_adapter_spec as IS
from tests import ip_mask_cpu as C
from tests import realarch
from tests import sd_spec as S
from tests.glue_geometries import SCALAR_GEOMETRIES, plans

BAR = 1e-9          # test_sd_spec.py's bar: module (fp64, CPU) against the spec (fp64, CPU)
VISIBLE = 1e-6      # what a deliberate defect must move the result by
FAMILIES = {"XL1.0": "sdxl", "1.5": "sd15"}
NI_BASE, NI_PLUS, CLIP_DIM, EMBED_DIM, SEQ = 4, 16, 48, 80, 10
WEIGHTS = (0.75, -0.5)
PH, PW = 16, 8      # sd_spec.unet_inputs' latent: the model row of the reduced-width forwards


def _gather(B, seed=0):
    """a synthetic fused batch of B = sd_spec.BATCH rows on a 16 x 8 row: one resampling step written twice (2 rows: a 12 x 6
    picked frame at (2, 1), so pad strips on both axes) and one view row whose 10 x 8 window starts at (-3, 0) -- context above
    the picture -- for ONE sample, on a 20 x 12 latent"""
    assert B == 3
    H, W, h, w = 20, 12, 12, 6
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 4, (1, h * w), generator=g, dtype=torch.uint8)
    src_row = torch.stack([torch.arange(h) * H // h, (torch.arange(h) * H // h + 1).clamp(max=H - 1)], 1).reshape(-1).int()
    src_col = torch.stack([torch.arange(w) * W // w, (torch.arange(w) * W // w + 1).clamp(max=W - 1)], 1).reshape(-1).int()
    return (H, W), (idx, src_row, src_col, h, w, 2, 1, torch.tensor([-3], dtype=torch.int32), torch.tensor([0], dtype=torch.int32),
                    10, 8, 4, 0, PH, PW, 2)


@functools.lru_cache(maxsize=None)
def _mask_rows(pad=0.0):
    (H, W), gather = _gather(S.BATCH)
    masks = C.u8_masks(1, 2, H, W, seed=11)
    return KS.mask_rows(masks, *gather, pad=pad), masks, gather


def _adapters(cfg, dtype=torch.float64):
    return [IS.random_adapter(cfg, NI_BASE, CLIP_DIM, seed=5, gain=4.0, dtype=dtype),
            MS.random_plus_adapter(cfg, NI_PLUS, EMBED_DIM, seed=6, gain=4.0, dtype=dtype)]


@functools.lru_cache(maxsize=None)
def _setup(sdv):
    """test_ip_adapter_multi._setup: the fp64 reduced-width UNet with a base adapter of 4 tokens and a Plus adapter of 16"""
    cfg = M.SMALL_UNET_CONFIGS[FAMILIES[sdv]]
    unet = realarch.build_small(sdv)[0].double().eval().requires_grad_(False)
    plain = {k: v.clone() for k, v in unet.state_dict().items()}
    adapters = _adapters(cfg)
    unet.install_ip_adapter(adapters[0])
    unet.install_ip_adapter(adapters[1], add=True)
    unet.ip_scales = WEIGHTS
    i = S.unet_inputs(cfg, (PH, PW), seed=3)
    g = torch.Generator().manual_seed(9)
    embeds = [torch.randn(S.BATCH, CLIP_DIM, generator=g, dtype=torch.float64),
              2.0 * torch.randn(S.BATCH, SEQ, EMBED_DIM, generator=g, dtype=torch.float64)]
    tokens = [MS.image_tokens(ad, e, cfg["cross_attention_dim"]) for ad, e in zip(adapters, embeds)]
    i["context"] = torch.cat([i["context"]] + [S.CONTEXT_SCALE * t for t in tokens], dim=1)
    return unet, plain, adapters, cfg, i


# ---- 1. spec vs module ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdv", list(FAMILIES))
def test_unet_with_masked_adapters_equals_the_spec_and_the_inputs_notice_the_defects(sdv):
    unet, plain, adapters, cfg, i = _setup(sdv)
    segs = (NI_BASE, NI_PLUS)
    m, _, _ = _mask_rows()
    assert tuple(m.shape) == (S.BATCH, 2, KS.layout(PH, PW)[1]) and m.dtype == torch.float32
    assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
    args = (plain, adapters, cfg, i["sample"], i["t"], i["context"], segs, WEIGHTS)
    with torch.no_grad():
        got = unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(m, PH, PW)).sample
        want = KS.unet_forward(*args, m, PH, PW, i["added"])
        e = S.rel_l2(got, want)
        print(f"{sdv}: masked module vs spec rel-L2 {e:.3e} (bar {BAR:.0e})")
        assert e <= BAR
        kv = unet.cross_attention_kv(i["context"])
        assert S.rel_l2(unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], cross_kv=kv,
                             ip_masks=(m, PH, PW)).sample, want) <= BAR
        assert all(a.ip_mask is None for a in unet.ip_attentions())          # the masks last for one forward
        for defect in ("mask_on_text", "masks_swapped", "level_stride", "key_mask"):
            moved = S.rel_l2(KS.unet_forward(*args, m, PH, PW, i["added"], defect=defect), want)
            print(f"{sdv}: {defect} moves the spec by {moved:.3e}")
            assert moved > VISIBLE, defect
        moved = S.rel_l2(KS.unet_forward(*args, _mask_rows(1.0)[0], PH, PW, i["added"]), want)       # pad value 1 instead of 0
        print(f"{sdv}: pad_one moves the spec by {moved:.3e}")
        assert moved > VISIBLE
        # all-ones masks are the unmasked forward; all-zero masks the forward at weights 0 (text only)
        ones = torch.ones_like(m)
        plain_out = unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"]).sample
        assert S.rel_l2(unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(ones, PH, PW)).sample,
                        plain_out) <= BAR
        text_only = S.unet_forward(plain, cfg, i["sample"], i["t"], i["context"][:, :S.CONTEXT_TOKENS], i["added"])
        assert S.rel_l2(unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"],
                             ip_masks=(torch.zeros_like(m), PH, PW)).sample, text_only) <= BAR
        assert S.rel_l2(want, plain_out) > 1e-3 and S.rel_l2(want, text_only) > 1e-3
        # a change of scales reaches the masked path through the one device tensor
        unet.ip_scales = (0.25, 1.5)
        want2 = KS.unet_forward(*args[:-1], (0.25, 1.5), m, PH, PW, i["added"])
        assert S.rel_l2(unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(m, PH, PW)).sample, want2) <= BAR
        unet.ip_scales = WEIGHTS


def test_single_adapter_with_masks_reads_its_scale_from_the_device_weights():
    """one adapter: without masks the by-value scale and no weight tensor, as always; with masks the UNet allocates the fp32 tensor
    and the scale setter keeps it current"""
    cfg = M.SMALL_UNET_CONFIGS["sd15"]
    unet = realarch.build_small("1.5")[0].double().eval().requires_grad_(False)
    plain = {k: v.clone() for k, v in unet.state_dict().items()}
    ad = _adapters(cfg)[0]
    unet.install_ip_adapter(ad)
    assert unet.ip_weights is None
    unet.ip_scale = 0.75
    i = S.unet_inputs(cfg, (PH, PW), seed=4)
    g = torch.Generator().manual_seed(2)
    tok = MS.image_tokens(ad, torch.randn(S.BATCH, CLIP_DIM, generator=g, dtype=torch.float64), cfg["cross_attention_dim"])
    ctx = torch.cat([i["context"], S.CONTEXT_SCALE * tok], dim=1)
    m = _mask_rows()[0][:, :1].contiguous()
    with torch.no_grad():
        got = unet(i["sample"], i["t"], ctx, added_cond_kwargs=i["added"], ip_masks=(m, PH, PW)).sample
        assert unet.ip_weights is not None and float(unet.ip_weights[0]) == 0.75
        assert S.rel_l2(got, KS.unet_forward(plain, [ad], cfg, i["sample"], i["t"], ctx, (NI_BASE,), (0.75,), m, PH, PW, i["added"])) <= BAR
        unet.ip_scale = -0.5
        got = unet(i["sample"], i["t"], ctx, added_cond_kwargs=i["added"], ip_masks=(m, PH, PW)).sample
        assert S.rel_l2(got, KS.unet_forward(plain, [ad], cfg, i["sample"], i["t"], ctx, (NI_BASE,), (-0.5,), m, PH, PW, i["added"])) <= BAR


def test_model_refuses_masks_it_cannot_place():
    unet, plain, adapters, cfg, i = _setup("1.5")
    m = _mask_rows()[0]
    with pytest.raises(ValueError, match="ip_masks"):
        unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(m[:, :1], PH, PW))      # one adapter's masks for two
    with pytest.raises(ValueError, match="ip_masks"):
        unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(m.double(), PH, PW))
    big = torch.ones(S.BATCH, 2, KS.layout(32, 16)[1])
    with pytest.raises(ValueError, match="matches no level"):       # a 32 x 16 pyramid for 16 x 8 rows: no cross attention finds its level
        unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], ip_masks=(big, 32, 16))
    assert all(a.ip_mask is None for a in unet.ip_attentions())
    bare = realarch.build_small("1.5")[0].double().eval()
    with pytest.raises(ValueError, match="without an installed IP-Adapter"):
        bare(i["sample"], i["t"], i["context"][:, :S.CONTEXT_TOKENS], added_cond_kwargs=i["added"], ip_masks=(m, PH, PW))


# ---- 2. the mask rows: the fp32 restatement against the spec's rule, on real geometries ------------------------------------------
@pytest.mark.parametrize("name", ["ff_views", "tf"])
def test_fp32_restatement_of_the_mask_rows_is_the_specs_rule(name):
    Hl, Wl, h, w, d = SCALAR_GEOMETRIES[name]
    pp, vp, gpad, vpad = plans(Hl, Wl, h, w, d)
    assert (gpad.PH, gpad.PW) == (vpad.PH, vpad.PW) == (d, d)
    torch.manual_seed(5)
    idx = torch.randint(0, 4, (2, h * w), dtype=torch.uint8)
    t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32)      # noqa: E731
    gather = (idx, t32(pp.src_row), t32(pp.src_col), h, w, gpad.top, gpad.left, t32(vp.win_y0), t32(vp.win_x0), vp.Sh, vp.Sw,
              vpad.top, vpad.left, d, d, 3)
    masks = C.u8_masks(2, 3, Hl, Wl, seed=Hl)
    got = C.mask_rows(masks, *gather)
    want = KS.mask_rows(masks, *gather)
    assert tuple(got.shape) == ((2 * 3 + vp.V) * 2, 3, KS.layout(d, d)[1]) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert C.layout(d, d) == KS.layout(d, d) == ops.ip_mask_layout(d, d)
    # levels are means: inside [0, 1]; and the fp64 rule differs from the fp32 one by rounding alone
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float((KS.mask_rows(masks.double(), *gather) - got.double()).abs().max()) < 1e-6
    # pad strips are 0 at level 0
    l0 = got[:, :, :d * d].view(-1, 3, d, d)
    assert gpad.left > 0 and float(l0[0, :, :, :gpad.left].abs().max()) == 0.0 and float(l0[0, :, :, gpad.left + w:].abs().max()) == 0.0


# ---- 3. argument rules, with no device -----------------------------------------------------------------------------------------
def test_argument_rules_of_the_masks():
    chk = P.check_ip_adapter_mask_arguments
    pic, lat = np.zeros((512, 768), np.uint8), torch.zeros(64, 96, dtype=torch.uint8)
    assert chk(0, None, 512, 768) is None and chk(2, None, 512, 768) is None
    out = chk(3, [pic, None, (0, 0, 768, 512)], 512, 768)
    assert out[0][0] == "pixel" and out[1] is None and out[2] == ("box", (0, 0, 768, 512))
    assert chk(1, [lat], 512, 768)[0][0] == "latent"
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        chk(0, [pic], 512, 768)
    with pytest.raises(ValueError, match="one entry per adapter"):
        chk(2, [pic], 512, 768)
    with pytest.raises(ValueError, match="one entry per adapter"):
        chk(1, pic, 512, 768)
    with pytest.raises(ValueError, match=r"ip_adapter_masks\[1\]: the mask is \(100, 100\)"):
        chk(2, [None, np.zeros((100, 100), np.uint8)], 512, 768)
    with pytest.raises(ValueError, match=r"ip_adapter_masks\[0\]: box"):
        chk(1, [(0, 0, 769, 512)], 512, 768)
    with pytest.raises(ValueError, match=r"ip_adapter_masks\[0\]: the mask must be"):
        chk(1, [np.zeros((512, 768), np.float32)], 512, 768)


def _bare_pipeline(kinds):
    """test_ip_adapter_multi._bare_pipeline: enough state for the argument checks, nothing a launch could use"""
    from tests.fakes import FakeUNet, FakeVAE
    pipe = P.ElasticDiffusion.__new__(P.ElasticDiffusion)
    torch.nn.Module.__init__(pipe)
    pipe.device = torch.device("cpu")
    pipe.unet, pipe.vae = FakeUNet(64), FakeVAE()
    pipe.vae_scale_factor = 8
    pipe._ip_set([{"name": f"a{k}", "encoder": None, "kind": kind} for k, kind in enumerate(kinds)])
    pipe._runner = None    # any use raises
    return pipe


@pytest.mark.parametrize("entry", ["generate_latents", "generate_image", "interleaved"])
def test_pipeline_raises_on_bad_masks_before_any_device_work(entry):
    base = torch.zeros(1, 8)
    box = (0, 0, 256, 512)

    def call(pipe, **kw):
        if entry == "interleaved":
            return pipe.generate_latents_interleaved([dict(prompts="p", seed=0, **kw)], height=512, width=512, num_inference_steps=2)
        return getattr(pipe, entry)("p", height=512, width=512, num_inference_steps=2, **kw)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        call(_bare_pipeline([]), ip_adapter_masks=[box])
    with pytest.raises(ValueError, match="one entry per adapter"):
        call(_bare_pipeline(["base", "base"]), ip_adapter_image_embeds=[base, base], ip_adapter_masks=[box])
    with pytest.raises(ValueError, match=r"ip_adapter_masks\[1\]: box"):
        call(_bare_pipeline(["base", "base"]), ip_adapter_image_embeds=[base, base], ip_adapter_masks=[box, (0, 0, 513, 512)])
    with pytest.raises(ValueError, match=r"ip_adapter_masks\[0\]: the mask is"):
        call(_bare_pipeline(["base"]), ip_adapter_image_embeds=base, ip_adapter_masks=[np.zeros((10, 10), np.uint8)])


def test_cli_mask_flags_match_the_adapters_by_position(tmp_path):
    from elasticdiffusion_official_amd import __main__ as cli
    opt = cli.build_parser().parse_args(["--ip_adapter_mask", "0,0,256,512", "--ip_adapter_mask", "none"])
    assert cli.parse_ip_adapter_masks(opt, 2) == [(0, 0, 256, 512), None]
    assert cli.parse_ip_adapter_masks(cli.build_parser().parse_args([]), 2) is None
    with pytest.raises(SystemExit, match="matched by position"):
        cli.parse_ip_adapter_masks(opt, 1)
    opt = cli.build_parser().parse_args(["--ip_adapter_mask", str(tmp_path / "m.png")])
    with pytest.raises(SystemExit, match="no such file"):
        cli.parse_ip_adapter_masks(opt, 1)
    assert cli.parse_ip_adapter_masks(cli.build_parser().parse_args(["--ip_adapter_mask", __file__]), 1, open_image=lambda p: "pic") == ["pic"]
    with pytest.raises(SystemExit, match="matched by position"):
        cli.main(["--ip_adapter_mask", "0,0,8,8"])                       # a mask without an adapter


# ---- 4. ops wrappers refuse before a launch ---------------------------------------------------------------------------------------
def test_wrappers_have_no_cpu_path():
    q = torch.zeros(1, 4, 64, dtype=torch.float16)
    k = torch.zeros(1, 5, 64, dtype=torch.float16)
    assert ops.flash_attention_ipm_ok(64, 77, (4, 16)) and not ops.flash_attention_ipm_ok(40, 77, (4,))
    assert not ops.flash_attention_ipm_ok(64, 161, (4,)) and not ops.flash_attention_ipm_ok(64, 77, (16, 17))
    with pytest.raises(RuntimeError, match="flash_attention_ipm"):
        ops.flash_attention_ipm(q, k, k, 1, 1, (4,), torch.zeros(1), torch.ones(1, 1, 4))
    with pytest.raises(RuntimeError, match="ip_mask_rows"):
        ops.ip_mask_rows(torch.zeros(1, 1, 8, 8), None, None, None, 0, 0, 0, 0, None, None, 0, 0, 0, 0, 8, 8, 2)
    lay, total = ops.ip_mask_layout(128, 64)
    assert lay == [(0, 8192), (8192, 2048), (10240, 512), (10752, 128)] and total == 10880


# ---- 5. index replay ---------------------------------------------------------------------------------------------------------------
def _emulator():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import emulate_flash_attention_ipm
    return emulate_flash_attention_ipm


@pytest.mark.parametrize("case", range(10))
def test_kernel_index_math_replay(case):
    """tools/emulate_flash_attention_ipm.py: which lane holds which query row and the address of m for it under m_sb, m_sa and the
    level offset, in fp64 against A + 1 masked softmaxes; every word of the mask buffer the rule does not address is NaN, and the
    set of words read is exactly the addressed one"""
    E = _emulator()
    assert len(E.CASES) == 10
    Nq, Nt, segs, kw = E.CASES[case]
    err = E.check_case(Nq, Nt, segs, **kw)
    assert err < 1e-12, (Nq, Nt, segs, kw, err)
