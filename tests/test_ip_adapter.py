"""IP-Adapter image prompts on the CPU: the module against the fp64 specification, the loader's strictness,
the image tokens, the CLIP input restatement against transformers' processor, and the argument rules."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from elasticdiffusion_official_amd import models as M
from elasticdiffusion_official_amd import pipeline as P
from tests import ip_adapter_cpu as C
from tests import ip_adapter_spec as IS
from tests import realarch
from tests import sd_spec as S
from tests.fakes import FakeUNet, FakeVAE

BAR = 1e-9          # test_sd_spec.py's bar: module (fp64, CPU) against the spec (fp64, CPU)
VISIBLE = 1e-6      # what a deliberate defect must move the result by
FAMILIES = {"XL1.0": "sdxl", "1.5": "sd15"}
NI, CLIP_DIM, SCALE = 4, 48, 0.7


@functools.lru_cache(maxsize=None)
def _setup(sdv):
    """(fp64 UNet with the adapter installed, its plain state dict, the adapter, cfg, inputs with context = [text | image tokens])"""
    cfg = M.SMALL_UNET_CONFIGS[FAMILIES[sdv]]
    unet = realarch.build_small(sdv)[0].double().eval().requires_grad_(False)
    plain = {k: v.clone() for k, v in unet.state_dict().items()}
    adapter = IS.random_adapter(cfg, NI, CLIP_DIM, seed=5, gain=4.0)
    assert unet.install_ip_adapter(adapter) == NI and unet.ip_tokens == NI
    unet.ip_scale = SCALE
    i = S.unet_inputs(cfg, (16, 8), seed=3)
    g = torch.Generator().manual_seed(9)
    embeds = torch.randn(S.BATCH, CLIP_DIM, generator=g, dtype=torch.float64)
    tokens = IS.image_tokens(adapter, embeds, cfg["cross_attention_dim"])
    i["context"] = torch.cat([i["context"], S.CONTEXT_SCALE * tokens], dim=1)
    return unet, plain, adapter, cfg, i


def _same_shape_down_up_swap(cfg):
    """a permutation of the layer list that swaps the first down-block layer with an up-block layer of the same width"""
    prefixes = IS.layer_prefixes(cfg)
    n = len(cfg["block_out_channels"])
    d = next(k for k, p in enumerate(prefixes) if p.startswith("down_blocks."))
    lvl = int(prefixes[d].split(".")[1])
    u = next(k for k, p in enumerate(prefixes) if p.startswith(f"up_blocks.{n - 1 - lvl}."))
    order = list(range(len(prefixes)))
    order[d], order[u] = order[u], order[d]
    return order


# ---- 1. spec vs module ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdv", list(FAMILIES))
def test_unet_with_adapter_equals_the_spec(sdv):
    unet, plain, adapter, cfg, i = _setup(sdv)
    with torch.no_grad():
        got = unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"]).sample
        want = IS.unet_forward(plain, adapter, cfg, i["sample"], i["t"], i["context"], SCALE, i["added"])
        e = S.rel_l2(got, want)
        print(f"{sdv}: module vs spec rel-L2 {e:.3e} (bar {BAR:.0e})")
        assert e <= BAR
        # the hoisted k|v gives the same forward
        kv = unet.cross_attention_kv(i["context"])
        assert S.rel_l2(unet(i["sample"], i["t"], i["context"], added_cond_kwargs=i["added"], cross_kv=kv).sample, want) <= BAR
        # the inputs notice each deliberate defect
        for name, kw in (("swapped layers", dict(order=_same_shape_down_up_swap(cfg))),
                         ("shared softmax", dict(defect="shared_softmax")), ("scale on text", dict(defect="scale_on_text"))):
            moved = S.rel_l2(IS.unet_forward(plain, adapter, cfg, i["sample"], i["t"], i["context"], SCALE, i["added"], **kw), want)
            print(f"{sdv}: {name} moves the spec by {moved:.3e}")
            assert moved > VISIBLE, name
        # and the adapter itself
        text_only = S.unet_forward(plain, cfg, i["sample"], i["t"], i["context"][:, :S.CONTEXT_TOKENS], i["added"])
        assert S.rel_l2(want, text_only) > 1e-3


def test_spec_context_manager_restores_sd_spec():
    before = S.attention
    with IS.decoupled(4, 1.0):
        assert S.attention is not before
    assert S.attention is before


def test_forward_guard_and_self_attention_untouched():
    unet, plain, adapter, cfg, i = _setup("1.5")
    with pytest.raises(ValueError, match="image tokens"):
        unet(i["sample"], i["t"], i["context"][:, :NI], added_cond_kwargs=i["added"])
    for name, mod in unet.named_modules():
        if name.endswith("attn1"):
            assert mod.ip_tokens == 0 and mod.to_k_ip is None


# ---- 2. loader ------------------------------------------------------------------------------------------------------------------
def _fresh(sdv="1.5"):
    return realarch.build_small(sdv)[0].eval().requires_grad_(False)


def _nested(flat):
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in flat.items():
        head, tail = k.split(".", 1)
        out[head][tail] = v
    return out


def test_flat_safetensors_and_nested_pickle_install_identical_tensors(tmp_path):
    from safetensors.torch import save_file
    cfg = M.SMALL_UNET_CONFIGS["sd15"]
    adapter = IS.random_adapter(cfg, NI, CLIP_DIM, seed=2, dtype=torch.float32)
    save_file({k: v.contiguous() for k, v in adapter.items()}, str(tmp_path / "a.safetensors"))
    torch.save(_nested(adapter), str(tmp_path / "a.bin"))
    states = []
    for src in (str(tmp_path / "a.safetensors"), str(tmp_path / "a.bin"), adapter, _nested(adapter)):
        unet = _fresh()
        keys0 = list(unet.state_dict())
        state, name = P.read_ip_adapter(src)
        assert name in ("a", "ip_adapter")
        unet.install_ip_adapter(state)
        sd = unet.state_dict()
        assert len(sd) == len(keys0) + 4 + 2 * len(IS.layer_prefixes(cfg))
        states.append(sd)
        # explicit mapping: layer n of the stated order holds ip_adapter.{2n+1}
        for n, p in enumerate(IS.layer_prefixes(cfg)):
            assert torch.equal(sd[p + ".to_k_ip.weight"], adapter[f"ip_adapter.{2 * n + 1}.to_k_ip.weight"])
            assert torch.equal(sd[p + ".to_v_ip.weight"], adapter[f"ip_adapter.{2 * n + 1}.to_v_ip.weight"])
        unet.remove_ip_adapter()
        assert list(unet.state_dict()) == keys0 and unet.ip_tokens == 0
    for sd in states[1:]:
        assert list(sd) == list(states[0]) and all(torch.equal(sd[k], states[0][k]) for k in sd)
    with pytest.raises(ValueError, match="safetensors"):
        P.read_ip_adapter(str(tmp_path / "a.ckpt"))


def _broken(adapter, how, cfg):
    bad = dict(adapter)
    cross = cfg["cross_attention_dim"]
    if how == "missing":
        del bad["ip_adapter.3.to_v_ip.weight"]
    elif how == "surplus":
        bad["ip_adapter.2.to_k_ip.weight"] = bad["ip_adapter.1.to_k_ip.weight"]
    elif how == "shape":
        bad["ip_adapter.1.to_k_ip.weight"] = bad["ip_adapter.1.to_k_ip.weight"][:-1]
    elif how == "ni33":
        bad["image_proj.proj.weight"] = torch.zeros(33 * cross, CLIP_DIM)
        bad["image_proj.proj.bias"] = torch.zeros(33 * cross)
    elif how == "resampler":
        bad["image_proj.latents"] = torch.zeros(1, 16, cross)
    return bad


@pytest.mark.parametrize("how", ["missing", "surplus", "shape", "ni33", "resampler"])
def test_a_file_that_does_not_fit_installs_nothing(how):
    cfg = M.SMALL_UNET_CONFIGS["sd15"]
    unet = _fresh()
    before = {k: v.clone() for k, v in unet.state_dict().items()}
    adapter = IS.random_adapter(cfg, NI, CLIP_DIM, seed=2, dtype=torch.float32)
    with pytest.raises(ValueError) as err:
        unet.install_ip_adapter(_broken(adapter, how, cfg))
    if how == "resampler":
        assert "Plus" in str(err.value) and "Resampler" in str(err.value)
    after = unet.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert unet.ip_tokens == 0 and unet.ip_image_proj is None
    # ... and on top of an installed adapter the installed one stays
    unet.install_ip_adapter(adapter)
    held = {k: v.clone() for k, v in unet.state_dict().items()}
    with pytest.raises(ValueError):
        unet.install_ip_adapter(_broken(adapter, how, cfg))
    after = unet.state_dict()
    assert list(after) == list(held) and all(torch.equal(after[k], held[k]) for k in held) and unet.ip_tokens == NI


# ---- 3. image tokens ------------------------------------------------------------------------------------------------------------
def test_image_tokens():
    unet, plain, adapter, cfg, i = _setup("1.5")
    cross = cfg["cross_attention_dim"]
    g = torch.Generator().manual_seed(4)
    e = torch.randn(3, CLIP_DIM, generator=g, dtype=torch.float64)
    assert S.rel_l2(unet.ip_image_tokens(e), IS.image_tokens(adapter, e, cross)) <= BAR
    un = unet.ip_image_tokens(torch.zeros(3, CLIP_DIM, dtype=torch.float64))
    assert un.shape == (3, NI, cross)
    assert S.rel_l2(un, IS.uncond_image_tokens(adapter, 3, cross)) <= BAR
    # the projection of zeros is LayerNorm(bias): not zero while proj.bias is not
    want = torch.nn.functional.layer_norm(adapter["image_proj.proj.bias"].reshape(1, NI, cross), (cross,),
                                          adapter["image_proj.norm.weight"], adapter["image_proj.norm.bias"], 1e-5)
    assert S.rel_l2(un[:1], want) <= BAR and float(un.abs().max()) > 0.1
    # [1, clip] broadcasts over the prompts
    one = unet.ip_image_tokens(e[:1].expand(3, -1))
    assert torch.equal(one[0], one[1]) and torch.equal(one[0], one[2])
    assert S.rel_l2(one[:1], unet.ip_image_tokens(e[:1])) <= BAR     # (a GEMM of another batch size may round differently)


# ---- 4. CLIP input --------------------------------------------------------------------------------------------------------------
PICTURES = {"landscape": (300, 517), "portrait": (517, 300), "square": (256, 256), "small": (150, 200)}


def picture(name):
    H, W = PICTURES[name]
    return np.random.default_rng(sorted(PICTURES).index(name)).integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _processor():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from transformers import CLIPImageProcessor
        return CLIPImageProcessor()


@pytest.mark.parametrize("name", list(PICTURES))
def test_clip_input_restatement_equals_the_processor(name):
    from PIL import Image
    u8 = picture(name)
    want = torch.as_tensor(np.asarray(_processor()(images=Image.fromarray(u8), return_tensors="np")["pixel_values"]))
    resized = C.pil_resize(u8)
    assert min(resized.shape[:2]) == 224
    from elasticdiffusion_official_amd import ops
    assert ops.clip_resize_size(*u8.shape[:2]) == tuple(resized.shape[:2]) == C.resize_size(*u8.shape[:2])
    got = C.u8_to_clip_input(torch.from_numpy(resized.copy()))
    assert got.shape == want.shape == (1, 3, 224, 224) and got.dtype == torch.float32
    d = float((got.double() - want.double()).abs().max())
    print(f"{name}: max |restatement - CLIPImageProcessor| = {d:.3e} (bar 1e-6)")
    assert d <= 1e-6


# ---- 5. arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_rules():
    chk = P.check_ip_adapter_arguments
    e = torch.zeros(1, 8)
    img = np.zeros((4, 4, 3), np.uint8)
    assert chk(False, False) is False
    assert chk(True, False, None, e) is True and chk(True, True, img, None) is True
    with pytest.raises(ValueError, match="unload_ip_adapter"):
        chk(True, True)
    with pytest.raises(ValueError, match="exactly one"):
        chk(True, True, img, e)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        chk(False, False, None, e)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        chk(False, False, img, None)
    with pytest.raises(ValueError, match="image_encoder"):
        chk(True, False, img, None)
    with pytest.raises(ValueError, match="clip_dim"):
        chk(True, False, None, torch.zeros(8))
    with pytest.raises(ValueError, match="RGB PIL image"):
        chk(True, True, torch.zeros(3, 4, 4), None)


class _NoDevice(nn.Module):
    """a stand-in that fails the test if the pipeline reaches a model before it has checked its arguments"""

    def forward(self, *a, **k):
        raise AssertionError("device work before the argument check")


def _bare_pipeline(loaded, encoder=None):
    """An ElasticDiffusion object without its constructor (which refuses a CPU device): enough state for the argument checks,
    nothing a launch could use."""
    pipe = P.ElasticDiffusion.__new__(P.ElasticDiffusion)
    nn.Module.__init__(pipe)
    pipe.device = torch.device("cpu")
    pipe.unet, pipe.vae = FakeUNet(64), FakeVAE()
    pipe.vae_scale_factor = 8
    pipe._ip = {"name": "a", "encoder": encoder} if loaded else None
    pipe._runner = None    # any use raises
    return pipe


@pytest.mark.parametrize("entry", ["generate_latents", "generate_image", "interleaved"])
def test_pipeline_raises_before_any_device_work(entry):
    e = torch.zeros(1, 8)
    img = np.zeros((8, 8, 3), np.uint8)

    def call(pipe, **kw):
        if entry == "interleaved":
            return pipe.generate_latents_interleaved([dict(prompts="p", seed=0, **kw)], height=512, width=512, num_inference_steps=2)
        return getattr(pipe, entry)("p", height=512, width=512, num_inference_steps=2, **kw)
    with pytest.raises(ValueError, match="unload_ip_adapter"):
        call(_bare_pipeline(True))
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        call(_bare_pipeline(False), ip_adapter_image_embeds=e)
    with pytest.raises(ValueError, match="image_encoder"):
        call(_bare_pipeline(True), ip_adapter_image=img)
    with pytest.raises(ValueError, match="exactly one"):
        call(_bare_pipeline(True, encoder=lambda p: e), ip_adapter_image=img, ip_adapter_image_embeds=e)
    if entry == "interleaved":
        with pytest.raises(ValueError, match="every job"):
            _bare_pipeline(True).generate_latents_interleaved(
                [dict(prompts="p", seed=0, ip_adapter_image_embeds=e), dict(prompts="q", seed=1)], height=512, width=512,
                num_inference_steps=2)


def test_cli_flags_are_parsed_and_checked(tmp_path):
    from elasticdiffusion_official_amd import __main__ as cli
    opt = cli.build_parser().parse_args(["--ip_adapter", "a.safetensors:0.7", "--ip_adapter_embeds", "e.pt"])
    assert cli._lora_arg(opt.ip_adapter) == ("a.safetensors", 0.7) and opt.ip_adapter_embeds == "e.pt"
    assert opt.ip_adapter_image is None and opt.image_encoder is None
    with pytest.raises(SystemExit, match="exactly one"):
        cli.main(["--ip_adapter", "a.safetensors"])
    with pytest.raises(SystemExit, match="need --ip_adapter"):
        cli.main(["--ip_adapter_embeds", "e.pt"])
    with pytest.raises(SystemExit, match="--image_encoder"):
        cli.main(["--ip_adapter", "a.safetensors", "--ip_adapter_image", "x.png"])
    with pytest.raises(SystemExit, match="no such file"):
        cli.main(["--ip_adapter", str(tmp_path / "none.safetensors"), "--ip_adapter_embeds", str(tmp_path / "e.pt")])
    t = torch.arange(6.0).reshape(1, 6)
    torch.save(t, str(tmp_path / "e.pt"))
    np.save(str(tmp_path / "e.npy"), t.numpy())
    assert torch.equal(cli._load_embeds(str(tmp_path / "e.pt")), t) and torch.equal(cli._load_embeds(str(tmp_path / "e.npy")), t)


def test_attention_module_paths_agree_on_the_cpu():
    """``models.Attention`` with an adapter: hoisted k|v and in-place refresh give the forward's own projection"""
    torch.manual_seed(0)
    a = M.Attention(64, 2, 32, cross_dim=24).double().eval().requires_grad_(False)
    a.set_ip_adapter(nn.Linear(24, 64, bias=False).double(), nn.Linear(24, 64, bias=False).double(), 3)
    a.ip_scale = 0.4
    x, ctx = torch.randn(2, 10, 64, dtype=torch.float64), torch.randn(2, 7 + 3, 24, dtype=torch.float64)
    kv = a.project_kv(ctx)
    assert kv.shape == (2, 10, 128)
    # (a GEMM on the fused weight may round differently from the separate one: 1e-12, not bit equality)
    assert S.rel_l2(kv[:, :7, :64], a.to_k(ctx[:, :7])) <= 1e-12 and S.rel_l2(kv[:, 7:, 64:], a.to_v_ip(ctx[:, 7:])) <= 1e-12
    assert S.rel_l2(kv[:, :7, 64:], a.to_v(ctx[:, :7])) <= 1e-12 and S.rel_l2(kv[:, 7:, :64], a.to_k_ip(ctx[:, 7:])) <= 1e-12
    out = a(x, ctx)
    assert torch.equal(a(x, ctx, kv=kv), out)
    held = kv.clone().zero_()
    assert a.project_kv(ctx, held) is held and torch.equal(held, kv)
    b = copy.deepcopy(a)
    b.set_ip_adapter()
    assert b.to_k_ip is None and b.ip_tokens == 0 and "to_k_ip.weight" not in b.state_dict()
    assert not torch.equal(b(x, ctx[:, :7]), out)
