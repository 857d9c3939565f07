"""models.py against the independent fp64 statement of the same forwards (tests/sd_spec.py), on the CPU.

Every parameter is randomised (``sd_spec.randomise``) so that no norm is an identity and no bias is small, every input row differs,
and the bar -- relative L2 <= 1e-9 -- sits six orders above fp64 rounding and four below the smallest semantic difference the models
show (a gelu flavour: 2.4e-5).  The blindness tests check that claim for THESE inputs: every ``SEMANTICS`` entry and every parameter
tensor zeroed on its own must move the spec's output by more than 1e-6.
"""
import functools
import math

import pytest
import torch

from elasticdiffusion_official_amd import models as M
from tests import sd_spec as S

BAR = 1e-9          # module (fp64, CPU) against the spec (fp64, CPU)
VISIBLE = 1e-6      # what one semantic change / one zeroed tensor must move the reference by: 1000 x BAR
SIZE = (16, 8)      # latent height, width of the whole-model inputs: not square, and 2 x 1 pixels are left at sd15's fourth level
FAMILIES = ("sd15", "sdxl")
VAE_BOC = tuple(M.SMALL_VAE_CHANNELS)


def _prepare(module, seed):
    """seeded default init, fp64, then every affine parameter / bias randomised"""
    M._seeded_init(module, seed)
    module = module.double().eval().requires_grad_(False)
    module.load_state_dict(S.randomise(module.state_dict(), seed))
    return module


@functools.lru_cache(maxsize=None)
def _unet(fam):
    m = _prepare(M.UNet2DConditionModel(**M.SMALL_UNET_CONFIGS[fam]), 11)
    return m, dict(m.state_dict())


@functools.lru_cache(maxsize=None)
def _controlnet(fam):
    m = _prepare(M.ControlNetModel(M.SMALL_UNET_CONFIGS[fam]), 12)
    return m, dict(m.state_dict())


@functools.lru_cache(maxsize=None)
def _vae():
    m = _prepare(M.AutoencoderKL(block_out_channels=VAE_BOC), 13)
    return m, dict(m.state_dict())


@functools.lru_cache(maxsize=None)
def _inputs(fam):
    return S.unet_inputs(M.SMALL_UNET_CONFIGS[fam], SIZE, seed=len(fam))


@functools.lru_cache(maxsize=None)
def _vae_inputs():
    g = torch.Generator().manual_seed(77)
    return (torch.rand(S.BATCH, 3, 32, 32, generator=g, dtype=torch.float64) * 2 - 1,
            torch.randn(S.BATCH, 4, 8, 8, generator=g, dtype=torch.float64))


def _kw(inp):
    return dict(added_cond_kwargs=inp["added"])


@functools.lru_cache(maxsize=None)
def _residuals(fam):
    """the spec's ControlNet outputs on the test inputs: the residuals the UNet comparisons feed to both sides (computed once)"""
    _, sd = _controlnet(fam)
    i = _inputs(fam)
    with torch.no_grad():
        return S.controlnet_forward(sd, M.SMALL_UNET_CONFIGS[fam], i["sample"], i["t"], i["context"], i["cond"],
                                    S.CONDITIONING_SCALE, i["added"])


def _check(name, got, want, bar=BAR):
    e = S.rel_l2(got, want)
    print(f"{name}: rel-L2 {e:.3e} (bar {bar:.0e})")
    assert e <= bar, (name, e)
    return e


# ---- sinusoid -------------------------------------------------------------------------------------------------------------------
def test_sinusoid_hand_table_and_closed_form():
    got = S.sinusoid(torch.tensor([1]), 4)[0].double()
    want = torch.tensor([math.cos(1.0), math.cos(0.01), math.sin(1.0), math.sin(0.01)], dtype=torch.float64)
    assert got.dtype == torch.float64 and S.sinusoid(torch.tensor([1]), 4).dtype == torch.float32      # computed in fp32
    assert float((got - want).abs().max()) <= 2 ** -23
    for dim in (4, 16, 64, 320):
        half = dim // 2
        t = torch.tensor([0, 1, 21, 500, 981, 999])
        emb = S.sinusoid(t, dim).double()
        assert emb.shape == (6, dim)
        for r, tv in enumerate(t.tolist()):
            for j in (0, 1, half // 2, half - 1):
                f = math.exp(-math.log(10000.0) * j / half)
                # fp32 evaluation: the argument t f carries a relative 2^-23 or so of its own size into cos / sin
                tol = 4 * 2 ** -23 * max(1.0, tv * f)
                assert abs(float(emb[r, j]) - math.cos(tv * f)) <= tol and abs(float(emb[r, half + j]) - math.sin(tv * f)) <= tol
    # the product's function states the same thing bit for bit (same fp32 formula)
    assert torch.equal(M.timestep_embedding(torch.tensor([981, 500, 21]), 64), S.sinusoid(torch.tensor([981, 500, 21]), 64))
    with S.override(flip_sin_to_cos=False):
        assert torch.equal(S.sinusoid(torch.tensor([1]), 4)[0, :2].double(), got[2:].float().double())
    assert S.SEMANTICS["flip_sin_to_cos"] is True


# ---- whole forwards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_unet_forward_equals_the_spec(fam):
    cfg = M.SMALL_UNET_CONFIGS[fam]
    m, sd = _unet(fam)
    i = _inputs(fam)
    down, mid = _residuals(fam)
    with torch.no_grad():
        plain = {}
        for t, tname in ((i["t"], "per-row t"), (i["t"][0], "scalar t")):
            plain[tname] = S.unet_forward(sd, cfg, i["sample"], t, i["context"], i["added"])
            _check(f"{fam} UNet, {tname}", m(i["sample"], t, i["context"], **_kw(i)).sample, plain[tname])
        assert S.rel_l2(plain["scalar t"][1:], plain["per-row t"][1:]) > 1e-3      # (rows 1, 2 have their own timestep)
        want_r = S.unet_forward(sd, cfg, i["sample"], i["t"], i["context"], i["added"], down, mid)
        got_r = m(i["sample"], i["t"], i["context"], down_block_additional_residuals=down, mid_block_additional_residual=mid, **_kw(i)).sample
        _check(f"{fam} UNet + ControlNet residuals", got_r, want_r)
        assert S.rel_l2(want_r, plain["per-row t"]) > 1e-3       # (the residuals are not a no-op)


@pytest.mark.parametrize("fam", FAMILIES)
def test_controlnet_forward_equals_the_spec(fam):
    m, _ = _controlnet(fam)
    i = _inputs(fam)
    want_down, want_mid = _residuals(fam)
    with torch.no_grad():
        got_down, got_mid = m(i["sample"], i["t"], i["context"], controlnet_cond=i["cond"], conditioning_scale=S.CONDITIONING_SCALE, **_kw(i))
    assert len(got_down) == len(want_down)
    for k, (g, w) in enumerate(zip(got_down, want_down)):
        assert g.shape == w.shape
        _check(f"{fam} ControlNet down residual {k}", g, w)
    _check(f"{fam} ControlNet mid residual", got_mid, want_mid)


def test_vae_encode_and_decode_equal_the_spec():
    m, sd = _vae()
    img, z = _vae_inputs()
    with torch.no_grad():
        dist = m.encode(img).latent_dist
        mean, std = S.vae_encode(sd, VAE_BOC, img)
        _check("VAE encode mean", dist.mean, mean)
        _check("VAE encode std", dist.std, std)
        _check("VAE decode", m.decode(z).sample, S.vae_decode(sd, VAE_BOC, z))
    assert float(std.std()) > 1e-3 * float(std.mean())     # (the std output is not a constant)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------
def _block(module, seed):
    module = _prepare(module, seed)
    return module, {"blk." + k: v for k, v in module.state_dict().items()}


def _rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("cin,cout,temb,eps", [(64, 64, 256, 1e-5), (64, 128, 256, 1e-5), (64, 64, None, 1e-6), (64, 96, None, 1e-6)])
def test_resnet_block_equals_the_spec(cin, cout, temb, eps):
    m, sd = _block(M.ResnetBlock2D(cin, cout, temb, eps=eps), cin + cout)
    x, emb = _rn(1, 3, cin, 12, 10), (None if temb is None else _rn(2, 3, temb))
    with torch.no_grad():
        _check(f"ResnetBlock2D {cin}->{cout} temb={temb}", m(x, emb), S.resnet(sd, "blk", x, emb, eps))
        with S.override(eps_unet=eps):          # eps left to the default entry
            _check("  (eps from SEMANTICS)", m(x, emb), S.resnet(sd, "blk", x, emb))


def test_resnet_block_on_a_concatenation_equals_the_spec():
    m, sd = _block(M.ResnetBlock2D(128 + 64, 96, 256), 5)
    x, skip, emb = _rn(1, 3, 128, 8, 12), _rn(2, 3, 64, 8, 12), _rn(3, 3, 256)
    with torch.no_grad():
        want = S.resnet_cat(sd, "blk", x, skip, emb)
        _check("ResnetBlock2D.forward_cat", m.forward_cat(x, skip, emb), want)
        with S.override(cat_x_first=False):
            assert S.rel_l2(S.resnet_cat(sd, "blk", x, skip, emb), want) > 1e-2


@pytest.mark.parametrize("C,heads,linear", [(128, 2, True), (128, 2, False), (320, 8, True), (320, 8, False)])
def test_transformer_2d_equals_the_spec(C, heads, linear):
    m, sd = _block(M.Transformer2DModel(C, heads, 2, 96, linear), C + heads + linear)
    x, ctx = _rn(1, 3, C, 6, 10), _rn(2, 3, S.CONTEXT_TOKENS, 96)
    with torch.no_grad():
        _check(f"Transformer2DModel C={C} heads={heads} linear={linear} depth 2", m(x, ctx), S.transformer_2d(sd, "blk", x, ctx, heads, 2, linear))
        # its parts, on the first block's own parameters
        t = _rn(3, 3, 60, C)
        p = "blk.transformer_blocks.0"
        b0 = m.transformer_blocks[0]
        pend, h = b0(t, ctx)
        _check("  BasicTransformerBlock", pend + h, S.basic_transformer_block(sd, p, t, ctx, heads))
        _check("  self-attention", b0.attn1(t), S.attention(sd, p + ".attn1", t, None, heads))
        _check("  cross-attention", b0.attn2(t, ctx), S.attention(sd, p + ".attn2", t, ctx, heads))
        _check("  cross-attention, precomputed k|v", b0.attn2(t, ctx, kv=b0.attn2.project_kv(ctx)), S.attention(sd, p + ".attn2", t, ctx, heads))
        _check("  GEGLU feed-forward", b0.ff(t), S.feed_forward(sd, p + ".ff", t))


def test_samplers_equal_the_spec():
    x = _rn(1, 3, 64, 10, 12)
    with torch.no_grad():
        m, sd = _block(M.Downsample2D(64, padding=1), 1)
        _check("Downsample2D(padding=1)", m(x), S.downsample(sd, "blk", x))
        m, sd = _block(M.Downsample2D(64, padding=0), 2)
        _check("Downsample2D(padding=0)", m(x), S.vae_downsample(sd, "blk", x))
        assert m(x).shape == (3, 64, 5, 6)
        m, sd = _block(M.Upsample2D(64), 3)
        _check("Upsample2D", m(x), S.upsample(sd, "blk", x))
        m, sd = _block(M.Upsample2D(64, vae=True), 4)
        _check("Upsample2D(vae)", m(x), S.vae_upsample(sd, "blk", x))


def test_vae_attention_and_condition_embedding_equal_the_spec():
    x = _rn(1, 3, 64, 6, 10)
    with torch.no_grad():
        m, sd = _block(M._VaeAttention(64), 1)
        _check("_VaeAttention", m(x), S.vae_attention(sd, "blk", x))
        m, sd = _block(M._CondEmbedding(64), 2)
        c = _rn(2, 3, 3, 32, 48)
        _check("ControlNet condition embedding", m(c), S.cond_embedding(sd, "blk", c))
        assert m(c).shape == (3, 64, 4, 6)
        vm, vsd = _vae()
        img, z = _vae_inputs()
        _check("VAE encoder", vm.encoder(img), S.vae_encoder(vsd, "encoder", VAE_BOC, img))
        _check("VAE decoder", vm.decoder(z), S.vae_decoder(vsd, "decoder", VAE_BOC, z))


# ---- blindness ------------------------------------------------------------------------------------------------------------------
def _spec_outputs(which, sds=None):
    """the spec's fp64 outputs on the tests' own inputs, one flat list of tensors per model"""
    sds = sds or {}
    out = {}
    with torch.no_grad():
        for fam in FAMILIES:
            cfg, i = M.SMALL_UNET_CONFIGS[fam], _inputs(fam)
            if ("unet", fam) in which:
                down, mid = _residuals(fam)
                out["unet", fam] = [S.unet_forward(sds.get(("unet", fam), _unet(fam)[1]), cfg, i["sample"], i["t"], i["context"], i["added"], down, mid)]
            if ("controlnet", fam) in which:
                d, m = S.controlnet_forward(sds.get(("controlnet", fam), _controlnet(fam)[1]), cfg, i["sample"], i["t"], i["context"], i["cond"],
                                            S.CONDITIONING_SCALE, i["added"])
                out["controlnet", fam] = list(d) + [m]
        if ("vae",) in which:
            img, z = _vae_inputs()
            sd = sds.get(("vae",), _vae()[1])
            out["vae",] = list(S.vae_encode(sd, VAE_BOC, img)) + [S.vae_decode(sd, VAE_BOC, z)]
    return out


MODELS = [("unet", "sd15"), ("unet", "sdxl"), ("controlnet", "sd15"), ("controlnet", "sdxl"), ("vae",)]


@functools.lru_cache(maxsize=None)
def _baseline():
    return _spec_outputs(set(MODELS))


ALTERNATIVES = {
    "eps_unet": 1e-6, "eps_transformer": 1e-5, "eps_vae": 1e-5, "eps_layernorm": 1e-6, "gelu": "tanh", "flip_sin_to_cos": False,
    "freq_shift": 1.0, "geglu_hidden_first": False, "cat_x_first": False, "cat_text_first": False, "asymmetric_pad": False,
    "attention_scale_exponent": -1.0, "vae_attention_bias": False,
}
# which models an entry can reach at all (a ControlNet has no up block, SD 1.5 no added condition, ...)
REACH = {"cat_x_first": [m for m in MODELS if m[0] == "unet"], "cat_text_first": [m for m in MODELS if m[-1] == "sdxl"],
         "asymmetric_pad": [("vae",)], "vae_attention_bias": [("vae",)], "eps_vae": [("vae",)],
         "attention_scale_exponent": MODELS}      # (the VAE attention's C ** exponent as well)
UNETS_AND_CONTROLNETS = [m for m in MODELS if m != ("vae",)]


def test_every_semantics_entry_has_an_alternative():
    assert set(ALTERNATIVES) == set(S.SEMANTICS)
    assert all(ALTERNATIVES[k] != v for k, v in S.SEMANTICS.items())


@pytest.mark.parametrize("entry", sorted(ALTERNATIVES))
def test_inputs_see_every_semantic_choice(entry):
    """a condition on the inputs: overriding one SEMANTICS entry moves every model it can reach by more than VISIBLE"""
    reach = REACH.get(entry, UNETS_AND_CONTROLNETS)
    base = _baseline()
    with S.override(**{entry: ALTERNATIVES[entry]}):
        moved = _spec_outputs(set(reach))
    assert S.SEMANTICS[entry] != ALTERNATIVES[entry]
    for m in reach:
        e = S.rel_l2(moved[m], base[m])
        print(f"{entry} -> {ALTERNATIVES[entry]!r}: {' '.join(m)} moves by {e:.3e}")
        assert e > VISIBLE, (entry, m, e)


def _invisible(model, key, sd):
    """Parameters no input can make visible, by the operations' own algebra (the test asserts that they move nothing):
    - the VAE attention's to_k.bias: it adds q.b to every score of a row, and softmax is invariant to a per-row constant;
    - where a GroupNorm has one channel per group (the small VAE's 32-channel level) a per-channel constant in front of it is removed by
      that channel's own mean: a ResnetBlock's conv1.bias in front of such a norm2, and, in the decoder's last level -- no upsampler, so
      nothing but residual adds between a block's output and conv_norm_out -- conv2.bias and conv_shortcut.bias as well.
    (The block tests compare those biases at widths where they do count.)"""
    if model != ("vae",):
        return False
    if key.endswith("attentions.0.to_k.bias"):
        return True
    if ".resnets." in key and key.endswith(".bias") and sd[key].shape[0] == S.GROUPS:
        last = f"decoder.up_blocks.{len(VAE_BOC) - 1}."
        return key.endswith(".conv1.bias") or (key.startswith(last) and key.endswith((".conv2.bias", ".conv_shortcut.bias")))
    return False


class _Memo:
    """The spec's block functions memoised on (prefix, the parameter tensors under the prefix by identity, the arguments by value): with
    ONE tensor of the state dict replaced, every block in front of it is a hit and only the rest of the network is computed again.
    Filled by the baseline run only, consulted by the trials."""
    FUNCS = ("time_embedding", "_conv", "resnet", "transformer_2d", "downsample", "upsample", "vae_downsample", "vae_attention",
             "cond_embedding")

    def __init__(self, sd):
        self.keys, self.store, self.recording = {}, {}, True
        for k in sd:
            parts = k.split(".")
            for n in range(1, len(parts)):
                self.keys.setdefault(".".join(parts[:n]), []).append(k)
        self.keys[""] = [k for k in sd if k.startswith(("time_embedding.", "add_embedding."))]     # (time_embedding's own, prefix "")

    @staticmethod
    def _same(a, b):
        if a is b:
            return True
        if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
        return isinstance(a, (bool, int, float, str, torch.dtype)) and type(a) is type(b) and a == b

    def wrap(self, name, fn):
        def cached(sd, p, *args, **kw):
            args = args + tuple(kw[k] for k in sorted(kw))
            key = (name, p, tuple(sorted(kw)), len(args), tuple(id(sd[k]) for k in self.keys[p]))
            hit = self.store.get(key)
            if hit is not None and all(self._same(a, b) for a, b in zip(args, hit[0])):
                return hit[1]
            out = fn(sd, p, *args[:len(args) - len(kw)], **kw)
            if self.recording:
                self.store[key] = (args, out)
            return out
        return cached


def _row0(model):
    """-> run(sd, part): the spec's outputs for the FIRST row of the tests' inputs (rows are independent in every model)"""
    if model == ("vae",):
        img, z = (t[:1] for t in _vae_inputs())
        return lambda sd, part: list(S.vae_encode(sd, VAE_BOC, img)) if part == "encode" else [S.vae_decode(sd, VAE_BOC, z)]
    kind, fam = model
    cfg, i = M.SMALL_UNET_CONFIGS[fam], _inputs(fam)
    x, t, ctx, cond = i["sample"][:1], i["t"][:1], i["context"][:1], i["cond"][:1]
    added = None if i["added"] is None else {k: v[:1] for k, v in i["added"].items()}
    if kind == "controlnet":
        def run(sd, part):
            d, m = S.controlnet_forward(sd, cfg, x, t, ctx, cond, S.CONDITIONING_SCALE, added)
            return list(d) + [m]
        return run
    down, mid = _residuals(fam)
    down, mid = [d[:1] for d in down], mid[:1]
    return lambda sd, part: [S.unet_forward(sd, cfg, x, t, ctx, added, down, mid)]


SHARDS = [(m, k, 4 if m[0] == "unet" else 1) for m in MODELS for k in range(4 if m[0] == "unet" else 1)]      # (a few seconds per case)


@pytest.mark.parametrize("model,shard,shards", SHARDS, ids=["-".join(m) + f"-{k + 1}of{n}" for m, k, n in SHARDS])
def test_inputs_see_every_parameter_tensor(model, shard, shards, monkeypatch):
    """A condition on the inputs: zeroing any ONE parameter tensor moves the spec's fp64 output by more than VISIBLE.  Every tensor is
    tried; to keep that affordable a trial computes the first input row only -- the rows are independent, so
    ||moved - base|| over all rows >= the same over row 0, and ||row-0 change|| / ||base, all rows|| is a LOWER bound of the relative
    change -- and reuses the baseline's blocks in front of the zeroed tensor (``_Memo``)."""
    sd = _vae()[1] if model == ("vae",) else {"unet": _unet, "controlnet": _controlnet}[model[0]](model[1])[1]
    full = _baseline()[model]
    memo = _Memo(sd)
    for name in _Memo.FUNCS:
        monkeypatch.setattr(S, name, memo.wrap(name, getattr(S, name)))
    run = _row0(model)
    parts = ("encode", "decode") if model == ("vae",) else ("all",)
    with torch.no_grad():
        base = {part: run(sd, part) for part in parts}
        memo.recording = False
        norm = {"encode": full[:2], "decode": full[2:], "all": full}
        for part in parts:     # the recorded row 0 IS row 0 of the whole-batch baseline
            assert S.rel_l2(base[part], [t[:1] for t in norm[part]]) < 1e-12
        worst = []
        for key in list(sd)[shard::shards]:
            part = "all" if model != ("vae",) else ("encode" if key.startswith(("encoder.", "quant_conv.")) else "decode")
            trial = dict(sd)
            trial[key] = torch.zeros_like(sd[key])
            moved = run(trial, part)
            num = math.sqrt(sum(float((a - b).pow(2).sum()) for a, b in zip(moved, base[part])))
            e = num / math.sqrt(sum(float(b.pow(2).sum()) for b in norm[part]))
            if _invisible(model, key, sd):
                assert e < 1e-12, (key, e)
                continue
            worst.append((e, key))
            assert e > VISIBLE, (model, key, e)
    worst.sort()
    print(f"{' '.join(model)} [{shard + 1}/{shards}]: {len(worst)} of {len(list(sd)[shard::shards])} tensors zeroed one at a time, each moves the output by more than {VISIBLE:.0e}; "
          "least visible: " + ", ".join(f"{k} {e:.2e}" for e, k in worst[:3]))
