"""-m gpu: IP-Adapter image prompts on the device -- the one-launch decoupled cross attention, the CLIP
input kernel, the dispatch of models.Attention, the real architectures with an adapter, the product loop against the oracle,
graphs, jobs in flight and the command line."""
import copy
import glob
import os

import pytest
import torch
import torch.nn.functional as F

from oracle.ddim import DDIMOracle
from oracle.elastic_oracle import ElasticOracle
from tests import ip_adapter_cpu as C
from tests import ip_adapter_spec as IS
from tests import procs
from tests import realarch as R
from tests.test_ip_adapter import PICTURES, picture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NI, CLIP_DIM = 4, 48


def _heads(t, H):
    return t.reshape(t.shape[0], -1, H, 64).transpose(1, 2)


def _attn_ref(q, k, v, H, scale=0.125):
    """fp32, as test_long_prompts_gpu._attn_ref"""
    B, Nq, HD = q.shape
    qf, kf, vf = (_heads(t.float(), H) for t in (q, k, v))
    return (torch.softmax(qf @ kf.transpose(-1, -2) * scale, dim=-1) @ vf).transpose(1, 2).reshape(B, Nq, HD)


def _ip_ref(q, k, v, H, nt, s):
    return _attn_ref(q, k[:, :nt], v[:, :nt], H) + s * _attn_ref(q, k[:, nt:], v[:, nt:], H)


def _sdpa(q, k, v, H):
    return F.scaled_dot_product_attention(_heads(q, H), _heads(k, H), _heads(v, H), scale=0.125).transpose(1, 2).reshape(q.shape)


def _qkv(B, H, Nq, N, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Nq, H * 64, device=DEV, generator=g).mul(1.5).to(dtype)
    kv = torch.randn(B, N, 2 * H * 64, device=DEV, generator=g)
    kv[..., :H * 64] *= 1.5
    kv = kv.to(dtype)
    return q, kv[..., :H * 64], kv[..., H * 64:]


# ---- 6. kernel vs fp32 reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H", [(2, 3), (1, 10)])
@pytest.mark.parametrize("Nq", [1, 100, 513])
@pytest.mark.parametrize("Nt", [1, 77, 96, 97, 154, 160])
def test_decoupled_cross_attention_against_fp32(dtype, B, H, Nq, Nt):
    """ops.flash_attention_ip vs two fp32 softmaxes, under test_long_prompts_gpu's bar relative to SDPA run the plain way (two
    SDPA calls and the axpy in the same dtype); k / v as the column halves of one [B, Nt + Ni, 2 inner] tensor give the bits the
    contiguous tensors give."""
    from elasticdiffusion_official_amd import ops
    for Ni in (1, 4, 16, 32):
        q, k, v = _qkv(B, H, Nq, Nt + Ni, dtype, Nq * 7 + Nt * 3 + Ni)
        for s in (0.6, 1.0):
            got = ops.flash_attention_ip(q, k, v, H, Nt, s)
            ref = _ip_ref(q, k, v, H, Nt, s)
            plain = _sdpa(q, k[:, :Nt], v[:, :Nt], H) + s * _sdpa(q, k[:, Nt:], v[:, Nt:], H)
            assert got.shape == (B, Nq, H * 64) and got.dtype == dtype and got.is_contiguous() and bool(torch.isfinite(got).all())
            err, err_p = float((got.float() - ref).abs().max()), float((plain.float() - ref).abs().max())
            rel, rel_p = float((got.float() - ref).norm() / ref.norm()), float((plain.float() - ref).norm() / ref.norm())
            print(f"ip {dtype} B{B} H{H} Nq{Nq} Nt{Nt} Ni{Ni} s{s}: max|err| {err:.2e} (plain {err_p:.2e})  rel {rel:.2e} (plain {rel_p:.2e})")
            assert rel < 1.5 * rel_p + 1e-4, (Ni, s, rel, rel_p)
            assert err < 3.0 * err_p + 4e-3, (Ni, s, err, err_p)
            assert torch.equal(got, ops.flash_attention_ip(q, k.contiguous(), v.contiguous(), H, Nt, s))


# ---- 7. scale 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Nt", [77, 154])
@pytest.mark.parametrize("Ni", [4, 32])
def test_scale_zero_is_the_text_only_kernel_bit_for_bit(dtype, Nt, Ni):
    from elasticdiffusion_official_amd import ops
    for B, H, Nq in ((2, 3, 513), (1, 10, 100)):
        q, k, v = _qkv(B, H, Nq, Nt + Ni, dtype, Nt + Ni)
        assert torch.equal(ops.flash_attention_ip(q, k, v, H, Nt, 0.0), ops.flash_attention(q, k[:, :Nt], v[:, :Nt], H, v_path=8))


# ---- 8. image-only limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_zero_text_values_leave_scale_times_the_image_attention(dtype):
    """v_t = 0: out = rn(scale * (o_i * inv_i)) where the small-KV kernel alone stores rn(o_i * inv_i) -- the two differ by the
    rounding of that stored value times the scale: |d| <= scale * ulp16(x) / 2 + one rounding of the product."""
    from elasticdiffusion_official_amd import ops
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8          # half an ulp, relative
    for Nt, Ni, s in ((77, 4, 0.6), (154, 32, 1.0), (96, 16, 0.6)):
        q, k, v = _qkv(2, 3, 300, Nt + Ni, dtype, 5 * Nt + Ni)
        v = v.clone()
        v[:, :Nt] = 0
        got = ops.flash_attention_ip(q, k, v, 3, Nt, s).float()
        alone = ops.flash_attention(q, k[:, Nt:], v[:, Nt:], 3, v_path=8).float()
        want = s * alone
        # half an ulp of the comparand's own stored value carried through the scale, plus half an ulp of the product (relative
        # eps each, 1 % for second order; 2^-25 each in absolute terms where fp16 is subnormal)
        bound = 2.02 * eps * want.abs() + 2.0 ** -24
        assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() - bound).max())
        if s == 1.0:
            assert torch.equal(got, alone)


# ---- 9. never reads past the keys ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Nt", [129, 154])
@pytest.mark.parametrize("Ni", [4, 31])
def test_decoupled_cross_attention_never_reads_past_the_keys(dtype, Nt, Ni):
    """K and V at the END of an allocation whose tail is NaN / Inf (test_streaming_cross_attention_never_reads_past_the_keys'
    layout): both the text blocks and the image block have masked rows, which must come from the row check, not from memory."""
    from elasticdiffusion_official_amd import ops
    B, H, Nq, N = 2, 3, 256, Nt + Ni
    g = torch.Generator(device=DEV).manual_seed(N)
    tail = 3 * 64 * H * 64
    pool = torch.empty(2, B * N * H * 64 + tail, device=DEV, dtype=dtype)
    pool[:, B * N * H * 64:] = float("nan")
    pool[:, B * N * H * 64::2] = float("inf")
    k, v = (pool[i, :B * N * H * 64].view(B, N, H * 64) for i in range(2))
    k.copy_(torch.randn(B, N, H * 64, device=DEV, generator=g))
    v.copy_(torch.randn(B, N, H * 64, device=DEV, generator=g))
    q = torch.randn(B, Nq, H * 64, device=DEV, generator=g).to(dtype)
    got = ops.flash_attention_ip(q, k, v, H, Nt, 0.6)
    assert bool(torch.isfinite(got).all())
    assert float((got.float() - _ip_ref(q, k, v, H, Nt, 0.6)).abs().max()) < 1.6 * (3e-2 if dtype == torch.bfloat16 else 6e-3)


# ---- 10. rejections -----------------------------------------------------------------------------------------------------
def test_shapes_outside_the_kernel_are_rejected_and_the_next_launch_is_clean():
    from elasticdiffusion_official_amd import ops
    q = torch.randn(1, 64, 128, device=DEV).half()
    kv = torch.randn(1, 200, 128, device=DEV).half()
    for n, nt in ((161 + 4, 161), (77, 77), (77 + 33, 77)):            # Nt = 161; Ni = 0; Ni = 33
        with pytest.raises(RuntimeError):
            ops.flash_attention_ip(q, kv[:, :n], kv[:, :n], 2, nt, 1.0)
    q40, kv40 = torch.randn(1, 64, 80, device=DEV).half(), torch.randn(1, 81, 80, device=DEV).half()
    with pytest.raises(RuntimeError):
        ops.flash_attention_ip(q40, kv40, kv40, 2, 77, 1.0)             # head dimension 40
    # the C entry point refuses the same shapes by itself, before any launch
    from elasticdiffusion_official_amd import _hip
    out = torch.empty_like(q)
    for nt, ni, hd in ((161, 4, 64), (77, 0, 64), (77, 33, 64), (77, 4, 40)):
        err = _hip.lib().ed_flash_attention_ip(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), out.data_ptr(), 1, 1, 2, 64, nt, ni, hd,
                                               q.stride(0), q.stride(1), kv.stride(0), kv.stride(1), kv.stride(0), kv.stride(1),
                                               out.stride(0), out.stride(1), 0.125, 1.0, torch.cuda.current_stream().cuda_stream)
        assert err != 0, (nt, ni, hd)
    torch.cuda.synchronize()
    k = kv[:, :81].contiguous()
    got = ops.flash_attention_ip(q, k, k, 2, 77, 1.0)
    torch.cuda.synchronize()
    assert float((got.float() - _ip_ref(q, k, k, 2, 77, 1.0)).abs().max()) < 1.2e-2


# ---- 11. dispatch -------------------------------------------------------------------------------------------------------
def _attention_with_adapter(dim, heads, head_dim, cross, ni, scale, seed):
    from elasticdiffusion_official_amd import models as M
    torch.manual_seed(seed)
    a = M.Attention(dim, heads, head_dim, cross_dim=cross)
    a.set_ip_adapter(torch.nn.Linear(cross, heads * head_dim, bias=False), torch.nn.Linear(cross, heads * head_dim, bias=False), ni)
    a.ip_scale = scale
    return a.eval().requires_grad_(False)


@pytest.mark.parametrize("head_dim,want", [(64, {"ed_flash_attention_ip": 1}), (40, {"ed_flash_attention": 2})])
def test_attention_module_takes_one_fused_launch_where_the_kernel_applies(head_dim, want):
    from elasticdiffusion_official_amd import ops
    heads = 10 if head_dim == 64 else 8
    a32 = _attention_with_adapter(heads * head_dim, heads, head_dim, 64, 4, 0.8, 3)
    a16 = copy.deepcopy(a32).to(DEV, torch.float16)
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(2, 4096, heads * head_dim, device=DEV, generator=g).half()
    ctx = torch.randn(2, 77 + 4, 64, device=DEV, generator=g).half()
    seen, orig = {}, ops._call

    def spy(name, *a):
        if name.startswith("ed_flash_attention"):
            seen[name] = seen.get(name, 0) + 1
        return orig(name, *a)
    ops._call = spy
    try:
        with torch.no_grad():
            got = a16(x, ctx)
            hoisted = a16(x, ctx, kv=a16.project_kv(ctx))
    finally:
        ops._call = orig
    assert seen == {k: 2 * n for k, n in want.items()}, seen           # (two forwards)
    assert torch.equal(got, hoisted)
    with torch.no_grad():
        ref = a32.to(DEV)(x.float(), ctx.float())                       # fp32: the plain torch path
    assert float((got.float() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())


# ---- 12. CLIP input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PICTURES))
def test_u8_to_clip_input_equals_its_cpu_restatement(name):
    from elasticdiffusion_official_amd import ops
    u8 = torch.from_numpy(picture(name)).to(DEV)
    size = ops.clip_resize_size(*u8.shape[:2])
    resized = ops.resize_u8(u8, size, "bicubic")
    assert torch.equal(resized.cpu(), torch.from_numpy(C.pil_resize(picture(name)).copy()))       # Pillow's bytes
    got = ops.u8_to_clip_input(resized)
    want = C.u8_to_clip_input(resized.cpu())
    assert got.shape == (1, 3, 224, 224) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    with pytest.raises(RuntimeError):
        ops.u8_to_clip_input(resized[:100])                               # smaller than the crop


# ---- 13. forward --------------------------------------------------------------------------------------------------------
def _adapter_for(sd, dtype=torch.float32, gain=4.0, seed=5):
    from elasticdiffusion_official_amd import models as M
    cfg = M.SMALL_UNET_CONFIGS["sdxl" if sd.startswith("XL") else "sd15"]
    return IS.random_adapter(cfg, NI, CLIP_DIM, seed=seed, dtype=dtype, gain=gain), cfg


def test_real_architecture_forward_with_adapter(monkeypatch):
    """One fp16 6-row forward of the reduced-width XL UNet with an adapter on 77 + 4 and 154 + 4 tokens against its fp32 CPU
    forward: rel-L2 at most twice the same forward's text-only figure (test_real_architecture_forward_on_two_and_three_chunks'
    factor, under cudnn.deterministic); hoisted k|v and TEXT_KV_ONCE = False agree as they do without an adapter; a ControlNet
    sees the text tokens alone."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    sd = "XL1.0"
    unet, vae, cn = R.build_small(sd, controlnet=True)
    adapter, cfg = _adapter_for(sd)
    S = unet.config.sample_size // 2       # a 64 x 64 latent: 1024 and 256 queries at the two attention levels, CPU side in seconds
    g = torch.Generator().manual_seed(21)
    x = torch.randn(6, 4, S, S, generator=g)
    text = torch.randn(6, 154, 64, generator=g)
    pooled = torch.randn(6, 32, generator=g)
    embeds = torch.randn(6, CLIP_DIM, generator=g)
    t = torch.tensor(500)
    kw = {"added_cond_kwargs": {"text_embeds": pooled, "time_ids": torch.zeros(6, 6)}}
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    pipe = ElasticDiffusion(DEV, sd, view_batch_size=4, unet=copy.deepcopy(unet).to(torch.float16), vae=copy.deepcopy(vae),
                            controlnet=copy.deepcopy(cn).to(torch.float16), text_encoder=lambda s: None, use_graphs=False)

    def forwards(txt, cond=None):
        outs = []
        for once in (True, False):
            pipe.TEXT_KV_ONCE = once
            txt16 = txt.to(DEV, torch.float16)
            kv = pipe._text_kv(txt16)
            assert (kv is not None) == once
            outs.append(pipe._forward_rows(x.to(DEV, torch.float16), t.to(DEV), txt16, pooled.to(DEV, torch.float16), cond, kv).float().cpu())
        return outs

    rel0, hoist0 = {}, {}
    with torch.no_grad():
        for n in (77, 154):
            txt = text[:, :n].contiguous()
            outs = forwards(txt)
            rel0[n] = R.rel_l2(outs[0], unet(x, t, encoder_hidden_states=txt, **kw)["sample"])
            hoist0[n] = R.rel_l2(outs[1], outs[0])
        assert pipe.load_ip_adapter(adapter, scale=0.8) == "ip_adapter" and pipe.ip_adapter == ("ip_adapter", 0.8, NI)
        unet.install_ip_adapter(adapter)
        unet.ip_scale = 0.8
        tokens = unet.ip_image_tokens(embeds)
        for n in (77, 154):
            txt = torch.cat([text[:, :n], tokens], dim=1).contiguous()
            want = unet(x, t, encoder_hidden_states=txt, **kw)["sample"]
            outs = forwards(txt)
            assert bool(torch.isfinite(outs[0]).all())
            rel, hoist = R.rel_l2(outs[0], want), R.rel_l2(outs[1], outs[0])
            print(f"real-arch {sd} fp16 forward with adapter on {n}+{NI} tokens vs fp32 CPU: rel-L2 {rel:.3e} (text-only {rel0[n]:.3e}); "
                  f"hoisted vs in-forward k|v {hoist:.3e} (text-only {hoist0[n]:.3e})")
            assert rel <= 2.0 * rel0[n], (n, rel, rel0[n])
            assert hoist <= 2.0 * hoist0[n], (n, hoist, hoist0[n])
        # ControlNet: handed the text part only, directly and through its hoisted k|v
        cond = torch.rand(6, 3, 8 * S, 8 * S, generator=g).to(DEV, torch.float16)
        pipe._cn_scale = 0.5
        seen, fwd = [], pipe.controlnet.forward

        def spy(*a, **k):
            out = fwd(*a, **k)
            seen.append((tuple(k["encoder_hidden_states"].shape), out))
            return out
        pipe.controlnet.forward = spy
        txt = torch.cat([text[:, :77], tokens], dim=1).contiguous()
        with_cn = forwards(txt, cond)
        pipe.controlnet.forward = fwd
        assert [s[0] for s in seen] == [(6, 77, 64)] * 2
        txt16 = text[:, :77].contiguous().to(DEV, torch.float16)
        down, mid = pipe.controlnet(x.to(DEV, torch.float16), t.to(DEV), encoder_hidden_states=txt16, controlnet_cond=cond,
                                    conditioning_scale=0.5, added_cond_kwargs={"text_embeds": pooled.to(DEV, torch.float16),
                                                                               "time_ids": torch.zeros(6, 6, device=DEV, dtype=torch.float16)})
        for _, (d, m) in seen[1:]:                                       # (the in-forward projection: the same calls as here)
            assert torch.equal(m, mid) and all(torch.equal(a, b) for a, b in zip(d, down))
        assert R.rel_l2(seen[0][1][1], mid) <= max(2.0 * hoist0[77], 1e-6)
        assert R.rel_l2(with_cn[1], with_cn[0]) <= max(4.0 * hoist0[77], 1e-6)


# ---- 14. loop -----------------------------------------------------------------------------------------------------------
def _ip_embed_fn(xl, un_tok, co_tok):
    base = R.embed_fn(xl)
    state = {"n": 0}

    def fn(p):
        e, pooled = base(p)
        state["n"] += 1
        tok = un_tok if state["n"] % 2 == 1 else co_tok
        return torch.cat([e, tok.to(e.dtype)], dim=1), pooled
    return fn


@pytest.mark.parametrize("case", ["cfg2_sd_512x1024", "cfg3_xl_1024x2048"])
def test_product_loop_with_adapter_against_the_oracle(case):
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = R.REAL_CASES[case]          # (3 steps for the SD 1.5 geometry, 2 for the XL one)
    xl = c["sd"].startswith("XL")
    unet, vae, _ = R.build_small(c["sd"])
    adapter, cfg = _adapter_for(c["sd"])
    embeds = torch.randn(1, CLIP_DIM, generator=torch.Generator().manual_seed(8))
    run = dict(height=c["H"], width=c["W"], num_inference_steps=c["steps"], resampling_steps=c["R"], **R.LOOP_KW)
    # oracle: the same UNet with the adapter on the CPU, the embed function returns [text | image tokens]
    cpu = copy.deepcopy(unet)
    cpu.install_ip_adapter(adapter)
    cpu.ip_scale = 1.0
    orc = ElasticOracle(cpu, vae, DDIMOracle(), _ip_embed_fn(xl, cpu.ip_image_tokens(torch.zeros_like(embeds)), cpu.ip_image_tokens(embeds)),
                        sd_version=c["sd"], view_batch_size=c["vbs"], pooled_dim=32 if xl else None)
    orc.seed_everything(c["seed"])
    want = []
    orc.generate_latent("p", "", trace=want, **run)
    tail = torch.rand(4)

    pipe = ElasticDiffusion(DEV, c["sd"], view_batch_size=c["vbs"], unet=copy.deepcopy(unet), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(xl))

    def product(**kw):
        pipe.text_encoder = R.embed_fn(xl)
        pipe.seed_everything(c["seed"])
        trace = []
        pipe.generate_latents("p", "", trace=trace, **run, **kw)
        return [z.cpu() for z in trace], torch.rand(4)
    text_only, _ = product()
    pipe.load_ip_adapter(adapter, scale=1.0)
    got, t1 = product(ip_adapter_image_embeds=embeds)
    rels = [R.rel_l2(a, b) for a, b in zip(got, want)]
    print(f"{case} fp32 loop with adapter vs oracle, per step: {['%.2e' % r for r in rels]}")
    assert len(got) == len(want) == c["steps"] and max(rels) < 1e-3, rels
    assert torch.equal(t1, tail)
    pipe.set_ip_adapter_scale(0.0)
    zero, _ = product(ip_adapter_image_embeds=embeds)
    d0, d1 = R.rel_l2(zero[-1], text_only[-1]), R.rel_l2(got[-1], text_only[-1])
    print(f"{case}: scale 0 vs text-only {d0:.2e}, scale 1 vs text-only {d1:.2e}")
    assert d0 < 1e-5 and d1 > 1e-3
    assert pipe._runner.stats()["eager"] == 0


# ---- 15. graphs, 16. interleaved ----------------------------------------------------------------------------------------
SMALL_RUN = dict(height=512, width=512, num_inference_steps=2, guidance_scale=10.0, resampling_steps=1, new_p=0.3, rrg_stop_t=0.4,
                 rrg_init_weight=1000, cosine_scale=10.0, repaint_sampling=True)


def _small_pipe(dtype=torch.float16):
    from elasticdiffusion_official_amd import ElasticDiffusion
    unet, vae, _ = R.build_small("1.5")
    return ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=copy.deepcopy(unet).to(dtype), vae=copy.deepcopy(vae),
                            text_encoder=R.embed_fn(False))


def test_adapter_images_replay_graphs_and_leave_nothing_behind(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)    # bit equality across captures
    pipe = _small_pipe()
    adapter, _ = _adapter_for("1.5")
    embeds = torch.randn(1, CLIP_DIM, generator=torch.Generator().manual_seed(8))

    def run(**kw):
        pipe.text_encoder = R.embed_fn(False)
        pipe.seed_everything(3)
        return pipe.generate_latents("p", "", **SMALL_RUN, **kw).clone()
    first = run()
    pipe.load_ip_adapter(adapter, scale=0.7)
    a1 = run(ip_adapter_image_embeds=embeds)
    pipe.set_ip_adapter_scale(0.3)
    other = run(ip_adapter_image_embeds=embeds)
    pipe.set_ip_adapter_scale(0.7)
    a2 = run(ip_adapter_image_embeds=embeds)
    assert pipe.ip_adapter == ("ip_adapter", 0.7, NI)
    assert pipe._runner.stats()["eager"] == 0 and pipe._runner.stats()["captured"] >= 1
    assert torch.equal(a1, a2) and not torch.equal(a1, other) and R.rel_l2(a1, first) > 1e-3
    with pytest.raises(ValueError, match="unload_ip_adapter"):
        run()
    pipe.unload_ip_adapter()
    assert pipe.ip_adapter is None and pipe.unet.ip_tokens == 0
    assert torch.equal(run(), first)
    assert pipe._runner.stats()["eager"] == 0
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        run(ip_adapter_image_embeds=embeds)


def test_image_prompt_through_an_image_encoder_callable(monkeypatch):
    """ip_adapter_image: one upload, the resize / crop / normalise on the device, then the image_encoder callable"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    pipe = _small_pipe()
    adapter, _ = _adapter_for("1.5")
    proj = torch.randn(CLIP_DIM, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen = []

    def encoder(pixels):
        seen.append(pixels)
        return pixels.mean((2, 3)) @ proj.t()
    pipe.load_ip_adapter(adapter, scale=1.0, image_encoder=encoder)
    u8 = picture("landscape")
    pipe.seed_everything(3)
    a = pipe.generate_latents("p", "", ip_adapter_image=torch.from_numpy(u8), **SMALL_RUN).clone()
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), C.u8_to_clip_input(torch.from_numpy(C.pil_resize(u8).copy())))
    pipe.text_encoder = R.embed_fn(False)
    pipe.seed_everything(3)
    b = pipe.generate_latents("p", "", ip_adapter_image_embeds=encoder(seen[0]), **SMALL_RUN)
    assert torch.equal(a, b)


def test_interleaved_jobs_with_their_own_image_prompts():
    pipe = _small_pipe(torch.float32)
    adapter, _ = _adapter_for("1.5")
    pipe.load_ip_adapter(adapter, scale=1.0)
    g = torch.Generator().manual_seed(8)
    jobs = [dict(prompts="p", seed=11, ip_adapter_image_embeds=torch.randn(1, CLIP_DIM, generator=g)),
            dict(prompts="q", seed=12, ip_adapter_image_embeds=torch.randn(1, CLIP_DIM, generator=g))]
    alone = []
    for j in jobs:
        pipe.text_encoder = R.embed_fn(False)
        pipe.seed_everything(j["seed"])
        alone.append(pipe.generate_latents(j["prompts"], "", ip_adapter_image_embeds=j["ip_adapter_image_embeds"], **SMALL_RUN).clone())
    assert R.rel_l2(alone[0], alone[1]) > 1e-3
    pipe.text_encoder = R.embed_fn(False)
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **SMALL_RUN)
    for z, want in zip(got, alone):
        assert R.rel_l2(z, want) < 1e-5, R.rel_l2(z, want)
    with pytest.raises(RuntimeError, match="in flight"):
        pipe._live_jobs = [1]
        try:
            pipe.set_ip_adapter_scale(0.5)
        finally:
            pipe._live_jobs = None
    with pytest.raises(ValueError, match="every job"):
        pipe.generate_latents_interleaved([jobs[0], dict(prompts="q", seed=12)], in_flight=2, **SMALL_RUN)


# ---- 17. command line ---------------------------------------------------------------------------------------------------
def test_command_line_takes_the_adapter_flags(tmp_path):
    from safetensors.torch import save_file
    from elasticdiffusion_official_amd import models as M
    cfg = M.UNET_CONFIGS[M.family("1.5")]
    adapter = IS.random_adapter(cfg, NI, CLIP_DIM, seed=1, dtype=torch.float16)
    save_file({k: v.contiguous() for k, v in adapter.items()}, str(tmp_path / "ip.safetensors"))
    torch.save(torch.randn(1, CLIP_DIM, generator=torch.Generator().manual_seed(2)), str(tmp_path / "e.pt"))
    r = procs.run([procs.PY, "-m", "elasticdiffusion_official_amd", "--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "2",
                   "--resampling_steps", "1", "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--view_batch_size", "4",
                   "--ip_adapter", f"{tmp_path / 'ip.safetensors'}:0.7", "--ip_adapter_embeds", str(tmp_path / "e.pt")],
                  timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "installed at scale 0.7: 4 image tokens" in r.stdout
    saved = glob.glob(os.path.join(str(tmp_path), "t", "*"))
    assert len(saved) == 1 and os.path.exists(os.path.join(saved[0], "0.png"))
    args = open(os.path.join(saved[0], "args.txt")).read()
    assert f"ip_adapter: {tmp_path / 'ip.safetensors'}:0.7" in args and f"ip_adapter_embeds: {tmp_path / 'e.pt'}" in args
    assert "ip_adapter_image: None" in args and "image_encoder: None" in args
