"""-m gpu: LoRA adapters merged into the weights.

Kernel (``ed_lora_merge``), ONE table of five tensors -- [8, 8] r = 1; [70, 37] with r = 3 and r = 16 (one negative scale); [1, 5]
r = 4; [130, 64] r = 33; a channels-last [64, 16, 3, 3] convolution weight with r = 130 and r = 2 -- in fp32, fp16 and bf16:
  1. fp32: |W - merged_fp64| <= (r_max + J + 2) * 2^-24 * (|base| + sum |c| |up| |down|), elementwise (tests/lora_cpu.fp32_bound);
  2. 16-bit: torch.equal to the kernel's own fp32 result of the same base, cast once;
  3. every tensor alone in a one-entry table, and a second launch of the table: the same bits;
  4. a tensor whose adapters are all at scale 0 (left out by the host), and every tensor of a table without adapters: the base's bits;
  5. tables the entry point must refuse, before any launch.
Pipeline, reduced-width SD 1.5 UNet: after ``load_lora`` / ``set_lora_scale`` / a second adapter / ``unload_lora`` on a pipeline
that has captured graphs and built derived weights, the merged Parameters are the fp64 statement's rounded once, a fresh
pipeline given clones of them derives bit-equal fused weights, and the latents of the two are held to rel-L2 <= 1e-5 (the suite's
bar for "interleaved equals alone"; both pipelines with the library convolutions in their deterministic algorithms, without which
the fp16 loop differs from ITSELF by 5e-3 run to run, adapter or not).
"""
import copy
import os

import pytest
import torch

from tests import lora_cpu as C
from tests import realarch as R
from tests.fakes import FakeUNet, FakeVAE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# (logical weight shape, channels-last?, [(rank, scale, alpha)])
TENSORS = [
    ((8, 8), False, [(1, 1.0, None)]),
    ((70, 37), False, [(3, 0.8, 1.0), (16, -0.6, None)]),
    ((1, 5), False, [(4, 1.3, 2.0)]),
    ((130, 64), False, [(33, 0.5, None)]),
    ((64, 16, 3, 3), True, [(130, 0.7, 64.0), (2, 1.0, None)]),
]


def _logical(i):
    """CPU fp32 base and logical factors [(up, down, c)] of tensor i (seeded, dtype-independent)"""
    shape, _, ads = TENSORS[i]
    g = torch.Generator().manual_seed(100 + i)
    base = torch.randn(*shape, generator=g)
    out = []
    for j, (r, scale, alpha) in enumerate(ads):
        up, down = C.random_factors(shape, r, 1000 + 10 * i + j)
        out.append((up, down, C.coefficient(scale, alpha, r)))
    return base, out


def _rows(dtype, base_dtype=None, only=None, zero=(), no_adapters=False):
    """Device rows for ``lora.LoraTable``: base rounded to ``base_dtype`` (default ``dtype``) and held in ``dtype``; the destination is
    poisoned; an index in ``zero`` has all its adapters at scale 0, so the host leaves them out."""
    from elasticdiffusion_official_amd import lora
    rows = []
    for i in (range(len(TENSORS)) if only is None else only):
        base, ads = _logical(i)
        base = base.to(base_dtype or dtype).to(dtype)
        if TENSORS[i][1]:
            base = base.contiguous(memory_format=torch.channels_last)
        base = base.to(DEV)
        dst = torch.full_like(base, float("nan"))
        assert dst.stride() == base.stride()
        dev_ads = []
        for up, down, c in ads:
            u, d = lora.factors(lora.LoraTarget("unet", f"t{i}", up, down, None), base)
            if i not in zero and not no_adapters:
                dev_ads.append((u.to(DEV), d.to(DEV), float(c)))
        rows.append((base, dst, dev_ads))
    return rows


def _merge(rows):
    from elasticdiffusion_official_amd import lora, ops
    table = lora.LoraTable(rows).upload(DEV)
    ops.lora_merge(table)
    torch.cuda.synchronize()
    return table


@pytest.fixture(scope="module")
def merged():
    """{(dtype name, base dtype name): [W of each tensor, on the CPU]} from one five-tensor launch each"""
    out = {}
    for name, base in (("fp32", "fp32"), ("fp32", "fp16"), ("fp32", "bf16"), ("fp16", "fp16"), ("bf16", "bf16")):
        rows = _rows(DTYPES[name], DTYPES[base])
        table = _merge(rows)
        assert (table.n_tensors, table.n_adapters) == (5, 7)
        assert table.n_tiles == 1 + 2 * 1 + 1 + 3 * 1 + 1 * 2
        out[(name, base)] = [dst.cpu() for _, dst, _ in rows]
    return out


def test_fp32_merge_within_the_forward_bound(merged):
    worst = 0.0
    for i in range(len(TENSORS)):
        base, ads = _logical(i)
        want, bound = C.merged_fp64(base, ads), C.fp32_bound(base, ads)
        got = merged[("fp32", "fp32")][i]
        assert got.shape == base.shape and bool(torch.isfinite(got).all())
        ratio = float(((got.double() - want).abs() / bound).max())
        print(f"tensor {i} {tuple(base.shape)}: worst |W - fp64| / bound = {ratio:.3f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (i, ratio)
        assert float((want - base.double()).abs().max()) > 1e-2      # the adapters moved the weight: the bound is not vacuous
    print(f"worst ratio {worst:.3f}")


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_16bit_destination_is_one_rounding_of_the_fp32_result(merged, name):
    for i in range(len(TENSORS)):
        w16, w32 = merged[(name, name)][i], merged[("fp32", name)][i]
        assert w16.dtype == DTYPES[name] and torch.equal(w16, w32.to(DTYPES[name])), i
        assert w16.stride() == w32.stride()


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_table_independence_and_repeatability(merged, name):
    dt = DTYPES[name]
    for i in range(len(TENSORS)):
        rows = _rows(dt, only=[i])
        _merge(rows)
        assert torch.equal(rows[0][1].cpu(), merged[(name, name)][i]), i
    rows = _rows(dt)
    table = _merge(rows)
    first = [dst.clone() for _, dst, _ in rows]
    from elasticdiffusion_official_amd import ops
    ops.lora_merge(table)
    torch.cuda.synchronize()
    assert all(torch.equal(a, dst) for a, (_, dst, _) in zip(first, rows))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(first, merged[(name, name)]))


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_scale_zero_and_unload_restore_the_bits(merged, name):
    dt = DTYPES[name]
    for z in (1, 4):                                   # the two-adapter tensors: the row tensor and the convolution
        rows = _rows(dt, zero=(z,))
        table = _merge(rows)
        assert table.n_adapters == 7 - 2
        for i, (base, dst, _) in enumerate(rows):
            if i == z:
                assert torch.equal(dst, base)
            else:
                assert torch.equal(dst.cpu(), merged[(name, name)][i]), i
    rows = _rows(dt, no_adapters=True)                 # what unload_lora launches: every tensor restored by the copy path
    for base, _, _ in rows:
        base[(0,) * base.dim()] = -0.0                 # a bit pattern that base + 0 would not keep
    table = _merge(rows)
    assert table.n_adapters == 0
    for base, dst, _ in rows:
        assert torch.equal(dst, base) and torch.equal(torch.signbit(dst), torch.signbit(base))


def test_rejected_tables_launch_nothing():
    from elasticdiffusion_official_amd import lora, ops
    rows = _rows(torch.float16)
    good = lora.LoraTable(rows)
    T, A = 8, 4
    a0 = T * good.n_tensors
    pokes = {
        "null base": (0, 0), "null destination": (T + 1, 0), "null up": (a0, 0), "null down": (a0 + A + 1, 0),
        "rank 0": (a0 + 2, 0), "negative rank": (a0 + 2 * A + 2, -3), "dtype code": (2 * T + 4, 7), "N = 0": (T + 2, 0),
        "odd 16-bit pointer": (3 * T, int(good.host[3 * T]) + 1), "adapter range": (T + 5, 0), "tile prefix": (2 * T + 7, 1),
        "non-finite coefficient": (a0 + 3, 0x7F800000), "coefficient high bits": (a0 + 3, 1 << 40),
    }
    for what, (word, value) in pokes.items():
        table = lora.LoraTable(rows)
        table.host[word] = value
        table.upload(DEV)
        with pytest.raises(RuntimeError, match="ed_lora_merge"):
            ops.lora_merge(table)
        assert ops._LAUNCH["device"] is None, what
    for n_tiles in (0, good.n_tiles - 1, good.n_tiles + 1):
        table = lora.LoraTable(rows).upload(DEV)
        table.n_tiles = n_tiles
        with pytest.raises(RuntimeError, match="ed_lora_merge"):
            ops.lora_merge(table)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(dst).all()) for _, dst, _ in rows)      # nothing was written
    # the wrapper's own checks: a table that is not on the device, tensors that do not fit their factors
    table = lora.LoraTable(rows)
    table.dev = table.host
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lora_merge(table)
    table = lora.LoraTable(rows).upload(DEV)
    table.keep[3] = (rows[3][0], rows[3][1], [(rows[1][2][0][0], rows[3][2][0][1], 1.0)])
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.lora_merge(table)
    assert ops._LAUNCH["device"] is None
    # and the launch state is clean: the good table still merges
    _merge(rows)
    assert all(bool(torch.isfinite(dst).all()) for _, dst, _ in rows)


# ---- pipeline ------------------------------------------------------------------------------------------------------------------
CASE = dict(sd="1.5", H=512, W=512, vbs=4, steps=2, R=1, seed=3)
BAR = 1e-5          # the suite's bar for "the same computation through another route" (interleaved equals alone)
BLOCK = "down_blocks.1.attentions.0"
TARGETS = [f"{BLOCK}.transformer_blocks.0.attn1.to_q", f"{BLOCK}.transformer_blocks.0.attn1.to_k",
           f"{BLOCK}.transformer_blocks.0.attn1.to_v", f"{BLOCK}.transformer_blocks.0.attn1.to_out.0",
           f"{BLOCK}.transformer_blocks.0.attn2.to_q", f"{BLOCK}.transformer_blocks.0.attn2.to_k",
           f"{BLOCK}.transformer_blocks.0.attn2.to_v", f"{BLOCK}.transformer_blocks.0.ff.net.0.proj",
           "mid_block.attentions.0.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.0.attn2.to_v",
           "down_blocks.0.resnets.1.conv1", f"{BLOCK}.proj_in"]


@pytest.fixture(scope="module")
def world():
    unet, vae, _ = R.build_small(CASE["sd"])
    mods = dict(unet.named_modules())
    adapters = {}
    for k, (rank, alpha, seed, paths) in enumerate([(4, 2.0, 11, TARGETS), (6, None, 12, TARGETS[::2])]):
        adapters[f"a{k}"] = [("unet", p, *[t * 0.5 for t in C.random_factors(tuple(mods[p].weight.shape), rank, seed + i)], alpha)
                             for i, p in enumerate(paths)]
    return dict(unet=unet, vae=vae, adapters=adapters)


def _pipe(world, unet=None, dtype=torch.float16):
    from elasticdiffusion_official_amd import ElasticDiffusion
    u = copy.deepcopy(world["unet"]).to(dtype) if unet is None else unet
    return ElasticDiffusion(DEV, CASE["sd"], view_batch_size=CASE["vbs"], unet=u, vae=copy.deepcopy(world["vae"]),
                            text_encoder=R.embed_fn(False))


def _run(pipe):
    pipe.seed_everything(CASE["seed"])
    return pipe.generate_latents("p", "", height=CASE["H"], width=CASE["W"], num_inference_steps=CASE["steps"],
                                 resampling_steps=CASE["R"], **R.LOOP_KW).float().cpu()


def _derived(unet):
    return {(n, slot): v[1] for n, m in unet.named_modules() for slot, v in m.__dict__.get("_derived", {}).items()}


def _flat(x):
    return [x] if isinstance(x, torch.Tensor) else [t for t in x if isinstance(t, torch.Tensor)]


def _check_against_fresh(world, pipe, z, originals, active):
    """``pipe`` (graphs captured, derived weights built before the change) against a fresh pipeline on clones of its merged
    Parameters; ``active`` = [(adapter key, scale)] is what the merged weights must be by the fp64 statement.  Returns the rel-L2
    of ``z`` against the fresh pipeline's latent."""
    mods = dict(pipe.unet.named_modules())
    half = 2.0 ** -11 if pipe.model_dtype == torch.float16 else 2.0 ** -24      # half an ulp of the weight's type, relative
    touched = {}
    for key, scale in active:
        for _, path, up, down, alpha in world["adapters"][key]:
            touched.setdefault(path, []).append((up, down, C.coefficient(scale, alpha, up.shape[1])))
    for path, ads in touched.items():
        w = mods[path].weight.detach().float().cpu()
        base = originals[path + ".weight"].float().cpu()
        want, mag = C.merged_fp64(base, ads), C.magnitude(base, ads)
        r_max = max(a[0].shape[1] for a in ads)
        # one rounding to the weight's type (half an ulp; 2^-25 absolute in fp16's subnormal range) of an fp32 sum inside its bound
        tol = half * want.abs() + 2.0 ** -25 + (r_max + len(ads) + 2) * 2.0 ** -24 * mag
        assert bool(((w.double() - want).abs() <= tol).all()), path
        assert not torch.equal(w, base), path
    ref_unet = copy.deepcopy(pipe.unet)
    for m in ref_unet.modules():
        m.__dict__.pop("_derived", None)
    ref = _pipe(world, ref_unet)
    assert ref.model_dtype == pipe.model_dtype
    zr = _run(ref)
    sd_p, sd_r = pipe.unet.state_dict(), ref.unet.state_dict()
    assert all(torch.equal(sd_p[k], sd_r[k]) and sd_p[k].data_ptr() != sd_r[k].data_ptr() for k in sd_p)
    dp, dr = _derived(pipe.unet), _derived(ref.unet)
    assert dp.keys() == dr.keys() and any("to_k" in str(slot) for _, slot in dp)
    for k in dp:
        assert all(torch.equal(a, b) for a, b in zip(_flat(dp[k]), _flat(dr[k]))), k
    return R.rel_l2(z, zr)


SCENARIOS = {
    "load": [("load", "a0", 1.0)],
    "rescale": [("load", "a0", 1.0), ("scale", None, 0.5)],
    "two adapters": [("load", "a0", 0.8), ("load", "a1", -0.6)],
    "one of two rescaled to zero": [("load", "a0", 0.8), ("load", "a1", 1.0), ("scale", "a1", 0.0)],
}


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_weights_and_derived_weights_after_a_change(world, scenario, tmp_path):
    """fp16 UNet: the merged Parameters are the fp64 statement's, rounded once; a fresh pipeline on clones of them derives bit-equal
    fused weights; the latents moved.  (How close the latents of the two pipelines are is the next test's subject.)"""
    from safetensors.torch import save_file
    pipe = _pipe(world)
    originals = {k: v.clone() for k, v in pipe.unet.state_dict().items()}
    z0 = _run(pipe)                                     # graphs captured, fused q|k|v and k|v weights derived
    assert pipe.loras == [] and _derived(pipe.unet) and pipe._runner.entries
    active = {}
    for i, (op, key, scale) in enumerate(SCENARIOS[scenario]):
        if op == "load":
            path = str(tmp_path / f"{key}.safetensors")
            save_file(C.write_kohya(world["adapters"][key]) if i else C.write_peft(world["adapters"][key]), path)
            assert pipe.load_lora(path, scale) == key
            active[key] = scale
        else:
            pipe.set_lora_scale(scale, key)
            for k in ([key] if key else list(active)):
                active[k] = scale
        assert not pipe._runner.entries
    assert pipe.loras == [(k, s, len(world["adapters"][k])) for k, s in active.items()]
    z = _run(pipe)
    err = _check_against_fresh(world, pipe, z, originals, [(k, s) for k, s in active.items() if s != 0])
    moved = R.rel_l2(z, z0)
    print(f"{scenario}: rel-L2 against the fresh pipeline {err:.3e}, against the no-adapter latent {moved:.3e}")
    assert moved >= 100 * BAR, moved
    # untouched tensors kept their bits
    touched = {p + ".weight" for k in active for _, p, *_ in world["adapters"][k]}
    assert all(torch.equal(v, originals[k]) for k, v in pipe.unet.state_dict().items() if k not in touched)


def test_unload_restores_weights_and_frees_the_copies(world):
    pipe = _pipe(world)
    originals = {k: v.clone() for k, v in pipe.unet.state_dict().items()}
    z0 = _run(pipe)
    pipe.load_lora(C.write_peft(world["adapters"]["a0"]), 1.0, name="x")
    pipe.load_lora(C.write_legacy(world["adapters"]["a1"]), 0.5, name="y")
    with pytest.raises(ValueError, match="already loaded"):
        pipe.load_lora(C.write_peft(world["adapters"]["a0"]), 1.0, name="x")
    assert len(pipe._lora.bases) == len(TARGETS)
    pipe.unload_lora("x")
    assert [l[0] for l in pipe.loras] == ["y"] and len(pipe._lora.bases) == len(TARGETS[::2])
    only_y = {p + ".weight" for _, p, *_ in world["adapters"]["a1"]}
    assert all(torch.equal(v, originals[k]) == (k not in only_y) for k, v in pipe.unet.state_dict().items())
    pipe.set_lora_scale(0.0)
    assert all(torch.equal(v, originals[k]) for k, v in pipe.unet.state_dict().items())
    pipe.set_lora_scale(0.5)
    pipe.unload_lora()
    assert pipe.loras == [] and pipe._lora.bases == {} and not pipe._runner.entries
    assert all(torch.equal(v, originals[k]) for k, v in pipe.unet.state_dict().items())
    assert bool(torch.isfinite(_run(pipe)).all()) and bool(torch.isfinite(z0).all())
    with pytest.raises(KeyError):
        pipe.unload_lora("x")
    pipe.unload_lora()      # nothing loaded: nothing to do


@pytest.fixture
def deterministic_library_convolutions():
    """The library convolutions in their deterministic algorithms for the duration of a test (PyTorch's switch of that name; on ROCm
    it sets MIOpen's deterministic attribute).  Two runs can only be compared below the 16-bit noise floor when each of them
    repeats itself: with the default algorithm choice two identical forwards of the reduced-width UNet already differ, first at the
    output of a library convolution (``down_blocks.1.resnets.0.conv2`` in fp16, one fp16 ulp; the stride-2 downsampler in fp32,
    2.4e-7), and the same pipeline's second image is 5.2e-3 (fp16) / 2.7e-6 (fp32) from its first with no adapter in play; with the
    switch on both are zero.  It changes which library kernel runs, for both arms of a comparison alike, and nothing in the package."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


@pytest.mark.parametrize("name", ["fp16", "fp32"])
def test_latents_after_a_change_equal_a_fresh_pipeline(world, name, deterministic_library_convolutions):
    """load, generate; set_lora_scale(0.5), generate; a second adapter, generate -- each against a fresh pipeline on clones of the
    merged Parameters -- then unload_lora, generate, against the first run: rel-L2 <= 1e-5 every time, zero expected (a stale derived
    weight or a replayed old graph would show as the 7e-2 .. 1e-1 the adapters move the latent by).  Both pipelines run the library
    convolutions in their deterministic algorithms (the fixture says why); the figures seen are printed."""
    dt = DTYPES[name]
    pipe = _pipe(world, dtype=dt)
    originals = {k: v.clone() for k, v in pipe.unet.state_dict().items()}
    z0 = _run(pipe)
    seen = {}
    pipe.load_lora(C.write_peft(world["adapters"]["a0"]), 1.0, name="a0")
    z1 = _run(pipe)
    seen["load"] = _check_against_fresh(world, pipe, z1, originals, [("a0", 1.0)])
    pipe.set_lora_scale(0.5)
    seen["set_lora_scale(0.5)"] = _check_against_fresh(world, pipe, _run(pipe), originals, [("a0", 0.5)])
    pipe.load_lora(C.write_kohya(world["adapters"]["a1"]), -0.6, name="a1")
    seen["two adapters"] = _check_against_fresh(world, pipe, _run(pipe), originals, [("a0", 0.5), ("a1", -0.6)])
    pipe.unload_lora()
    assert all(torch.equal(v, originals[k]) for k, v in pipe.unet.state_dict().items())
    seen["unload"] = R.rel_l2(_run(pipe), z0)
    moved = R.rel_l2(z1, z0)
    print(f"{name}: rel-L2 " + ", ".join(f"{k} {v:.3e}" for k, v in seen.items()) + f"; the first load moved the latent by {moved:.3e}")
    assert moved >= 100 * BAR
    assert all(v <= BAR for v in seen.values()), seen


def test_no_adapter_no_launch_and_refusals_change_nothing(world):
    from elasticdiffusion_official_amd import ops
    counts = []
    pipe = _pipe(world)
    for stage in range(3):
        if stage == 2:      # after a load and an unload the loop launches what it launched before
            pipe.load_lora(C.write_peft(world["adapters"]["a0"]), 1.0)
            pipe.unload_lora()
        ops.TIMER.start()
        try:
            _run(pipe)
        finally:
            counts.append({k: v[0] for k, v in ops.TIMER.stop().items()})
        if stage == 0:
            assert pipe.loras == [] and "_lora" not in pipe.__dict__
            pipe = _pipe(world)
    assert "ed_lora_merge" not in counts[0] and counts[0] == counts[1] == counts[2], counts
    # a refused file leaves the pipeline as it was: weights, graphs, listing
    before = {k: v.clone() for k, v in pipe.unet.state_dict().items()}
    entries = len(pipe._runner.entries)
    bad = C.write_peft(world["adapters"]["a0"])
    bad["unet.mid_block.attentions.0.proj_in.lora_A.weight"] = torch.zeros(3, 5)
    bad["unet.mid_block.attentions.0.proj_in.lora_B.weight"] = torch.zeros(7, 3)
    ops.TIMER.start()
    try:
        with pytest.raises(RuntimeError, match="do not fit"):
            pipe.load_lora(bad)
        with pytest.raises(RuntimeError, match="text_encoder=False"):       # an injected callable encoder has no CLIP modules
            pipe.load_lora(C.write_kohya([("text_encoder", "text_model.encoder.layers.0.mlp.fc1", torch.zeros(4, 2), torch.zeros(2, 4), None)]))
    finally:
        assert not ops.TIMER.stop()
    assert pipe.loras == [] and len(pipe._runner.entries) == entries
    assert all(torch.equal(v, before[k]) for k, v in pipe.unet.state_dict().items())
    both = dict(C.write_peft(world["adapters"]["a0"]),
                **C.write_kohya([("text_encoder", "text_model.encoder.layers.0.mlp.fc1", torch.zeros(4, 2), torch.zeros(2, 4), None)]))
    pipe.load_lora(both, text_encoder=False)
    assert pipe.loras == [("lora0", 1.0, len(TARGETS))]


def test_change_is_refused_with_images_in_flight(world):
    pipe = _pipe(world)
    pipe.load_lora(C.write_peft(world["adapters"]["a0"]), 1.0, name="a")
    kw = dict(height=CASE["H"], width=CASE["W"], num_inference_steps=CASE["steps"], resampling_steps=CASE["R"], **R.LOOP_KW)
    jobs = [dict(prompts="p", seed=1), dict(prompts="p", seed=2)]
    seen = []

    def on_done(j, latent):
        seen.append(j)
        pipe.set_lora_scale(0.5)

    with pytest.raises(RuntimeError, match="in flight"):
        pipe.generate_latents_interleaved(jobs, in_flight=2, on_done=on_done, **kw)
    assert seen == [0] and pipe.loras == [("a", 1.0, len(TARGETS))]
    pipe.set_lora_scale(0.5)                            # nothing in flight any more
    assert pipe.loras == [("a", 0.5, len(TARGETS))]
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    assert len(got) == 2 and all(bool(torch.isfinite(z).all()) for z in got)


def test_text_encoder_keys_change_the_embeddings_as_predicted():
    from transformers import CLIPTextConfig, CLIPTextModel
    from elasticdiffusion_official_amd import ElasticDiffusion, lora
    from elasticdiffusion_official_amd.text import ClipTextEncoder
    from tests.test_models_and_text import _Tok
    cfg = CLIPTextConfig(vocab_size=100, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                         max_position_embeddings=8)
    torch.manual_seed(0)
    clip = CLIPTextModel(cfg).eval()
    spec = copy.deepcopy(clip).double()
    enc = ClipTextEncoder([_Tok()], [copy.deepcopy(clip).to(DEV)], xl=False, device=DEV)
    pipe = ElasticDiffusion(DEV, "1.5", view_batch_size=4, unet=FakeUNet(64), vae=FakeVAE(), text_encoder=enc)
    ids = _Tok()(["hello"], "max_length", 8, True, "pt").input_ids
    e0 = pipe.get_text_embeds("hello")[0].cpu()
    with torch.no_grad():
        want0 = spec(ids)[0]
    noise = R.rel_l2(e0, want0)                        # what the fp32 forward itself is off by, no adapter involved
    inner = getattr(spec, "text_model", spec)
    paths = {"text_model.encoder.layers.0.self_attn.q_proj": inner.encoder.layers[0].self_attn.q_proj,
             "text_model.encoder.layers.1.mlp.fc1": inner.encoder.layers[1].mlp.fc1,
             "text_model.encoder.layers.1.self_attn.out_proj": inner.encoder.layers[1].self_attn.out_proj}
    entries = [("text_encoder", p, *C.random_factors(tuple(m.weight.shape), 3, 40 + i), 1.5) for i, (p, m) in enumerate(paths.items())]
    assert pipe.load_lora(C.write_kohya(entries), 0.7, name="te") == "te"
    assert pipe.loras == [("te", 0.7, 3)]
    with torch.no_grad():
        for (_, p, up, down, alpha) in entries:
            m = paths[p]
            m.weight.copy_(C.merged_fp64(m.weight, [(up, down, C.coefficient(0.7, alpha, 3))]))
        want = spec(ids)[0]
    e = pipe.get_text_embeds("hello")[0].cpu()
    err, moved = R.rel_l2(e, want), R.rel_l2(e, e0)
    print(f"text encoder: rel-L2 to the fp64 statement {err:.3e} (plain forward {noise:.3e}), moved by {moved:.3e}")
    assert err <= 4 * noise + 1e-6 and moved > 1e-2
    pipe.unload_lora()
    assert torch.equal(pipe.get_text_embeds("hello")[0].cpu(), e0)


def test_command_line_lora(tmp_path, capsys):
    from safetensors.torch import save_file
    from elasticdiffusion_official_amd import models as M
    from elasticdiffusion_official_amd.__main__ import _lora_arg, main
    assert _lora_arg("a/b.safetensors") == ("a/b.safetensors", 1.0) and _lora_arg("a/b.safetensors:0.7") == ("a/b.safetensors", 0.7)
    assert _lora_arg("a:b/c.safetensors") == ("a:b/c.safetensors", 1.0) and _lora_arg("x.safetensors:-1e-1") == ("x.safetensors", -0.1)
    cfg = M.unet_config("sd15")
    q = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    c = cfg["block_out_channels"][-1]
    path = str(tmp_path / "style.safetensors")
    save_file(C.write_kohya([("unet", q, *C.random_factors((c, c), 4, 9), 4.0)], sgm_cfg=cfg), path)
    with pytest.raises(SystemExit, match="no such file"):
        main(["--lora", str(tmp_path / "absent.safetensors")])
    save_dir = main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "1", "--resampling_steps", "1",
                     "--outdir", str(tmp_path), "--exp", "t", "--seed", "3", "--prompt", "p", "--view_batch_size", "4",
                     "--lora", f"{path}:0.7"])
    assert os.path.isfile(os.path.join(save_dir, "0.png"))
    assert "LoRA 'style' merged at scale 0.7: 1 tensors" in capsys.readouterr().out
    assert f"'{path}:0.7'" in open(os.path.join(save_dir, "args.txt")).read()
