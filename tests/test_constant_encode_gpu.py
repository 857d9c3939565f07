"""-m gpu: the kernels behind the narrowed constant-image VAE encode through the C ABI, and the encode itself.

Weighted GroupNorm (ed_groupnorm_nhwc_f32_weighted, plain and split output; ed_groupnorm_f32_weighted) and the biased row softmax
(ed_softmax_rows_bias) against the PLAIN fp64 op on the tensor expanded by repeating the weighted row / column, taken back to the
narrowed positions; the bar is test_vae_split.py's, e <= max(2 e_ref32, 3e-7) with e_ref32 torch's fp32 op on the same expanded
tensor.  Null weights / a null bias must give the unweighted entry point's bits.  Then AutoencoderKL.encode_constant on the split
path against ``encode`` of the full image and against the fp64 CPU encode, and pipeline._strip_frames with the switch on and off."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _axis_index(n, at, weight):
    """(expand, first): the index list that repeats position ``at`` ``weight`` times, and where each original position first lands"""
    expand = list(range(at + 1)) + [at] * (weight - 1) + list(range(at + 1, n))
    first = [i if i <= at else i + weight - 1 for i in range(n)]
    return torch.tensor(expand, device=DEV), torch.tensor(first, device=DEV)


def _weight_vector(n, at, weight):
    w = torch.ones(n, device=DEV)
    w[at] = weight
    return w


GN_CASES = {"wx": ((23, 89), None), "wy": (None, (2, 17)), "both": ((23, 89), (2, 17))}


def _gn_reference(x, gamma, beta, groups, silu, colw, roww):
    """(fp64, fp32) plain GroupNorm of ``x`` [N, C, H, W] expanded by the weighted column / row, at the narrowed positions; and (wx, wy)"""
    N, C, H, W = x.shape
    big, wx, wy = x, None, None
    pick_x = pick_y = None
    if colw is not None:
        ex, pick_x = _axis_index(W, *colw)
        big, wx = big.index_select(3, ex), _weight_vector(W, *colw)
    if roww is not None:
        ey, pick_y = _axis_index(H, *roww)
        big, wy = big.index_select(2, ey), _weight_vector(H, *roww)
    big = big.contiguous()

    def back(y):
        y = y if pick_x is None else y.index_select(3, pick_x)
        return y if pick_y is None else y.index_select(2, pick_y)

    want = F.group_norm(big.double(), groups, gamma.double(), beta.double(), 1e-6)
    ref32 = F.group_norm(big, groups, gamma, beta, 1e-6)
    if silu:
        want, ref32 = F.silu(want), F.silu(ref32)
    return back(want), back(ref32), wx, wy


def _gn_inputs(C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(2, C, 6, 40, generator=g) * 2.5 + 0.7).to(DEV)
    return x, (torch.randn(C, generator=g) * 0.5 + 1).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)


@pytest.mark.parametrize("case", sorted(GN_CASES))
def test_weighted_groupnorm_nhwc_f32_plain_and_split(case):
    from elasticdiffusion_official_amd import ops
    C, G = 128, 32
    x, gamma, beta = _gn_inputs(C, 128)
    x = x.contiguous(memory_format=torch.channels_last)
    want, ref32, wx, wy = _gn_reference(x, gamma, beta, G, True, *GN_CASES[case])
    y = ops.groupnorm_nhwc_f32(x, gamma, beta, G, 1e-6, silu=True, wx=wx, wy=wy)
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last) and y.shape == x.shape
    e, e32 = _rel(y, want), _rel(ref32, want)
    print(f"weighted groupnorm_nhwc_f32 {case}: e = {e:.3e}, e_ref32 = {e32:.3e}")
    assert e <= max(2.0 * e32, 3e-7), (e, e32)
    assert _rel(ops.groupnorm_nhwc_f32(x, gamma, beta, G, 1e-6, silu=True), want) > 1e-3     # the weights matter
    s = ops.groupnorm_nhwc_f32(x, gamma, beta, G, 1e-6, silu=True, split=True, wx=wx, wy=wy)
    assert s.dtype == torch.float16 and tuple(s.shape) == (2, 3 * C, 6, 40) and s.is_contiguous(memory_format=torch.channels_last)
    hi, lo, hi2 = s[:, :C], s[:, C:2 * C], s[:, 2 * C:]
    assert torch.equal(hi, hi2) and torch.equal(hi, y.half())
    err = (hi.double() + lo.double() - y.double()).abs()
    assert bool((err <= y.double().abs() * 2.0 ** -21 + 2.0 ** -24).all())


def test_all_ones_weights_are_the_unweighted_groupnorm_bit_for_bit():
    from elasticdiffusion_official_amd import ops
    x, gamma, beta = _gn_inputs(128, 128)
    xl = x.contiguous(memory_format=torch.channels_last)
    ones_x, ones_y = torch.ones(40, device=DEV), torch.ones(6, device=DEV)
    for split in (False, True):
        plain = ops.groupnorm_nhwc_f32(xl, gamma, beta, 32, 1e-6, silu=True, split=split)
        for wx, wy in ((ones_x, ones_y), (ones_x, None), (None, ones_y)):
            assert torch.equal(plain, ops.groupnorm_nhwc_f32(xl, gamma, beta, 32, 1e-6, silu=True, split=split, wx=wx, wy=wy))
    x, gamma, beta = _gn_inputs(64, 64)
    plain = ops.groupnorm_f32(x, gamma, beta, 32, 1e-6, silu=True)
    for wx, wy in ((ones_x, ones_y), (ones_x, None), (None, ones_y)):
        assert torch.equal(plain, ops.groupnorm_f32(x, gamma, beta, 32, 1e-6, silu=True, wx=wx, wy=wy))


@pytest.mark.parametrize("case", sorted(GN_CASES))
def test_weighted_groupnorm_f32_nchw(case):
    from elasticdiffusion_official_amd import ops
    C, G = 64, 32
    x, gamma, beta = _gn_inputs(C, 64)
    for silu in (True, False):
        want, ref32, wx, wy = _gn_reference(x, gamma, beta, G, silu, *GN_CASES[case])
        y = ops.groupnorm_f32(x, gamma, beta, G, 1e-6, silu=silu, wx=wx, wy=wy)
        assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == x.shape
        e, e32 = _rel(y, want), _rel(ref32, want)
        print(f"weighted groupnorm_f32 {case} silu={silu}: e = {e:.3e}, e_ref32 = {e32:.3e}")
        assert e <= max(2.0 * e32, 3e-7), (e, e32)
    assert _rel(ops.groupnorm_f32(x, gamma, beta, G, 1e-6), want) > 1e-3


def test_softmax_rows_with_a_log_multiplicity_bias():
    """softmax(scale * s + log m) over the narrowed keys = the plain softmax over the keys repeated m times, summed over the copies"""
    from elasticdiffusion_official_amd import ops
    g = torch.Generator(device="cpu").manual_seed(9)
    s = (torch.randn(3, 70, 240, generator=g) * 4).to(DEV)
    mult = torch.ones(240, dtype=torch.int64)
    mult[57], mult[200] = 97, 5
    scale = 64 ** -0.5
    owner = torch.repeat_interleave(torch.arange(240), mult).to(DEV)               # expanded key -> narrowed key
    big = s.index_select(2, owner)

    def back(p):                                                                    # the copies' probabilities, summed in fp64
        return torch.zeros(3, 70, 240, dtype=torch.float64, device=DEV).index_add_(2, owner, p.double())

    want = back(torch.softmax(big.double() * scale, -1))
    ref32 = back(torch.softmax(big * scale, -1))
    bias = mult.to(DEV).float().log()
    got = ops.softmax_rows_(s.clone(), scale, bias)
    e, e32 = _rel(got, want), _rel(ref32, want)
    print(f"softmax_rows_ with bias: e = {e:.3e}, e_ref32 = {e32:.3e}")
    assert e <= max(2.0 * e32, 3e-7), (e, e32)
    assert torch.equal(ops.softmax_rows_(s.clone(), scale), ops.softmax_rows_(s.clone(), scale, torch.zeros(240, device=DEV)))
    assert _rel(ops.softmax_rows_(s.clone(), scale), want) > 1e-2                   # the bias matters


# ---- the encode ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vae64():
    """(fp32 VAE (64, 128, 128, 128) on the device, the same weights in fp64 on the CPU, 3 colours).  The weights are those of the CPU
    test (tests/test_constant_encode.py): random and non-degenerate -- He-scaled matrices, biases 0.1 +- 0.3, GroupNorm gains 1 +- 0.3 --
    so that every affine parameter takes part (PyTorch's default init has unit gains and zero GroupNorm biases)."""
    from elasticdiffusion_official_amd import models as M
    torch.manual_seed(4)
    cpu = M.AutoencoderKL(block_out_channels=(64, 128, 128, 128)).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    for name, p in cpu.named_parameters():
        if p.dim() > 1:
            p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5)
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.3 + (1.0 if "norm" in name and name.endswith("weight") else 0.1))
    colours = torch.rand(3, 3, generator=torch.Generator().manual_seed(8)) * 2 - 1
    return copy.deepcopy(cpu).to(DEV), cpu.double(), colours


@functools.lru_cache(maxsize=None)
def _fp64_moments(Hpx, Wpx):
    _, cpu, colours = _vae64()
    with torch.no_grad():
        d = cpu.encode(colours.double()[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous()).latent_dist
    return torch.cat([d.mean, d.logvar], 1)


@pytest.mark.parametrize("Hpx,Wpx", [(64, 512), (512, 64)])
def test_narrowed_encode_on_the_split_path(Hpx, Wpx):
    """rel(narrowed, full) < 5e-5 is test_vae_split.py's bar between two fp32 paths; e_narrowed <= max(2 e_full, 1e-6) against fp64.
    Measured on the MI355X with these weights: 64 x 512: rel 3.1e-5, e_narrowed 1.2e-5, e_full 3.0e-5; 512 x 64: rel 1.3e-5,
    e_narrowed 5.0e-6, e_full 1.3e-5.  On a CONSTANT image the distance between the arms is the FULL path's own error: its GroupNorm
    statistics are shifted by the group's first element, a corner pixel that zero padding makes an outlier, so the variance of the
    constant interior is a small difference of large fp32 sums (the same encoder is 1e-6 from fp64 on a random image, and the library
    convolutions give the same figures as the split ones); the narrowed arm keeps the interior's multiplicity in double and is 2.5 to 5
    times closer to fp64.  With PyTorch's default init (models._seeded_init) instead of these weights the full path is 3.3e-5 / 7.3e-5
    from fp64, the narrowed one 8e-6 / 1.4e-5, and the 512 x 64 arms are 7.7e-5 apart: above this bar, for that reason."""
    from elasticdiffusion_official_amd import models as M, ops
    vae, _, colours = _vae64()
    assert M.VAE_NARROW_CONSTANT and M.VAE_SPLIT_CONV
    col = colours.to(DEV)

    def run(fn):
        ops.TIMER.start()
        try:
            with torch.no_grad():
                d = fn().latent_dist
        finally:
            seen = ops.TIMER.stop()
        return torch.cat([d.mean, d.logvar], 1), seen, sum(w[0] for w in ops.TIMER.work.values())

    full, seen_full, flops_full = run(lambda: vae.encode(col[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous()))
    got, seen, flops = run(lambda: vae.encode_constant(col, Hpx, Wpx))
    assert got.shape == full.shape == (3, 8, Hpx // 8, Wpx // 8)
    want = _fp64_moments(Hpx, Wpx)
    r, e, e_full = _rel(got, full), _rel(got, want), _rel(full, want)
    print(f"encode_constant {Hpx} x {Wpx}: rel(narrowed, full) = {r:.3e}, e_narrowed = {e:.3e}, e_full = {e_full:.3e}, "
          f"declared GFLOP {flops / 1e9:.2f} vs {flops_full / 1e9:.2f}")
    assert r < 5e-5
    assert e <= max(2.0 * e_full, 1e-6), (e, e_full)
    assert {"ed_conv3x3_nhwc_f32out", "ed_groupnorm_nhwc_f32_weighted", "ed_groupnorm_f32_weighted", "ed_softmax_rows_bias"} <= set(seen), seen
    assert "ed_groupnorm_nhwc_f32" not in seen and "ed_softmax_rows" not in seen
    assert "ed_groupnorm_nhwc_f32_weighted" not in seen_full and "ed_conv3x3_nhwc_f32out" in seen_full
    assert 0 < flops < 0.6 * flops_full


def _moments(dist):
    return torch.cat([dist.mean, dist.logvar], 1)


def _both_arms(vae, col, Hpx, Wpx):
    with torch.no_grad():
        full = _moments(vae.encode(col[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous()).latent_dist)
        got = _moments(vae.encode_constant(col, Hpx, Wpx).latent_dist)
    return got, full


@pytest.mark.parametrize("Hpx,Wpx", [(64, 512), (512, 64)])
def test_narrowed_encode_with_the_split_path_off(Hpx, Wpx, monkeypatch):
    """The fp32 VAE on the library convolutions (VAE_SPLIT_CONV off): NCHW throughout, every GroupNorm through
    ed_groupnorm_f32_weighted, the ResnetBlocks as plain blocks (no folded biases).  Same bars as on the split path.  Measured on the
    MI355X: 64 x 512: rel 3.0e-5, e_narrowed 1.1e-5, e_full 3.0e-5; 512 x 64: rel 1.3e-5, e_narrowed 5.0e-6, e_full 1.3e-5."""
    from elasticdiffusion_official_amd import models as M, ops
    monkeypatch.setattr(M, "VAE_SPLIT_CONV", False)
    vae, _, colours = _vae64()
    ops.TIMER.start()
    try:
        got, full = _both_arms(vae, colours.to(DEV), Hpx, Wpx)
    finally:
        seen = ops.TIMER.stop()
    want = _fp64_moments(Hpx, Wpx)
    r, e, e_full = _rel(got, full), _rel(got, want), _rel(full, want)
    print(f"encode_constant, split path off, {Hpx} x {Wpx}: rel(narrowed, full) = {r:.3e}, e_narrowed = {e:.3e}, e_full = {e_full:.3e}")
    assert r < 5e-5
    assert e <= max(2.0 * e_full, 1e-6), (e, e_full)
    assert {"ed_groupnorm_f32_weighted", "ed_softmax_rows_bias"} <= set(seen) and "ed_conv3x3_nhwc_f32out" not in seen, seen


@pytest.mark.parametrize("Hpx,Wpx", [(64, 512), (512, 64)])
def test_narrowed_encode_of_a_16_bit_vae(Hpx, Wpx):
    """An fp16 VAE: ``encode`` runs the fused 16-bit blocks (conv1's bias folded into norm2), the narrowed encode the plain blocks
    with the weighted statistics and the attention's log multiplicity in fp32.  Both arms against the fp64 CPU encode of the
    unrounded weights: e_narrowed <= max(2 e_full, 2^-9).  The floor is four fp16 roundings (2^-11 each): below it twice the full
    arm's error says nothing about a path of some thirty 16-bit layers.  Measured on the MI355X: e_narrowed 2.28e-3 / 2.28e-3, e_full
    2.25e-3 / 2.18e-3, the arms 2.2e-3 / 2.0e-3 apart."""
    import copy as _copy
    vae, _, colours = _vae64()
    vae16 = _copy.deepcopy(vae).half()
    got, full = _both_arms(vae16, colours.to(DEV).half(), Hpx, Wpx)
    assert got.dtype == torch.float16 and got.shape == full.shape == (3, 8, Hpx // 8, Wpx // 8)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(full).all())
    want = _fp64_moments(Hpx, Wpx)
    e, e_full = _rel(got, want), _rel(full, want)
    print(f"encode_constant, fp16 VAE, {Hpx} x {Wpx}: e_narrowed = {e:.3e}, e_full = {e_full:.3e}, rel(narrowed, full) = {_rel(got, full):.3e}")
    assert e <= max(2.0 * e_full, 2.0 ** -9), (e, e_full)


@pytest.mark.parametrize("Hpx,Wpx", [(64, 512), (512, 64)])
def test_default_init_narrowed_arm_is_the_one_closer_to_fp64(Hpx, Wpx):
    """PyTorch's default init (models._seeded_init), where the two fp32 arms are up to 7.7e-5 apart (the docstring of
    test_narrowed_encode_on_the_split_path): the distance is the FULL arm's error on a constant image, so the narrowed arm must be
    at least as close to the fp64 CPU encode as the full one.  Measured: 8.1e-6 against 3.3e-5, 1.4e-5 against 7.3e-5."""
    from elasticdiffusion_official_amd import models as M
    cpu = M.AutoencoderKL(block_out_channels=(64, 128, 128, 128))
    M._seeded_init(cpu, 3)
    cpu = cpu.eval().requires_grad_(False)
    colours = _vae64()[2]
    got, full = _both_arms(copy.deepcopy(cpu).to(DEV), colours.to(DEV), Hpx, Wpx)
    with torch.no_grad():
        want = _moments(cpu.double().encode(colours.double()[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous()).latent_dist)
    e, e_full = _rel(got, want), _rel(full, want)
    print(f"encode_constant, default init, {Hpx} x {Wpx}: e_narrowed = {e:.3e}, e_full = {e_full:.3e}, rel(narrowed, full) = {_rel(got, full):.3e}")
    assert e <= e_full, (e, e_full)


def test_strip_frames_with_the_switch_on_and_off():
    """The flagship's pad geometry scaled down (two 8 x 64-latent strips, 3 timesteps) through the reduced-width pipeline: same frames
    to fp32 re-association, same host RNG state afterwards, and the narrowed path batches both units into ONE VAE call."""
    from elasticdiffusion_official_amd import ElasticDiffusion, geometry, models as M
    from tests import ddim_variants as V
    from tests.fakes import FakeUNet
    _, vae = M.build_models("1.5", device="cpu", dtype=torch.float32, small=True, seed=0)
    pipe = ElasticDiffusion(DEV, "1.5", unet=FakeUNet(64), vae=copy.deepcopy(vae), text_encoder=V.embed_fn(False))
    pad = geometry.PadPlan(48, 64, 64)
    assert [s[2:4] for s in pad.strips] == [(8, 64), (8, 64)]
    ts = list(pipe.scheduler.set_timesteps(3))
    calls = []
    orig = pipe.vae.encode_constant
    pipe.vae.encode_constant = lambda colour, H, W: (calls.append(tuple(colour.shape)), orig(colour, H, W))[1]
    out, state = {}, {}
    saved = M.VAE_NARROW_CONSTANT
    try:
        for on in (False, True):
            M.VAE_NARROW_CONSTANT = on
            pipe.seed_everything(7)
            out[on] = pipe._strip_frames(pad, ts, 4).clone()
            state[on] = torch.get_rng_state()
    finally:
        M.VAE_NARROW_CONSTANT = saved
    assert calls == [(6, 3)]
    assert torch.equal(state[True], state[False])
    assert bool(torch.isfinite(out[True]).all()) and float(out[False].abs().max()) > 0
    r = _rel(out[True], out[False])
    print(f"_strip_frames narrowed vs full: rel-L2 = {r:.3e}")
    assert r < 5e-5
