"""The VAE encoder on a constant-colour image (AutoencoderKL.encode_constant, geometry.plan_constant_axis), on the
CPU in fp64 with the reduced-width VAE (32, 64, 64, 64) and random non-degenerate weights:

  * the activations differ from their interior value only inside the border the recurrence predicts (constant_border_trace), and the
    plan's representative row / column and its neighbours lie inside the clean interior at every layer's input;
  * the narrowed, weighted encode equals the full one to rounding (columns, rows, both axes at once);
  * an image too small to narrow takes the full path, bit for bit;
  * every level's weights sum to the full size.
"""
import functools

import pytest
import torch

from elasticdiffusion_official_amd import geometry, models

CHANNELS = (32, 64, 64, 64)


@functools.lru_cache(maxsize=None)
def _vae():
    torch.manual_seed(11)
    vae = models.AutoencoderKL(block_out_channels=CHANNELS).double().eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    for name, p in vae.named_parameters():      # non-degenerate: no zero biases, no unit gains
        if p.dim() > 1:
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (2.0 / p[0].numel()) ** 0.5)
        else:
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3 + (1.0 if "norm" in name and name.endswith("weight") else 0.1))
    return vae


def _colours(n=2):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2 - 1


def _moments(dist):
    return torch.cat([dist.mean, dist.logvar], 1)


@functools.lru_cache(maxsize=None)
def _full(Hpx, Wpx):
    """the reference, computed once per size: ``encode`` of the expanded image"""
    col = _colours()
    with torch.no_grad():
        return _moments(_vae().encode(col[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous()).latent_dist)


def test_trace_is_the_sd_vae_recurrence():
    t = {name: (lead, trail) for name, _, lead, trail in geometry.constant_border_trace(4, 2)}
    assert t["conv_in"] == (1, 1) and t["down0.resnet1"] == (5, 5) and t["down0.downsample"] == (3, 3)
    assert t["down1.resnet1"] == (7, 7) and t["down1.downsample"] == (4, 4) and t["down2.resnet1"] == (8, 8)
    assert t["down2.downsample"] == (4, 5) and t["down3.resnet1"] == (8, 9) and t["mid.resnet1"] == (12, 13)
    assert t["conv_out"] == (13, 14)
    assert geometry.plan_constant_axis(128).keep == 32 and geometry.plan_constant_axis(63) is None


@pytest.mark.parametrize("Hpx,Wpx,axis", [(64, 512, 3), (512, 64, 2)])
def test_activations_are_constant_outside_the_analytic_border(Hpx, Wpx, axis):
    vae = _vae()
    enc = vae.encoder
    stages = [("conv_in", enc.conv_in)]
    for lv, blk in enumerate(enc.down_blocks):
        stages += [(f"down{lv}.resnet{k}", r) for k, r in enumerate(blk.resnets)]
        if blk.downsamplers is not None:
            stages.append((f"down{lv}.downsample", blk.downsamplers[0]))
    stages += [("mid.resnet0", enc.mid_block.resnets[0]), ("mid.attention", enc.mid_block.attentions[0]),
               ("mid.resnet1", enc.mid_block.resnets[1]), ("conv_out", enc.conv_out)]
    seen = {}
    hooks = [m.register_forward_hook(lambda _m, _i, out, name=name: seen.__setitem__(name, out)) for name, m in stages]
    try:
        with torch.no_grad():
            enc(_colours()[:, :, None, None].expand(-1, 3, Hpx, Wpx).contiguous())
    finally:
        for h in hooks:
            h.remove()
    trace = geometry.constant_border_trace(4, 2)
    assert [n for n, *_ in trace] == [n for n, _ in stages]
    for name, _, lead, trail in trace:
        a = seen[name].movedim(axis, -1)                    # the axis under test last
        n = a.shape[-1]
        assert lead + trail < n
        inner = a[..., lead:n - trail]
        centre = a[..., n // 2:n // 2 + 1]
        assert float((inner - centre).abs().max()) <= 1e-13 * float(a.abs().max()), name
        # and the border is really there (the recurrence is not an over-estimate by more than the structure allows at the two outermost units)
        assert float((a[..., :1] - centre).abs().max()) > 1e-9 * float(a.abs().max()), name


@pytest.mark.parametrize("L", [64, 128, 96])
def test_representative_lies_in_the_clean_interior_at_every_layer_input(L):
    """every stage reads its input at most one row / column away (3 x 3 taps; the downsampler's window starts on the representative or
    one before it), so the representative and both neighbours must be clean in every stage's INPUT, which is the previous stage's output"""
    plan = geometry.plan_constant_axis(L)
    S = 8
    for name, lv, lead, trail in geometry.constant_border_trace(4, 2):
        n = plan.keep * (S >> lv)
        r = plan.rep[lv]
        assert r == plan.rep_lat * (S >> lv) + (S >> lv) // 2
        assert lead <= r - 1 and r + 1 <= n - trail - 1, (name, lead, trail, r, n)
    # a downsampler window starts exactly on the representative (levels 0 -> 1, 1 -> 2) or one column before it (2 -> 3)
    assert plan.rep[0] == 2 * plan.rep[1] and plan.rep[1] == 2 * plan.rep[2] and plan.rep[2] == 2 * plan.rep[3] + 1
    # and the removed run is a whole number of windows at every level that is downsampled
    assert all((w[r] - 1) % 2 == 0 for w, r in zip(plan.weights[:3], plan.rep[:3]))
    assert plan.expand[:plan.rep_lat + 1] == list(range(plan.rep_lat + 1)) and plan.expand[-1] == plan.keep - 1
    assert plan.expand.count(plan.rep_lat) == L - plan.keep + 1 and len(plan.expand) == L


@pytest.mark.parametrize("Hpx,Wpx,rows,cols", [(64, 512, False, True), (512, 64, True, False), (512, 512, True, True)])
def test_narrowed_encode_equals_the_full_encode(Hpx, Wpx, rows, cols):
    vae = _vae()
    py, px = vae.constant_plan(Hpx, Wpx)
    assert (py is not None) == rows and (px is not None) == cols
    got = _moments(vae.encode_constant(_colours(), Hpx, Wpx).latent_dist)
    want = _full(Hpx, Wpx)
    assert got.shape == want.shape
    err = float((got - want).abs().max() / want.abs().max())
    print(f"encode_constant {Hpx} x {Wpx}: max abs / max abs = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("Hpx,Wpx", [(256, 256), (64, 504)])
def test_small_images_take_the_full_path_bit_for_bit(Hpx, Wpx):
    vae = _vae()
    assert vae.constant_plan(Hpx, Wpx) == (None, None)
    assert torch.equal(_moments(vae.encode_constant(_colours(), Hpx, Wpx).latent_dist), _full(Hpx, Wpx))


def test_switch_off_is_the_full_path(monkeypatch):
    monkeypatch.setattr(models, "VAE_NARROW_CONSTANT", False)
    assert torch.equal(_moments(_vae().encode_constant(_colours(), 64, 512).latent_dist), _full(64, 512))


@pytest.mark.parametrize("Wpx", [512, 1024, 520])
def test_level_weights_sum_to_the_full_size(Wpx):
    plan = geometry.plan_constant_axis(Wpx // 8)
    for lv, w in enumerate(plan.weights):
        assert sum(w) == Wpx >> lv and len(w) == (plan.keep * 8) >> lv
        assert sorted(set(w)) == [1, 1 + ((8 * (Wpx // 8 - plan.keep)) >> lv)]


def test_weights_take_no_folded_bias_and_a_16_bit_vae_runs_the_plain_blocks():
    """a folded bias or a token layout arriving while the weights are active is an error, never dropped; and a 16-bit VAE (here bf16 on
    the CPU) goes through the narrowed encode: both arms are then a few bf16 roundings (2^-8 each) from the fp64 encode"""
    x = torch.randn(1, 32, 4, 8, dtype=torch.float64)
    norm = torch.nn.GroupNorm(32, 32).double()
    models._CONSTANT_ENCODE.planes = {(4, 8): (torch.ones(8, dtype=torch.float64), None, torch.zeros(32, dtype=torch.float64))}
    try:
        ref = torch.nn.functional.group_norm(x, 32, norm.weight, norm.bias, norm.eps)
        assert float((models.group_norm_act(norm, x) - ref).abs().max()) < 1e-12
        for kw in (dict(conv_bias=torch.zeros(32, dtype=torch.float64)), dict(chan_bias=torch.zeros(1, 32, dtype=torch.float64)), dict(tokens=True)):
            with pytest.raises(RuntimeError, match="weighted statistics"):
                models.group_norm_act(norm, x, **kw)
    finally:
        models._CONSTANT_ENCODE.planes = None
    import copy
    v16 = copy.deepcopy(_vae()).bfloat16()
    got = _moments(v16.encode_constant(_colours().bfloat16(), 64, 512).latent_dist)
    full = _moments(v16.encode(_colours().bfloat16()[:, :, None, None].expand(-1, 3, 64, 512).contiguous()).latent_dist)
    want = _full(64, 512)
    e, e_full = (float((t.double() - want).norm() / want.norm()) for t in (got, full))
    print(f"bf16 VAE on the CPU: e_narrowed = {e:.3e}, e_full = {e_full:.3e}")
    assert got.dtype == torch.bfloat16 and e <= max(2.0 * e_full, 2.0 ** -6)
