"""CPU: Multi-ControlNet and guidance windows -- the keep table by hand and at its edges, the argument rules,
the ABI contract of ``ed_control_residuals`` and the torch fallback of ``ops.control_residuals`` on tensors that are not on a device."""
import re

import pytest
import torch

from elasticdiffusion_official_amd import _hip, ops
from elasticdiffusion_official_amd.pipeline import check_control_arguments, control_keep
from tests import multi_controlnet_cpu as mc
from tests.test_abi import header_functions


def _columns(table):
    return [list(col) for col in zip(*table)]


def test_keep_table_by_hand():
    """T = 4, windows (0, 0.5) and (0.25, 1.0)"""
    for fn in (control_keep, mc.control_keep):
        net0, net1 = _columns(fn(4, [0.0, 0.25], [0.5, 1.0]))
        assert net0 == [1.0, 1.0, 0.0, 0.0]
        assert net1 == [0.0, 1.0, 1.0, 1.0]


def test_keep_table_edges():
    for fn in (control_keep, mc.control_keep):
        for T in (1, 3, 50):
            assert fn(T, [0.0, 0.0], [1.0, 1.0]) == [[1.0, 1.0]] * T           # the defaults keep every step
        assert fn(1, [0.0], [1.0]) == [[1.0]]
        assert fn(1, [0.0], [0.5]) == [[0.0]]                                   # (i + 1) / T = 1 > 0.5
        assert _columns(fn(4, [0.3], [0.45]))[0] == [0.0] * 4                   # narrower than one step: closed everywhere
        assert _columns(fn(5, [0.2], [0.4]))[0] == [0.0, 1.0, 0.0, 0.0, 0.0]    # exactly one step wide
    assert control_keep(7, [0.1, 0.5, 0.0], [0.9, 1.0, 0.3]) == mc.control_keep(7, [0.1, 0.5, 0.0], [0.9, 1.0, 0.3])


def test_single_net_defaults_stay_on_the_legacy_path():
    assert check_control_arguments(1, False, 0.2) is None
    assert check_control_arguments(1, False, 0.2, 0.0, 1.0) is None
    assert check_control_arguments(0, False, 1.0) is None                      # no ControlNet at all
    assert check_control_arguments(1, True, 0.2) == ([0.2], [0.0], [1.0])      # a list of one net is the multi path
    assert check_control_arguments(1, False, [0.2]) == ([0.2], [0.0], [1.0])   # ... so is a list-valued scale
    assert check_control_arguments(1, False, 0.2, 0.0, 0.5) == ([0.2], [0.0], [0.5])  # ... and a window
    assert check_control_arguments(2, True, 0.5, [0.0, 0.25], 1.0) == ([0.5, 0.5], [0.0, 0.25], [1.0, 1.0])


@pytest.mark.parametrize("args", [
    dict(n_nets=2, nets_listed=True, scale=[0.2]),                                          # list lengths
    dict(n_nets=2, nets_listed=True, scale=0.2, start=[0.0, 0.1, 0.2]),
    dict(n_nets=2, nets_listed=True, scale=0.2, end=[1.0]),
    dict(n_nets=1, nets_listed=False, scale=[0.2, 0.3]),
    dict(n_nets=1, nets_listed=False, scale=0.2, start=0.5, end=0.5),                       # start >= end
    dict(n_nets=2, nets_listed=True, scale=0.2, start=[0.0, 0.6], end=[1.0, 0.4]),
    dict(n_nets=1, nets_listed=False, scale=0.2, start=-0.1),                               # out of [0, 1]
    dict(n_nets=1, nets_listed=False, scale=0.2, end=1.5),
    dict(n_nets=1, nets_listed=False, scale=0.2, start=float("nan")),
    dict(n_nets=1, nets_listed=False, scale=0.2, condition_image=[object(), object()]),     # a list of conditions with one net
    dict(n_nets=1, nets_listed=False, scale=0.2, condition_image=[object()]),
    dict(n_nets=2, nets_listed=True, scale=0.2, condition_image=[object()]),
    dict(n_nets=ops.CONTROL_MAX_NETS + 1, nets_listed=True, scale=0.2),                     # more than ED_CONTROL_MAX_NETS nets
    dict(n_nets=0, nets_listed=False, scale=[0.2]),                                         # no net to apply it to
])
def test_argument_rules(args):
    with pytest.raises(ValueError):
        check_control_arguments(**args)


def test_wrapper_refuses_too_many_nets_and_bad_weights():
    r = [[torch.zeros(2, 3)] for _ in range(ops.CONTROL_MAX_NETS + 1)]
    with pytest.raises(ValueError):
        ops.control_residuals(None, r, torch.ones(2, len(r)))
    with pytest.raises(ValueError):
        ops.control_residuals(None, r[:2], torch.ones(2, 3))
    with pytest.raises(ValueError):
        ops.control_residuals(None, r[:2], torch.ones(2, 2, dtype=torch.float64))
    x = torch.zeros(2, 3)
    with pytest.raises(ValueError):                                                         # the output aliases a residual
        ops.control_residuals([torch.zeros(2, 3)], [[x]], torch.ones(2, 1), outs=[x])
    with pytest.raises(ValueError):                                                         # f16 skip with f32 residuals
        ops.control_residuals([torch.zeros(2, 3, dtype=torch.float16)], [[x]], torch.ones(2, 1))


def test_entry_point_is_declared_with_matching_arity():
    declared = dict(header_functions())
    name = "ed_control_residuals"
    assert name in declared and name in _hip.SIGNATURES
    args = [a.strip() for a in declared[name].split(",") if a.strip()]
    assert len(args) == len(_hip.SIGNATURES[name])
    assert [a.split()[-1].lstrip("*") for a in args] == ["table_host", "n_levels", "n_nets", "w", "n_tiles", "stream"]
    header = open(_hip.INCLUDE + "/elastic_hip.h").read()
    consts = {n: int(re.search(r"%s\s*=\s*(\d+)" % n, header).group(1))
              for n in ("ED_CONTROL_MAX_NETS", "ED_CONTROL_LEVEL_WORDS", "ED_CONTROL_TILE", "ED_CONTROL_MAX_LEVELS")}
    assert consts == {"ED_CONTROL_MAX_NETS": ops.CONTROL_MAX_NETS, "ED_CONTROL_LEVEL_WORDS": ops.CONTROL_LEVEL_WORDS,
                      "ED_CONTROL_TILE": ops.CONTROL_TILE, "ED_CONTROL_MAX_LEVELS": ops.CONTROL_MAX_LEVELS}
    assert consts["ED_CONTROL_MAX_NETS"] == 4 and consts["ED_CONTROL_LEVEL_WORDS"] == 8 + consts["ED_CONTROL_MAX_NETS"]


def test_abi_version_is_still_13_and_the_library_exports_it():
    assert _hip.ABI_VERSION == 13
    _hip.build_library()
    L = _hip.lib()
    assert L.ed_version() == 13
    assert hasattr(L, "ed_control_residuals")


def test_control_table_layout():
    skip, r0, r1 = torch.zeros(3, 5000), torch.zeros(3, 5000), torch.zeros(3, 5000)
    out2, q0, q1 = torch.zeros(3, 7, dtype=torch.float16), torch.zeros(3, 7, dtype=torch.float16), torch.zeros(3, 7, dtype=torch.float16)
    host, n_tiles = ops.control_table([(skip, skip, [r0, r1]), (None, out2, [q0, q1])], 2)
    assert host.dtype == torch.int64 and host.numel() == 2 * ops.CONTROL_LEVEL_WORDS
    a, b = host[:12].tolist(), host[12:].tolist()
    assert a == [skip.data_ptr(), skip.data_ptr(), 5000, 3, ops.ED_F32, ops.ED_F32, 0, 0, r0.data_ptr(), r1.data_ptr(), 0, 0]
    assert b == [0, out2.data_ptr(), 7, 3, ops.ED_F16, ops.ED_F16, 6, 0, q0.data_ptr(), q1.data_ptr(), 0, 0]
    assert n_tiles == 3 * 2 + 3 * 1


@pytest.mark.parametrize("dt,rdt", [(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
                                    (torch.float32, torch.float16), (torch.float32, torch.bfloat16)])
def test_cpu_fallback_agrees_with_the_restatement(dt, rdt):
    g = torch.Generator().manual_seed(3)
    B, N = 3, 3
    shapes = [(B, 5, 3, 4), (B, 7), (B, 2, 9, 1)]
    skips = [torch.randn(s, generator=g).to(dt) for s in shapes]
    res = [[torch.randn(s, generator=g).to(rdt) for s in shapes] for _ in range(N)]
    w = torch.tensor([[0.2, 0.5, 1.5], [0.0, 0.3, 0.0], [0.0, 0.0, 0.0]])
    res[0][1][1] = float("nan")                                                             # unread: w[1, 0] == 0
    res[2][0][2] = float("inf")
    want = [mc.control_residuals_cpu(skips[l], [res[n][l] for n in range(N)], w) for l in range(len(shapes))]
    keep = [s.clone() for s in skips]
    got = ops.control_residuals([s.clone() for s in skips], res, w)
    for l in range(len(shapes)):
        assert got[l].dtype == dt and torch.isfinite(got[l].float()).all()
        assert torch.equal(got[l], want[l])
        assert torch.equal(got[l][2], keep[l][2])                                           # all-zero weights: the skip
    if dt == rdt:                                                                           # without skips: the sum, +0 where closed
        got = ops.control_residuals(None, res, w)
        for l in range(len(shapes)):
            want_l = mc.control_residuals_cpu(None, [res[n][l] for n in range(N)], w)
            assert got[l].dtype == rdt and torch.equal(got[l], want_l)
            assert not got[l][2].any() and not torch.signbit(got[l][2].float()).any()
