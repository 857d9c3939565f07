"""CPU: the Canny specification of DESIGN.md ("Canny condition extraction") as restated in tests/canny_cpu.py -- its
hand-checkable anchors, its hysteresis against an independent formulation (scipy connected components), the new C-ABI
names, and the pin against OpenCV itself for whoever has it installed."""
import numpy as np
import pytest

from tests import canny_cpu as cc


def _step(height, transpose=False):
    a = np.zeros((16, 16), np.uint8)
    a[:, 8:] = height
    return a.T.copy() if transpose else a


def test_anchor_vertical_step_gives_column_7():
    e = cc.canny(_step(255))
    want = np.zeros((16, 16), np.uint8)
    want[:, 7] = 255
    assert np.array_equal(e, want)


def test_anchor_horizontal_step_gives_row_7():
    e = cc.canny(_step(255, transpose=True))
    want = np.zeros((16, 16), np.uint8)
    want[7, :] = 255
    assert np.array_equal(e, want)


def test_anchor_weak_step_gives_nothing():
    """A step of height 40 has Sobel magnitude 4 * 40 = 160: a candidate (100 < 160 <= 200) that no strong pixel touches."""
    a = _step(40)
    assert int(cc.gradients(a)[2].max()) == 160
    cmap = cc.canny_map(a)
    assert set(np.unique(cmap)) == {0, 1} and np.array_equal(np.nonzero((cmap == 0).any(0))[0], [7])
    assert not cc.canny(a).any()


def test_thresholds_are_floored_and_swapped():
    assert cc.thresholds(100.9, 200.2) == (100, 200) and cc.thresholds(200, 100) == (100, 200)
    a = np.random.default_rng(3).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    assert np.array_equal(cc.canny(a, 200, 100), cc.canny(a, 100, 200))


def test_channel_choice_prefers_lowest_index_on_ties():
    a = _step(255)
    rgb = np.stack([a, a, a], axis=2)
    assert np.array_equal(cc.canny(rgb), cc.canny(a))
    dx, dy, m = cc.gradients(np.stack([a, 255 - a, a], axis=2))      # equal magnitudes, opposite signs: channel 0 wins
    assert int(dx[5, 7]) == 4 * 255 and int(m[5, 7]) == 4 * 255


@pytest.mark.parametrize("kind", ["noise", "blur3", "blur5"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("thr", [(100, 200), (50, 150), (20, 40)])
def test_hysteresis_matches_connected_components(kind, C, thr):
    rng = np.random.default_rng(sum(map(ord, kind)) + C)
    img = rng.integers(0, 256, (150, 211, C), dtype=np.uint8)
    if kind != "noise":
        img = cc.box_blur(img, int(kind[-1]))
    cmap = cc.canny_map(img, *thr)
    flood, passes = cc.hysteresis(cmap)
    assert passes >= 1 and np.array_equal(flood, cc.hysteresis_by_labels(cmap))
    assert np.array_equal(flood == 1, cmap == 1)                      # only candidates ever change


def test_hysteresis_pass_count_is_the_chain_length():
    """A straight chain of 20 candidates behind one strong pixel: 20 promoting waves + the empty one."""
    cmap = np.ones((5, 30), np.uint8)
    cmap[2, 3] = 2
    cmap[2, 4:24] = 0
    flood, passes = cc.hysteresis(cmap)
    assert passes == 21 and (flood[2, 3:24] == 2).all() and (flood == 2).sum() == 21


def test_new_entry_points_are_declared_and_exported():
    """Fails without the feature: the four ed_canny_* names are in the ctypes table and the built library exports them."""
    from elasticdiffusion_official_amd import _hip
    names = ["ed_canny_workspace", "ed_canny_map", "ed_canny_hysteresis", "ed_canny_edges"]
    for n in names:
        assert n in _hip.SIGNATURES, n
    assert _hip.ABI_VERSION >= 10
    _hip.build_library()
    L = _hip.lib()
    for n in names:
        assert hasattr(L, n), n
    assert any(src.endswith("canny_kernels.hip") for src in _hip.SOURCES)
    # bounds are checked before anything touches a device: C in {1, 3}, 1 <= H, W <= 8192
    assert L.ed_canny_workspace(512, 512, 3) > 0
    for bad in ((0, 5, 3), (5, 8193, 1), (5, 5, 2), (5, 5, 4)):
        assert L.ed_canny_workspace(*bad) < 0, bad
    assert L.ed_canny_map(None, 4, 4, 3, 100, 200, None, None) != 0
    assert L.ed_canny_map(1, 4, 4, 2, 100, 200, 1, None) == 1          # hipErrorInvalidValue, no launch
    assert L.ed_canny_edges(1, 0, 4, 1, None, None) == 1


def test_wrappers_refuse_cpu_tensors():
    import torch
    from elasticdiffusion_official_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.canny(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.canny_hysteresis(torch.ones(8, 8, dtype=torch.uint8))


def test_restatement_matches_opencv():
    """THE PIN for anyone who has OpenCV: the restatement (and through tests/test_canny_gpu.py the HIP kernels) against
    ``cv2.Canny`` itself.  OpenCV is not installed where this suite was written or where its GPU tests run, so there this
    test is reported as skipped; the specification was written from OpenCV 4.x's source, not checked against the library."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(0)
    for C in (1, 3):
        for shape in ((1, 1), (3, 5), (64, 96), (301, 517)):
            for blur in (0, 3, 5):
                img = rng.integers(0, 256, shape + (C,), dtype=np.uint8)
                img = cc.box_blur(img, blur) if blur else img
                img = np.ascontiguousarray(img[:, :, 0] if C == 1 else img)
                for lo, hi in ((100, 200), (50, 150), (0, 0), (200, 100), (300, 300)):
                    assert np.array_equal(cc.canny(img, lo, hi), cv2.Canny(img, lo, hi)), (C, shape, blur, lo, hi)
