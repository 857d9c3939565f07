"""CPU: the specification of the score PCA maps (tests/score_pca_cpu.py) against the libraries the
reference script calls, and the host-side pieces of the feature (the bilinear coefficient table, the argument rules).

The reference cap, from the restatement's own comparison with sklearn while the goldens were written (make_score_pca.py): no
byte differs by more than 1 and at most 1e-4 of the bytes differ."""
import os

import numpy as np
import pytest

from tests import resize_cpu, score_pca_cpu as S
from tests.golden import make_score_pca as M

ULP2 = 2.4e-7   # 2 ulp of fp32: the project's bar for a quantity computed in higher precision
CASES = [(name, tag) for name in M.names() for tag in ("raw", "norm")]


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_score_pca.npz"))


def test_inputs_regenerate_exactly(g17):
    """The goldens store no inputs: integer hashing and exactly rounded fp64 operations must give them again, to the bit sum."""
    for name in list(M.names()) + ["mean50"]:
        s = M.score(name)
        assert s.dtype == np.float32 and float(s.astype(np.float64).sum()) == float(g17[f"sum_{name}"]), name
    assert abs(float(M.score("mean50").mean()) - 50.0) < 0.5
    assert os.path.getsize(os.path.join(os.path.dirname(M.__file__), "g17_score_pca.npz")) < 1 << 20


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_against_live_sklearn(name, tag):
    pytest.importorskip("sklearn")
    s = M.score(name)
    ref, comps, var = M.reference_map(s, tag == "norm")
    mine = S.score_pca_map(s, tag == "norm")
    worst, share = S.byte_difference(mine["bytes"], ref)
    print(f"{name} {tag}: max {worst}, share {share:.2e}")
    assert worst <= M.CAP_MAX and share <= M.CAP_SHARE


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_against_stored_goldens(g17, name, tag):
    """What the real libraries gave when the goldens were written: within the cap always, and -- the restatement does not depend
    on the library -- exactly where it was exact then (all but two cases; the maker's printed table)."""
    mine = S.score_pca_map(M.score(name), tag == "norm")
    worst, share = S.byte_difference(mine["bytes"], g17[f"bytes_{name}_{tag}"])
    assert worst <= M.CAP_MAX and share <= M.CAP_SHARE
    if (name, tag) not in (("3x64x64_f32", "norm"), ("1x128x256_f16", "norm")):
        assert worst == 0
    # sklearn's own fit is an fp32 computation: its components are the restatement's to a few fp32 ulp, its variances likewise
    assert np.abs(mine["components"] - g17[f"components_{name}_{tag}"]).max() < 1e-5
    assert np.abs(mine["explained_variance"] / g17[f"variance_{name}_{tag}"] - 1).max() < 1e-5


def test_mean50_golden_is_the_restatement(g17):
    s = M.score("mean50")
    for tag, normalize in (("raw", False), ("norm", True)):
        assert np.array_equal(S.score_pca_map(s, normalize)["bytes"], g17[f"mean50_bytes_{tag}"])


@pytest.mark.parametrize("name", list(M.names()) + ["mean50"])
def test_components_against_an_independent_fp64_decomposition(name):
    """The restatement diagonalises the 4 x 4 covariance; the singular value decomposition of the centred data (what sklearn's
    ``full`` solver does) is another route to the same components, and numpy.linalg.eigh of numpy.cov a third."""
    s = M.score(name)
    out = S.score_pca_map(s)
    for b in range(s.shape[0]):
        X = s[b].transpose(1, 2, 0).reshape(-1, 4).astype(np.float64)
        Xc = X - X.mean(axis=0)
        _, sv, vt = np.linalg.svd(Xc, full_matrices=False)
        w, v = np.linalg.eigh(np.cov(X.T))
        for j in range(3):
            for other in (vt[j], v[:, 3 - j]):
                other = other * np.sign(other[np.argmax(np.abs(other))])
                assert np.abs(out["components"][b, j] - other).max() <= ULP2
            assert out["components"][b, j][np.argmax(np.abs(out["components"][b, j]))] > 0
        assert np.abs(out["explained_variance"][b] / (sv[:3] ** 2 / (len(X) - 1)) - 1).max() <= ULP2
        assert np.abs(out["mean"][b] - X.mean(axis=0)).max() <= ULP2 * max(1.0, np.abs(X.mean(axis=0)).max())
        assert (np.diff(out["explained_variance"][b]) < 0).all()


@pytest.mark.parametrize("name", list(M.names()) + ["mean50"])
def test_normalisation_does_not_move_the_bytes(name):
    """An affine map of the score leaves the components alone and scales the projection and its range alike: on scores whose
    spread is of the size of their values the reference's normalisation moves the picture only through its fp32 rounding.  (It is
    not a licence to skip it: a score whose channels are nearly constant at different levels is quantised by it, which is why the
    kernels form it per element.)"""
    s = M.score(name)
    a, b = S.score_pca_map(s, False), S.score_pca_map(s, True)
    worst, share = S.byte_difference(a["bytes"], b["bytes"])
    print(f"{name}: max {worst}, share {share:.2e}")
    assert worst <= 1 and share <= 1e-4
    # and the statistics move as the map says, with max - min rounded to fp32 as the reference has it
    lo, hi = float(s.min()), float(s.max())
    scale = 2.0 / float(np.float32(hi) - np.float32(lo))
    assert np.abs(b["components"] - a["components"]).max() <= ULP2
    assert np.abs(b["mean"] - ((a["mean"] - lo) * scale - 1)).max() <= ULP2
    assert np.abs(b["explained_variance"] / (a["explained_variance"] * scale ** 2) - 1).max() <= ULP2


def test_constant_projection_gives_zero_bytes():
    out = S.score_pca_map(np.full((2, 4, 5, 7), 0.25, np.float32))
    assert out["bytes"].shape == (2, 5, 7, 3) and not out["bytes"].any()
    assert not S.to_bytes(np.zeros((3, 3, 3), np.float32)).any()
    r = np.zeros((2, 2, 3), np.float32)
    r[0, 0, 0], r[1, 1, 2] = -1.0, 3.0
    assert S.to_bytes(r)[0, 0, 0] == 0 and S.to_bytes(r)[1, 1, 2] == 255 and S.to_bytes(r)[0, 1, 1] == 63   # 0.25 * 255 = 63.75


def test_specification_argument_rules():
    with pytest.raises(ValueError, match=r"\[B, 4, H, W\]"):
        S.score_pca_map(np.zeros((1, 9, 8, 8), np.float32))
    with pytest.raises(ValueError, match=r"\[B, 4, H, W\]"):
        S.score_pca_map(np.zeros((4, 8, 8), np.float32))
    with pytest.raises(ValueError, match="at least 4 pixels"):
        S.score_pca_map(np.zeros((1, 4, 1, 3), np.float32))


@pytest.mark.parametrize("hw,k", M.BILINEAR + [((33, 47), 8), ((64, 64), 3), ((3, 5), 8), ((1, 1), 8), ((16, 9), 8)])
def test_bilinear_table_gives_pillows_bytes(g17, hw, k):
    """A triangle filter of support 1 in resample.FILTERS is PIL.Image.resize(..., BILINEAR), byte for byte, at the enlargements
    the maps take (x8: the VAE factor) and at x3; against the installed Pillow and against the recorded outputs."""
    from PIL import Image
    h, w = hw
    img = M.bilinear_input(h, w)
    got = resize_cpu.resize(img, (h * k, w * k), "bilinear")
    assert np.array_equal(got, np.asarray(Image.fromarray(img).resize((w * k, h * k), Image.BILINEAR)))
    if (hw, k) in M.BILINEAR:
        assert np.array_equal(img, g17[f"bl_in_{h}x{w}"]) and np.array_equal(got, g17[f"bl_out_{h}x{w}_x{k}"])
    grey = np.ascontiguousarray(img[:, :, 0])
    assert np.array_equal(resize_cpu.resize(grey, (h * k, w * k), "bilinear"),
                          np.asarray(Image.fromarray(grey).resize((w * k, h * k), Image.BILINEAR)))


def test_bilinear_reductions_match_pillow_too():
    """The table is Pillow's for any size pair, not only enlargements (support scales with the reduction)."""
    from PIL import Image
    img = M.bilinear_input(37, 53)
    for size in ((17, 53), (37, 20), (9, 11), (40, 30)):
        assert np.array_equal(resize_cpu.resize(img, size, "bilinear"),
                              np.asarray(Image.fromarray(img).resize(size[::-1], Image.BILINEAR)))


def test_enlarged_maps_are_pillows(g17):
    out = S.score_pca_map(M.score("2x13x19_f32"), patch=8)
    assert out["enlarged"].shape == (2, 104, 152, 3)
    for b in range(2):
        assert np.array_equal(out["enlarged"][b], resize_cpu.resize(out["bytes"][b], (104, 152), "bilinear"))


def test_pipeline_argument_rules():
    from elasticdiffusion_official_amd import pipeline, resample
    from elasticdiffusion_official_amd.__main__ import build_parser
    assert pipeline.check_score_pca_arguments(False, 9) is False and pipeline.check_score_pca_arguments(True, 4) is True
    assert pipeline.check_score_pca_arguments(0, 4) is False
    for channels in (3, 8, 9, 16):
        with pytest.raises(ValueError, match="4-channel"):
            pipeline.check_score_pca_arguments(True, channels)
    assert pipeline.SCORE_PCA_KEYS == ("pca_cls_dir", "pca_uncond")
    assert set(resample.FILTERS) == {"bicubic", "lanczos", "bilinear"} and resample.FILTERS["bilinear"][1] == 1.0
    assert resample.ksize(16, 128, "bilinear") == 3
    with pytest.raises(ValueError, match="filter must be one of"):
        resample.coefficient_lists(8, 64, "nearest")
    assert build_parser().parse_args([]).score_pca is False
    assert build_parser().parse_args(["--score_pca", "true"]).score_pca is True
