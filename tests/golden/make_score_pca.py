"""Writes tests/golden/g17_score_pca.npz: what the REAL ``sklearn.decomposition.PCA`` + Pillow make of small seeded 4-channel
scores (pca_diffusion_scores.py:165-180), so that the tests of ``ops.score_pca`` have a reference that does not depend on the
scikit-learn or Pillow installed where they run; and Pillow's BILINEAR enlargement of small uint8 images.

    python tests/golden/make_score_pca.py

The inputs are not stored: ``score(name)`` regenerates them with integer hashing and exactly rounded fp64 arithmetic only (no
library generator, no libm), and ``sum_<name>`` holds the fp64 sum of each for the tests to check that they did.

Input construction (``score``): a 4-channel smooth pattern (cubic-smoothed triangle waves of the pixel coordinates) plus 0.5 x
unit-variance noise, scaled per channel by 3, 1.7, 1, 0.5, mixed by a 4 x 4 rotation (a product of six plane rotations with
Pythagorean cosines), plus an offset (0.1; 50 in the large-mean case).  Consecutive eigenvalues of the covariance then differ by a
factor >= 1.5 (asserted), so the three kept components are well defined.

Keys: ``bytes_<name>_<raw|norm>`` (sklearn + ``np.uint8``), ``components_...`` / ``variance_...`` (sklearn's, fp64), ``sum_<name>``,
``mean50_bytes_<raw|norm>`` (the restatement's: there sklearn forms its
covariance in fp32 and is the noisy party), ``bl_in_<h>x<w>`` / ``bl_out_<h>x<w>_x<k>``, ``sklearn_version``, ``pillow_version``.

While writing, the maker ASSERTS that the fp64 restatement (tests/score_pca_cpu.py) is within the reference cap of sklearn on every
stored case: no byte differs by more than 1 and at most 1e-4 of the bytes differ; and that the restatement's bytes with and without
the normalisation are within the same cap of each other.  A byte flips where a value lies within an fp32 rounding of a multiple of
1 / 255, about 3e-5 of the bytes, so in a map of fewer than 10^4 bytes a single flip already exceeds the share: an input that misses
a cap is replaced (another seed below), never the cap."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SHAPES = [(1, 3, 5), (1, 8, 8), (2, 13, 19), (1, 33, 47), (3, 64, 64), (1, 128, 256)]
SEEDS = {(1, 3, 5): 4, (1, 8, 8): 2, (2, 13, 19): 3, (1, 33, 47): 8, (3, 64, 64): 5, (1, 128, 256): 6}
MEAN50 = (1, 33, 47)
CAP_MAX, CAP_SHARE = 1, 1e-4
MIN_RATIO = 1.5
SCALES = (3.0, 1.7, 1.0, 0.5)
BILINEAR = [((8, 12), 8), ((5, 7), 8), ((13, 19), 8), ((13, 19), 3)]
_PYTHAGOREAN = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (12, 35, 37))


def _hash01(seed, n):
    """n doubles in [0, 1) from splitmix64 of (seed, index): integer arithmetic, the same on every machine."""
    x = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed * 0xD1B54A32D192ED03 % 2 ** 64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _wave(x):
    """a smooth wave of period 1 in [-1, 1] from exactly rounded operations: a triangle wave through s (1.5 - 0.5 s^2)"""
    s = 2.0 * np.abs(2.0 * (x - np.floor(x)) - 1.0) - 1.0
    return s * (1.5 - 0.5 * s * s)


def _rotation(seed):
    u = _hash01(seed ^ 0x5151, 12)
    Q = np.eye(4)
    for k, (p, q) in enumerate(((0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2))):
        a, b, c = _PYTHAGOREAN[int(u[2 * k] * len(_PYTHAGOREAN))]
        co, si = a / c, (b / c if u[2 * k + 1] < 0.5 else -b / c)
        G = np.eye(4)
        G[p, p], G[q, q], G[p, q], G[q, p] = co, co, -si, si
        Q = G @ Q
    return Q


def make_score(seed, B, H, W, offset=0.1):
    """-> fp32 [B, 4, H, W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    u, v = yy / float(max(H - 1, 1)), xx / float(max(W - 1, 1))
    out = np.empty((B, 4, H, W), np.float64)
    for b in range(B):
        sd = seed * 1000 + b
        par = _hash01(sd, 12).reshape(4, 3)
        noise = (_hash01(sd + 500, 4 * H * W).reshape(4, H, W) - 0.5) * 12.0 ** 0.5
        base = np.stack([_wave((0.5 + 2.5 * par[c, 0]) * u + (0.5 + 2.5 * par[c, 1]) * v + par[c, 2]) for c in range(4)])
        base = (base + 0.5 * noise) * np.asarray(SCALES).reshape(4, 1, 1)
        out[b] = np.einsum("ij,jhw->ihw", _rotation(sd), base) + offset
    return out.astype(np.float32)


def names():
    """-> {name: (shape, fp16-rounded?)} of the cases with sklearn bytes"""
    return {f"{B}x{H}x{W}_{kind}": ((B, H, W), kind == "f16") for B, H, W in SHAPES for kind in ("f32", "f16")}


def score(name):
    """The input of case ``name`` (a key of ``names()``, or "mean50"), fp32 [B, 4, H, W]."""
    if name == "mean50":
        return make_score(50, *MEAN50, offset=50.0)
    shape, half = names()[name]
    s = make_score(SEEDS[shape], *shape)
    return s.astype(np.float16).astype(np.float32) if half else s


def reference_map(s, normalize):
    """pca_diffusion_scores.py:165-179 with the real libraries, every sample: -> (bytes, components, explained variance)"""
    from sklearn.decomposition import PCA
    s = np.asarray(s, np.float32)
    if normalize:
        s = (s - s.min()) / (s.max() - s.min()) * 2 - 1
    B, _, H, W = s.shape
    out, comps, var = np.empty((B, H, W, 3), np.uint8), np.empty((B, 3, 4)), np.empty((B, 3))
    for b in range(B):
        X = np.ascontiguousarray(s[b].transpose(1, 2, 0).reshape(-1, 4))
        pca = PCA(n_components=3)
        pca.fit(X)
        img = pca.transform(X).reshape(H, W, 3)
        img = (img - img.min()) / (img.max() - img.min())
        out[b], comps[b], var[b] = np.uint8(img * 255), pca.components_, pca.explained_variance_
    return out, comps, var


def bilinear_input(h, w):
    return (_hash01(h * 100 + w, h * w * 3) * 256.0).astype(np.uint8).reshape(h, w, 3)


def main():
    import PIL
    import sklearn
    from PIL import Image

    from tests.score_pca_cpu import byte_difference, score_pca_map
    data = {"sklearn_version": np.array(sklearn.__version__), "pillow_version": np.array(PIL.__version__)}
    for name in names():
        s = score(name)
        data[f"sum_{name}"] = np.array(s.astype(np.float64).sum())
        for b in range(s.shape[0]):
            w = np.sort(np.linalg.eigvalsh(np.cov(s[b].reshape(4, -1).astype(np.float64))))[::-1]
            assert (w[:3] / w[1:] >= MIN_RATIO).all(), f"{name}[{b}]: eigenvalue ratios {w[:3] / w[1:]}: pick another seed"
        for tag, normalize in (("raw", False), ("norm", True)):
            ref, comps, var = reference_map(s, normalize)
            mine = score_pca_map(s, normalize)
            worst, share = byte_difference(mine["bytes"], ref)
            print(f"{name:>16s} {tag:>4s}: restatement vs sklearn max {worst}, share {share:.2e}")
            assert worst <= CAP_MAX and share <= CAP_SHARE, f"{name} {tag}: replace this input (another seed), not the cap"
            data[f"bytes_{name}_{tag}"], data[f"components_{name}_{tag}"], data[f"variance_{name}_{tag}"] = ref, comps, var
        # on these inputs the normalisation moves the picture through its fp32 rounding only: the same cap
        worst, share = byte_difference(score_pca_map(s, False)["bytes"], score_pca_map(s, True)["bytes"])
        assert worst <= CAP_MAX and share <= CAP_SHARE, f"{name}: normalised vs not: max {worst}, share {share:.2e}: another seed"
    s = score("mean50")
    data["sum_mean50"] = np.array(s.astype(np.float64).sum())
    for tag, normalize in (("raw", False), ("norm", True)):
        data[f"mean50_bytes_{tag}"] = score_pca_map(s, normalize)["bytes"]
        worst, share = byte_difference(data[f"mean50_bytes_{tag}"], reference_map(s, normalize)[0])
        print(f"          mean50 {tag:>4s}: restatement vs sklearn max {worst}, share {share:.2e} (not a bar: sklearn is the noisy party)")
    for (h, w), k in BILINEAR:
        img = bilinear_input(h, w)
        data[f"bl_in_{h}x{w}"] = img
        data[f"bl_out_{h}x{w}_x{k}"] = np.asarray(Image.fromarray(img).resize((w * k, h * k), Image.BILINEAR))
    path = os.path.join(HERE, "g17_score_pca.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(data)} arrays, {os.path.getsize(path)} bytes, sklearn {sklearn.__version__}, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
