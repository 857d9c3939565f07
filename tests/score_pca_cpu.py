"""numpy restatement of the reference's per-step score PCA picture (pca_diffusion_scores.py:165-179): what
``sklearn.decomposition.PCA(n_components=3).fit / transform`` + the min-max scaling + ``np.uint8`` make of one 4-channel score,
with the moments taken in fp64.  A test helper and the specification of ``ops.score_pca``: numpy only, written for clarity."""
import numpy as np


def normalise(score):
    """The script's ``(d - d.min()) / (d.max() - d.min()) * 2 - 1`` over the WHOLE tensor, every operation in fp32."""
    s = np.asarray(score, np.float32)
    lo, hi = s.min(), s.max()
    return (s - lo) / (hi - lo) * np.float32(2) - np.float32(1)


def fit(X):
    """X fp32 [n, 4] -> (components f64 [3, 4], mean f64 [4], explained_variance f64 [3]).

    Mean and covariance (divided by n - 1) from fp64 sums, the three largest eigenpairs in descending order, every component's
    sign chosen so that its entry of largest magnitude is positive (sklearn's ``svd_flip(u_based_decision=False)``)."""
    X64 = np.asarray(X, np.float64)
    n = X64.shape[0]
    mean = X64.sum(axis=0) / n
    Xc = X64 - mean
    cov = Xc.T @ Xc / (n - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1][:3]
    comps = v[:, order].T.copy()
    for j in range(3):
        if comps[j, np.argmax(np.abs(comps[j]))] < 0:
            comps[j] = -comps[j]
    return comps, mean, np.maximum(w[order], 0.0)


def to_bytes(r):
    """r fp32 [H, W, 3] -> uint8 [H, W, 3]: ``np.uint8((r - r.min()) / (r.max() - r.min()) * 255)`` in fp32, truncating.  Where the
    reference divides by zero (``r.max() == r.min()``) the bytes are 0: a stated difference."""
    r = np.asarray(r, np.float32)
    lo, hi = r.min(), r.max()
    if not hi > lo:
        return np.zeros(r.shape, np.uint8)
    return np.uint8((r - lo) / (hi - lo) * np.float32(255))


def enlarge(img, patch):
    """Pillow's bilinear enlargement of one uint8 [H, W, 3] map by ``patch`` (``T.Resize`` on a PIL image is this call)."""
    from PIL import Image
    h, w = img.shape[:2]
    return np.asarray(Image.fromarray(img).resize((w * patch, h * patch), Image.BILINEAR))


def score_pca_map(score, normalize=False, patch=None):
    """score fp32 [B, 4, H, W] -> dict: ``bytes`` uint8 [B, H, W, 3], ``components`` f64 [B, 3, 4], ``mean`` f64 [B, 4],
    ``explained_variance`` f64 [B, 3] and, with ``patch``, ``enlarged`` uint8 [B, H * patch, W * patch, 3]."""
    s = np.asarray(score, np.float32)
    if s.ndim != 4 or s.shape[1] != 4:
        raise ValueError(f"score must be [B, 4, H, W], got {s.shape}")
    B, _, H, W = s.shape
    if H * W < 4:
        raise ValueError(f"a score needs at least 4 pixels to fit three components, got {H} x {W}")
    if normalize:
        s = normalise(s)
    out = {"bytes": np.empty((B, H, W, 3), np.uint8), "components": np.empty((B, 3, 4)), "mean": np.empty((B, 4)),
           "explained_variance": np.empty((B, 3))}
    for b in range(B):
        X = s[b].transpose(1, 2, 0).reshape(-1, 4)
        comps, mean, var = fit(X)
        r = ((X.astype(np.float64) - mean) @ comps.T).astype(np.float32)
        out["bytes"][b] = to_bytes(r.reshape(H, W, 3))
        out["components"][b], out["mean"][b], out["explained_variance"][b] = comps, mean, var
    if patch:
        out["enlarged"] = np.stack([enlarge(m, patch) for m in out["bytes"]])
    return out


def byte_difference(a, b):
    """-> (largest absolute difference, share of differing bytes) of two equal-shaped uint8 arrays."""
    d = np.abs(np.asarray(a, np.int16) - np.asarray(b, np.int16))
    return int(d.max()), float(np.count_nonzero(d)) / d.size
