"""-m gpu: the score PCA maps through the HIP path (csrc/pca_kernels.hip, ``ops.score_pca``).

Bars:
  * bytes against the recorded ``sklearn.decomposition.PCA`` + ``np.uint8`` outputs (tests/golden/g17_score_pca.npz): every byte
    within 1, at most 1e-3 of the bytes differ -- ten times the cap the fp64 restatement itself meets against sklearn (the
    margin was meant for an fp32 contraction order in the projection; the kernels project in fp64 and need none of it).  The mean-50 case meets the same bar against the restatement (there sklearn's fp32 covariance is the
    noisy party); un-shifted fp32 or naive sums would fail it;
  * the fit: components and mean within 2.4e-7 (2 ulp of fp32) absolute of the fp64 restatement -- for the mean, whose fp32
    rounding alone is |mean| * 6e-8, of max(1, |mean|) --, explained variance within 2.4e-7 relative;
  * two launches give the same bits; a batch is its samples; the enlargement is Pillow's BILINEAR byte for byte;
  * in the pipeline the keyword only reads: latents bit-equal, host RNG in the same state, and without it no launch is added.
"""
import os

import numpy as np
import pytest
import torch

from tests import score_pca_cpu as S
from tests.fakes import FakeUNet, FakeVAE, synthetic_text_embeds
from tests.golden import cases
from tests.golden import make_score_pca as M
from tests.test_guidance_rescale_gpu import EPS, _loop_kw, _pipe
from tests.test_hip_parity import DEV

pytestmark = pytest.mark.gpu

ULP2 = 2.4e-7
BAR_MAX, BAR_SHARE = 1, 1e-3
CASES = [(name, tag) for name in list(M.names()) + ["mean50"] for tag in ("raw", "norm")]


def _ops():
    from elasticdiffusion_official_amd import ops
    return ops


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_score_pca.npz"))


_SPEC = {}


def _spec(name, normalize):
    """The fp64 restatement of one golden input, computed once and shared."""
    if (name, normalize) not in _SPEC:
        _SPEC[name, normalize] = S.score_pca_map(M.score(name), normalize)
    return _SPEC[name, normalize]


def _check_bytes(got, want, what):
    worst, share = S.byte_difference(got, want)
    print(f"{what}: max byte difference {worst}, share of differing bytes {share:.2e} (bar {BAR_MAX}, {BAR_SHARE:.0e})")
    assert worst <= BAR_MAX and share <= BAR_SHARE, (what, worst, share)


def _check_fit(fit, spec, what):
    comps, mean, var = (t.cpu().double().numpy() for t in fit)
    e_c = np.abs(comps - spec["components"]).max()
    e_m = (np.abs(mean - spec["mean"]) / np.maximum(1.0, np.abs(spec["mean"]))).max()
    e_v = np.abs(var / spec["explained_variance"] - 1).max()
    print(f"{what}: components {e_c:.2e}, mean {e_m:.2e}, explained variance {e_v:.2e} (bar {ULP2:.1e})")
    assert e_c <= ULP2 and e_m <= ULP2 and e_v <= ULP2, (what, e_c, e_m, e_v)


# ---------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES)
def test_bytes_fit_and_determinism(g17, name, tag):
    """(1,3,5): fewer pixels than one wave; (1,8,8): less than one block; (2,13,19): tails and per-sample indexing; (1,33,47);
    (3,64,64); (1,128,256): 64 blocks per sample, the merge.  fp32 and fp16-rounded values, with and without ``normalize``."""
    ops = _ops()
    normalize = tag == "norm"
    host = M.score(name)
    assert float(host.astype(np.float64).sum()) == float(g17[f"sum_{name}"]), "the seeded input did not regenerate"
    s = torch.from_numpy(host).to(DEV)
    out, fit = ops.score_pca(s, normalize=normalize, return_fit=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (s.shape[0], s.shape[2], s.shape[3], 3)
    spec = _spec(name, normalize)
    want = g17[f"mean50_bytes_{tag}"] if name == "mean50" else g17[f"bytes_{name}_{tag}"]
    _check_bytes(out.cpu().numpy(), want, f"{name} {tag} vs {'restatement' if name == 'mean50' else 'sklearn'}")
    _check_bytes(out.cpu().numpy(), spec["bytes"], f"{name} {tag} vs restatement")
    _check_fit(fit, spec, f"{name} {tag}")
    ws = ops.score_pca_workspace(s.shape[0], s.shape[2] * s.shape[3], DEV)
    out2, fit2 = ops.score_pca(s, normalize=normalize, workspace=ws, return_fit=True)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(fit, fit2))
    # an affine map of the score moves the bytes only through its fp32 rounding; the statistics move with it
    out3, fit3 = ops.score_pca(s, normalize=not normalize, workspace=ws, return_fit=True)
    _check_bytes(out3.cpu().numpy(), out.cpu().numpy(), f"{name}: normalised vs not")
    assert not torch.equal(fit[2], fit3[2])


@pytest.mark.parametrize("name", ["2x13x19_f32", "3x64x64_f16"])
def test_a_batch_is_its_samples(name):
    ops = _ops()
    s = torch.from_numpy(M.score(name)).to(DEV)
    out, fit = ops.score_pca(s, return_fit=True)
    for b in range(s.shape[0]):
        one, fit1 = ops.score_pca(s[b:b + 1].contiguous(), return_fit=True)
        assert torch.equal(one[0], out[b])
        assert all(torch.equal(a[0], f[b]) for a, f in zip(fit1, fit))


@pytest.mark.parametrize("name", ["2x13x19_f32", "1x8x8_f32", "1x33x47_f16"])
def test_misaligned_view(name):
    """A score that starts one element into its buffer (4-byte, not 16-byte, aligned) gives the bits of the aligned copy."""
    ops = _ops()
    s = torch.from_numpy(M.score(name)).to(DEV)
    buf = torch.empty(s.numel() + 1, device=DEV)
    buf[1:].copy_(s.flatten())
    view = buf[1:].view(s.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    a, fa = ops.score_pca(s, normalize=True, return_fit=True)
    b, fb = ops.score_pca(view, normalize=True, return_fit=True)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(fa, fb))


def test_constant_score_gives_zero_bytes():
    ops = _ops()
    s = torch.full((2, 4, 9, 11), 0.25, device=DEV)
    for normalize in (False, True):
        out, fit = ops.score_pca(s, normalize=normalize, return_fit=True)
        assert not bool(out.any())
        assert torch.equal(fit[1], torch.full((2, 4), 0.25, device=DEV)) and not bool(fit[2].any())


def test_rejections_launch_nothing_and_leave_the_state_clean():
    import ctypes
    from elasticdiffusion_official_amd import _hip
    ops = _ops()
    L = _hip.lib()
    good = torch.from_numpy(M.score("1x8x8_f32")).to(DEV)
    want = ops.score_pca(good, normalize=True)
    torch.cuda.synchronize()
    # the wrapper
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_pca(good.cpu())
    with pytest.raises(RuntimeError, match=r"\[B, 4, H, W\]"):
        ops.score_pca(torch.zeros(1, 9, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match=r"\[B, 4, H, W\]"):
        ops.score_pca(torch.zeros(4, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match="4 <= H"):
        ops.score_pca(torch.zeros(1, 4, 1, 3, device=DEV))
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        ops.score_pca(good.half())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.score_pca(good.permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match="workspace must hold"):
        ops.score_pca(good, workspace=torch.empty(4, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="score_pca_workspace"):
        ops.score_pca_workspace(1, 3, DEV)
    assert L.ed_score_pca_workspace(1, 3) == 0 and L.ed_score_pca_workspace(0, 64) == 0 and L.ed_score_pca_workspace(1, 2 ** 28 + 1) == 0
    # the C ABI: every rule of the header, checked before anything is launched (the outputs keep their fill)
    ws = ops.score_pca_workspace(1, 64, DEV)
    comps, mean, var, norm = (torch.full((1, k), 7.0, device=DEV) for k in (12, 4, 3, 2))
    out = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    INVALID = 1   # hipErrorInvalidValue

    def fit(score=good, B=1, C=4, H=8, W=8, c=comps, m=mean, v=var, n=norm, w=ws):
        return L.ed_score_pca_fit(p(score) if score is not None else None, B, C, H, W, 1, p(c) if c is not None else None, p(m),
                                  p(v), p(n), p(w) if w is not None else None, stream)

    def pmap(score=good, B=1, C=4, H=8, W=8, n=norm, o=out, w=ws):
        return L.ed_score_pca_map(p(score), B, C, H, W, p(n) if n is not None else None, p(o) if o is not None else None, p(w),
                                  stream)

    big = torch.empty(1, dtype=torch.float32, device=DEV)   # never dereferenced: the extents are refused first
    for bad in (dict(C=3), dict(C=9), dict(H=1, W=3), dict(H=0), dict(B=0), dict(B=-1), dict(score=big, H=1 << 15, W=1 << 14),
                dict(score=None), dict(c=None), dict(w=None), dict(c=good), dict(m=comps), dict(w=good), dict(n=var)):
        assert fit(**bad) == INVALID, bad
    misaligned = torch.empty(17, dtype=torch.float64, device=DEV).view(torch.uint8)[4:]
    assert fit(w=misaligned) == INVALID
    for bad in (dict(C=5), dict(H=1, W=3), dict(B=0), dict(o=None), dict(o=good), dict(w=good), dict(n=good), dict(n=ws)):
        assert pmap(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (comps, mean, var, norm)) and bool((out == 9).all())
    # and the next valid call succeeds, with the same bits as before
    assert torch.equal(ops.score_pca(good, normalize=True), want)
    assert fit() == 0 and pmap() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("hw,k", M.BILINEAR)
def test_bilinear_resize_is_pillows_bytes(g17, hw, k):
    ops = _ops()
    h, w = hw
    img = torch.from_numpy(g17[f"bl_in_{h}x{w}"]).to(DEV)
    got = ops.resize_u8(img, (h * k, w * k), filter="bilinear")
    assert np.array_equal(got.cpu().numpy(), g17[f"bl_out_{h}x{w}_x{k}"])
    with pytest.raises(ValueError, match="filter must be one of"):
        ops.resize_u8(img, (h * k, w * k), filter="nearest")


# ---------------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------------
class _Recorder:
    """Wrapped round ``ops.score_pca``: keeps every call's input (a copy, on the host), keyword and output."""

    def __init__(self, monkeypatch):
        ops = _ops()
        self.calls, real = [], ops.score_pca

        def wrapped(score, normalize=False, **kw):
            out = real(score, normalize=normalize, **kw)
            self.calls.append((score.detach().cpu().numpy().copy(), bool(normalize), out))
            return out

        monkeypatch.setattr(ops, "score_pca", wrapped)


def _check_maps_against_calls(maps, calls, indices, shape):
    """maps = {"pca_cls_dir": {i: bytes}, "pca_uncond": {i: bytes}}; calls in loop order: (direction, True), (local, False) per index"""
    assert set(maps) == {"pca_cls_dir", "pca_uncond"}
    assert len(calls) == 2 * len(indices)
    for n, i in enumerate(indices):
        for key, (score, normalize, out) in (("pca_cls_dir", calls[2 * n]), ("pca_uncond", calls[2 * n + 1])):
            assert normalize == (key == "pca_cls_dir") and score.shape == shape
            assert sorted(maps[key]) == list(indices) and maps[key][i] is out
            assert out.dtype == torch.uint8 and tuple(out.shape) == (shape[0], shape[2], shape[3], 3) and out.is_cuda
            _check_bytes(out.cpu().numpy(), S.score_pca_map(score, normalize)["bytes"], f"{key}[{i}]")
    assert not np.array_equal(calls[0][0], calls[1][0])     # direction and local score are different signals ...
    assert not np.array_equal(calls[0][0], calls[2][0])     # ... and move from step to step


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["cfg2_sd_512x1024", "overlap_536x776"])
def test_generate_image_maps_and_nothing_else_moves(monkeypatch, name, fused):
    """cfg2: padded global rows, RePaint and RRG active; overlap: overlapping views on an odd latent (67 x 97)."""
    from PIL import Image
    from elasticdiffusion_official_amd import ops, pipeline
    c = cases.E2E_CASES[name]
    kw = dict(_loop_kw(name), progress=lambda it: it)
    indices = [i for i in range(c["steps"]) if i % 2 == 0]
    monkeypatch.setattr(pipeline, "FUSED_GLUE", fused)
    lat, tails, counts = {}, {}, {}
    kept = []
    real_epilogue = ops.phase_epilogue
    monkeypatch.setattr(ops, "phase_epilogue", lambda *a, **k: (kept.append(k.get("direction") is not None), real_epilogue(*a, **k))[1])
    for label, extra in (("off", {}), ("false", dict(score_pca=False))):
        pipe = _pipe(name, EPS, log_freq=2)
        pipe.seed_everything(c["seed"])
        ops.TIMER.start()
        try:
            imgs, log = pipe.generate_image("p", "", **kw, **extra)
        finally:
            counts[label] = {k: v[0] for k, v in ops.TIMER.stop().items()}
        lat[label], tails[label] = pipe.last_latents.clone(), torch.rand(4)
        assert log == {} and pipe.last_score_pca is None
    assert not any(kept) and not any("pca" in k or "resize" in k for k in counts["off"]) and counts["off"] == counts["false"]
    rec = _Recorder(monkeypatch)
    pipe = _pipe(name, EPS, log_freq=2)
    pipe.seed_everything(c["seed"])
    ops.TIMER.start()
    try:
        imgs, log = pipe.generate_image("p", "", **kw, score_pca=True)
    finally:
        counts["on"] = {k: v[0] for k, v in ops.TIMER.stop().items()}
    tails["on"] = torch.rand(4)
    assert torch.equal(pipe.last_latents, lat["off"]) and torch.equal(lat["false"], lat["off"])
    assert torch.equal(tails["on"], tails["off"]) and torch.equal(tails["false"], tails["off"])
    # the only launches the keyword adds: two fits and two maps per logged index, and the enlargements after the loop
    added = {k: v for k, v in counts["on"].items() if counts["off"].get(k) != v}
    assert added == {"ed_score_pca_fit": 2 * len(indices), "ed_score_pca_map": 2 * len(indices),
                     "ed_resize_rows_u8": 2 * len(indices), "ed_resize_cols_u8": 2 * len(indices)}, added
    Hl, Wl = c["H"] // 8, c["W"] // 8
    maps = pipe.last_score_pca
    _check_maps_against_calls(maps, rec.calls, indices, (1, 4, Hl, Wl))
    assert set(log) == {"pca_cls_dir", "pca_uncond"}
    for key in log:
        assert sorted(log[key]) == indices
        for i, picture in log[key].items():
            assert isinstance(picture, Image.Image) and picture.mode == "RGB" and picture.size == (c["W"], c["H"])
            small = Image.fromarray(maps[key][i][0].cpu().numpy())
            assert np.array_equal(np.asarray(picture), np.asarray(small.resize((Wl * 8, Hl * 8), Image.BILINEAR)))


def test_first_phase_inputs_with_verbose_and_controlnet_signature():
    """The keyword composes with ``verbose`` (both keep the by-products) and exists on the ControlNet pipeline."""
    import inspect
    from elasticdiffusion_official_amd import ElasticDiffusion, ElasticDiffusionControlNet
    for cls in (ElasticDiffusion, ElasticDiffusionControlNet):
        assert inspect.signature(cls.generate_image).parameters["score_pca"].default is False
        assert inspect.signature(cls.generate_latents).parameters["score_pca"].default is False
    name = "cfg2_sd_512x1024"
    lat = {}
    for verbose in (False, True):
        pipe = _pipe(name, EPS, verbose=verbose, log_freq=3)
        pipe.seed_everything(3)
        _, log = pipe.generate_image("p", "", **_loop_kw(name), progress=lambda it: it, score_pca=True)
        lat[verbose] = (pipe.last_latents.clone(), {k: {i: m.clone() for i, m in v.items()} for k, v in pipe.last_score_pca.items()})
        assert {"pca_cls_dir", "pca_uncond"} <= set(log) and sorted(log["pca_uncond"]) == [0, 3]
    assert torch.equal(lat[False][0], lat[True][0])
    for key in lat[False][1]:
        assert all(torch.equal(lat[False][1][key][i], lat[True][1][key][i]) for i in (0, 3))
    assert "intermediate_x0_imgs" in log


def test_generate_on_a_bare_latent(monkeypatch):
    """``generate()`` is the script's own loop (PCA:151-204): maps of cond - uncond and of uncond, on a latent that needs padding."""
    from elasticdiffusion_official_amd import ElasticDiffusion
    c = cases.G11_CASES["gen_sd_pad_32x64"]
    (un, pun), (co, pco) = synthetic_text_embeds(1)
    text, pooled = torch.cat([un, co]), torch.cat([pun, pco])
    rec = _Recorder(monkeypatch)
    seen, infos, tails = {}, {}, {}
    for flag in (False, True):
        pipe = ElasticDiffusion(DEV, c["sd"], log_freq=2, unet=FakeUNet(c["sample"]), vae=FakeVAE())
        pipe.default_size = (4 * 8 * c["h"], 4 * 8 * c["w"])
        pipe.scheduler.set_timesteps(c["steps"])
        pipe.seed_everything(c["seed"])
        z = torch.randn(2, 4, c["h"], c["w"])
        dec = pipe.decode_latents
        pipe.decode_latents = lambda lat_, dec=dec, flag=flag: (seen.__setitem__(flag, lat_.clone()), dec(lat_))[1]
        _, infos[flag] = pipe.generate(z, text.repeat_interleave(2, 0), pooled.repeat_interleave(2, 0), guidance_scale=c["guidance"],
                                       score_pca=flag)
        tails[flag] = torch.rand(4)
        if not flag:
            assert set(infos[False]) == {"inter_x0"} and not rec.calls
    assert torch.equal(seen[False], seen[True]) and torch.equal(tails[False], tails[True])
    indices = [i for i in range(c["steps"]) if i % 2 == 0]
    _check_maps_against_calls({k: infos[True][k] for k in ("pca_cls_dir", "pca_uncond")}, rec.calls, indices, (2, 4, c["h"], c["w"]))
    with pytest.raises(ValueError, match="4-channel"):
        pipe.generate(torch.zeros(1, 3, 8, 8), text, pooled, score_pca=True)


def test_interleaved_jobs_with_and_without_the_key(monkeypatch):
    """A job's maps are those of running it alone.  The rows of several jobs share one model batch, and a model's rounding depends on
    the batch shape, so the inputs of a map agree to rounding, not to the bit.  For the local score that is a perturbation far below
    a byte step (the byte bar holds against the alone run's map).  FakeUNet's class direction is a per-channel CONSTANT plus the
    rounding noise of cond - uncond: its map is a picture of that noise, comparable between two runs only where the inputs are
    bit-equal -- so every map is also checked against the restatement of the input it was made from."""
    name = "cfg2_sd_512x1024"
    kw = _loop_kw(name)

    def embed(prompts):  # stateless (the programs' calls interleave)
        (un, pun), (co, pco) = synthetic_text_embeds(1)
        p = prompts[0] if isinstance(prompts, (list, tuple)) else prompts
        return (un, pun) if p == "" else (co, pco)

    rec = _Recorder(monkeypatch)

    def input_of(out):
        return next(score for score, _, o in rec.calls if o is out)

    pipe = _pipe(name, EPS, text_encoder=embed, log_freq=2)
    seeds = [cases.E2E_CASES[name]["seed"], 11, 12]
    alone = []
    for s in seeds:
        pipe.seed_everything(s)
        z = pipe.generate_latents("p", "", **kw, score_pca=True).clone()
        alone.append((z, pipe.last_score_pca))
    jobs = [dict(prompts="p", negative_prompts="", seed=s, score_pca=flag) for s, flag in zip(seeds, (True, False, True))]
    got = pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    assert sorted(pipe.job_score_pca) == [0, 2]
    for j in (0, 2):
        maps = pipe.job_score_pca[j]
        assert set(maps) == {"pca_cls_dir", "pca_uncond"}
        for key in maps:
            assert sorted(maps[key]) == [0, 2]
            for i in maps[key]:
                mine, theirs = maps[key][i], alone[j][1][key][i]
                a, b = input_of(mine), input_of(theirs)
                assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(b)   # the project's bar for interleaved against alone
                _check_bytes(mine.cpu().numpy(), S.score_pca_map(a, key == "pca_cls_dir")["bytes"], f"job {j} {key}[{i}] vs restatement")
                if np.array_equal(a, b):
                    assert torch.equal(mine, theirs)
                elif key == "pca_uncond":
                    _check_bytes(mine.cpu().numpy(), theirs.cpu().numpy(), f"job {j} {key}[{i}] vs alone")
    for z, (want, _) in zip(got, alone):
        assert float((z - want).norm() / want.norm()) < 1e-5
    assert not torch.equal(pipe.job_score_pca[0]["pca_uncond"][2], pipe.job_score_pca[2]["pca_uncond"][2])
    pipe.unet.config.in_channels = 8   # a model whose scores are not 4-channel: refused before anything runs
    with pytest.raises(ValueError, match="4-channel"):
        pipe.generate_latents_interleaved(jobs, in_flight=2, **kw)
    with pytest.raises(ValueError, match="4-channel"):
        pipe.generate_latents("p", "", **kw, score_pca=True)


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------
def test_cli_writes_the_scripts_file_names(tmp_path):
    from PIL import Image
    from elasticdiffusion_official_amd.__main__ import main
    d = main(["--sd_version", "1.5", "--H", "512", "--W", "512", "--steps", "3", "--resampling_steps", "1", "--outdir",
              str(tmp_path), "--seed", "3", "--prompt", "a test prompt", "--view_batch_size", "4", "--exp", "pca",
              "--score_pca", "true", "--log_freq", "2"])
    names = sorted(f for f in os.listdir(d) if f.startswith("pca_"))
    assert names == ["pca_cls_dir_0.png", "pca_cls_dir_2.png", "pca_uncond_0.png", "pca_uncond_2.png"]
    for f in names:
        a = np.asarray(Image.open(os.path.join(d, f)))
        assert a.shape == (512, 512, 3) and a.min() < 64 and a.max() > 192   # the maps span 0..255 before the enlargement
    assert "score_pca: True" in open(os.path.join(d, "args.txt")).read()
