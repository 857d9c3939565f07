"""elasticdiffusion_official_amd -- MI355X-native (gfx950) implementation of ONE hot path of ElasticDiffusion: the
patched global/local denoising loop behind ``ElasticDiffusion.generate_image()``.

    from elasticdiffusion_official_amd import ElasticDiffusion      # drop-in for the reference class, GPU only

HIP kernels + C ABI: csrc/elastic_kernels.hip / include/elastic_hip.h (loaded by _hip.py, wrapped by ops.py).
The package never imports ``oracle`` and has no CPU path.
"""
import os as _os

# MIOpen JIT-compiles its convolution kernels on first use (minutes for the SDXL UNet on a fresh box).  Keep its
# user find-db and compiled-kernel cache inside the repo tree so they travel with the source snapshot like the built
# .so does (git-ignored build artefacts); an empty / missing cache only costs compile time.
_MIOPEN_CACHE = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "miopen_cache")


def _writable(path):
    """MIOpen opens its kernel cache (SQLite in WAL mode) and db files for writing, and creates -wal / -shm files next to
    them; in a directory it cannot write to, every convolution fails with miopenStatusInternalError."""
    if not _os.access(path, _os.W_OK | _os.X_OK):
        return False
    return all(_os.access(_os.path.join(path, n), _os.W_OK) for n in _os.listdir(path)
               if _os.path.isfile(_os.path.join(path, n)))


def _miopen_cache_dir(src=_MIOPEN_CACHE, writable=_writable, homes=None):
    """The directory MIOpen's user db and kernel cache live in: the in-tree ``src`` when this process may write there;
    otherwise (a read-only checkout) a per-user copy of it, keyed by the tree cache's contents so the tuned records keep
    applying -- under $XDG_CACHE_HOME or ~/.cache, else the system temp directory."""
    try:
        _os.makedirs(src, exist_ok=True)
    except OSError:
        pass
    if not _os.path.isdir(src) or writable(src):
        return src
    import hashlib
    import shutil
    import tempfile
    names = sorted(n for n in _os.listdir(src) if _os.path.isfile(_os.path.join(src, n)))
    h = hashlib.sha1()
    for n in names:
        h.update(n.encode() + b"\0")
        with open(_os.path.join(src, n), "rb") as f:
            h.update(hashlib.sha1(f.read()).digest())
    tag = "miopen_" + h.hexdigest()[:16]
    if homes is None:
        homes = [_os.environ.get("XDG_CACHE_HOME") or _os.path.join(_os.path.expanduser("~"), ".cache"),
                 _os.path.join(tempfile.gettempdir(), f"elasticdiffusion_official_amd_{_os.getuid()}")]
    for home in homes:
        dst = _os.path.join(home, "elasticdiffusion_official_amd", tag)
        try:
            _os.makedirs(dst, exist_ok=True)
            for n in names:
                if not _os.path.exists(_os.path.join(dst, n)):   # copy once; concurrent importers each replace atomically
                    tmp = _os.path.join(dst, f".{n}.{_os.getpid()}.tmp")
                    shutil.copyfile(_os.path.join(src, n), tmp)
                    _os.chmod(tmp, 0o644)
                    _os.replace(tmp, _os.path.join(dst, n))
        except OSError:
            continue
        if writable(dst):
            return dst
    return src


if "MIOPEN_USER_DB_PATH" not in _os.environ or "MIOPEN_CUSTOM_CACHE_DIR" not in _os.environ:
    _MIOPEN_DIR = _miopen_cache_dir()
    _os.environ.setdefault("MIOPEN_USER_DB_PATH", _MIOPEN_DIR)
    _os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", _MIOPEN_DIR)

from .schedule import ConstScheduler, CosineScheduler, DDIMSchedule, DPMSolverSchedule, LCMSchedule, LinearScheduler  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not require a GPU (build check, CPU host-logic tests)
    if name in ("ElasticDiffusion", "ElasticDiffusionControlNet"):
        from . import pipeline
        return getattr(pipeline, name)
    raise AttributeError(name)
