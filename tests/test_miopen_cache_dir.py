"""CPU: where the package points MIOpen's user db / kernel cache.  A read-only checkout must not make every convolution
fail (MIOpen opens its SQLite kernel cache for writing): the in-tree records are then used from a per-user copy."""
import os

from elasticdiffusion_official_amd import _miopen_cache_dir


def _tree(tmp_path):
    src = tmp_path / "tree" / "miopen_cache"
    src.mkdir(parents=True)
    (src / "gfx950100.ukdb").write_bytes(b"kernels" * 100)
    (src / "gfx950100.ufdb.txt").write_text("3-256-1024-3x3-128=ConvBinWinogradRxSf2x3g1\n")
    return src


def test_writable_tree_cache_is_used_in_place(tmp_path):
    src = _tree(tmp_path)
    assert _miopen_cache_dir(str(src), writable=lambda p: True, homes=[str(tmp_path / "home")]) == str(src)
    assert not (tmp_path / "home").exists()


def test_read_only_tree_cache_is_copied_once_per_content(tmp_path):
    src = _tree(tmp_path)
    ro = lambda p: p != str(src)  # noqa: E731
    homes = [str(tmp_path / "unusable" / "x"), str(tmp_path / "home")]
    open(tmp_path / "unusable", "w").close()       # a file where the first cache home's directory would go: unusable
    dst = _miopen_cache_dir(str(src), writable=ro, homes=homes)
    assert dst.startswith(str(tmp_path / "home")) and dst != str(src)
    assert sorted(os.listdir(dst)) == sorted(os.listdir(src))
    for n in os.listdir(src):
        assert open(os.path.join(dst, n), "rb").read() == open(os.path.join(src, n), "rb").read()
    open(os.path.join(dst, "gfx950100.ukdb"), "ab").write(b"+records MIOpen added")   # the copy is MIOpen's to write
    assert _miopen_cache_dir(str(src), writable=ro, homes=homes) == dst              # same contents: same copy, kept
    assert open(os.path.join(dst, "gfx950100.ukdb"), "rb").read().endswith(b"+records MIOpen added")
    (src / "gfx950100.ufdb.txt").write_text("changed\n")
    assert _miopen_cache_dir(str(src), writable=ro, homes=homes) != dst              # new tree contents: a fresh copy


def test_no_writable_location_keeps_the_tree_path(tmp_path):
    src = _tree(tmp_path)
    assert _miopen_cache_dir(str(src), writable=lambda p: False, homes=[str(tmp_path / "home")]) == str(src)
