"""CPU tier of the exact nearest-neighbour index and the image-search application: the host-only refusal of clip_amd_index_create,
the reference's query classification, and the database checks of `search` that run before any device work."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    # no visible device at all, even on a GPU machine: the context is host-only
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def test_index_create_on_host_only_context_returns_null(clip_lib, fixture_cache):
    from oracle import fixtures
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    code = ("import clip_cpp_amd as c\n"
            "m = c.Clip(%r, verbosity=0)\n"
            "assert c.lib().clip_amd_ctx_device(m.ctx) == -1\n"
            "L = c.lib()\n"
            "print('create', bool(L.clip_amd_index_create(m.ctx, 32, 1)))\n"
            "print('load', bool(L.clip_amd_index_load(m.ctx, b'/nonexistent/images.index')))\n"
            "try:\n"
            "    c.Index(m, 32)\n"
            "except RuntimeError as e:\n"
            "    print('raised', e)\n") % model
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "create False" in r.stdout and "load False" in r.stdout and "raised clip_amd_index_create failed" in r.stdout
    assert "clip_amd_index_create: host-only context" in r.stderr


def test_index_entry_points_reject_null_arguments(clip_lib):
    L = clip_lib.lib()
    assert not L.clip_amd_index_create(None, 512, 1)
    assert not L.clip_amd_index_add(None, None, 1)
    assert not L.clip_amd_index_add_device(None, None, 1)
    assert not L.clip_amd_index_search(None, None, 1, 5, None, None)
    assert not L.clip_amd_index_search_device(None, None, 1, 5, None, None)
    assert not L.clip_amd_index_save(None, b"x")
    assert not L.clip_amd_index_load(None, b"x")
    assert L.clip_amd_index_size(None) == 0 and L.clip_amd_index_dim(None) == 0
    L.clip_amd_index_free(None)


@pytest.mark.parametrize("args, want", [
    (["a", "photo", "of", "a", "cat"], ("", "a photo of a cat")),
    (["cat.jpg"], ("cat.jpg", "")),
    (["dir/x.JPEG"], ("dir/x.JPEG", "")),
    (["a.png"], ("a.png", "")),
    (["b.GIF"], ("b.GIF", "")),
    (["photo.webp"], ("", "photo.webp")),
    (["photo.Jpg"], ("", "photo.Jpg")),      # the reference knows two spellings per extension, not every case
    (["cat.jpg", "and", "dog"], ("", "cat.jpg and dog")),
    (["find", "cat.jpg"], ("", "find cat.jpg")),   # an image extension only counts when the query is that one argument
    (["noext"], ("", "noext")),
])
def test_query_classification_matches_reference(args, want):
    from clip_cpp_amd import image_search
    assert image_search.classify_query(args) == want


def test_image_extension_rule():
    from clip_cpp_amd import image_search as s
    for ok in ("a.jpg", "a.JPG", "a.jpeg", "a.JPEG", "a.gif", "a.GIF", "a.png", "a.PNG", "x.y/a.png"):
        assert s.is_image_file_extension(ok)
    for bad in ("a.bmp", "a.Png", "a", "a.png.txt", "jpg", ".tiff"):
        assert not s.is_image_file_extension(bad)


def _search(db, *args):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search", "search", "--db", str(db)] + list(args)
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def test_search_without_database_fails(tmp_path):
    r = _search(tmp_path, "a", "cat")
    assert r.returncode != 0
    assert "main: Unable to load model from" in r.stdout
    assert "images.paths" in r.stderr


def test_search_with_mismatched_database_fails(tmp_path):
    import struct
    (tmp_path / "images.paths").write_text("model.gguf\nimg/a.jpg\nimg/b.jpg\n")
    with open(tmp_path / "images.index", "wb") as f:        # a valid header that holds 3 rows against 2 paths
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 4, 0, 3) + b"\0" * 48)
    r = _search(tmp_path, "a", "cat")
    assert r.returncode != 0
    assert "main: index files size missmatch" in r.stdout


def test_search_with_missing_index_file_fails(tmp_path):
    (tmp_path / "images.paths").write_text("model.gguf\nimg/a.jpg\n")
    r = _search(tmp_path, "cat.png")
    assert r.returncode != 0
    assert "images.index" in r.stderr


def test_cli_usage_errors(tmp_path):
    r = subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"], capture_output=True, text=True, env=_host_only_env(), cwd=ROOT,
                       timeout=120)
    assert r.returncode != 0 and "Usage" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search", "build", "--db", str(tmp_path)], capture_output=True, text=True,
                       env=_host_only_env(), cwd=ROOT, timeout=120)
    assert r.returncode != 0 and "dir/with/pictures" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search", "search", "-h"], capture_output=True, text=True,
                       env=_host_only_env(), cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "-n N, --results N: Number of results to display. Default: 5" in r.stdout
