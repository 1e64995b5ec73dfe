"""CPU tier of the query-set searches and of `image_search match`: the new entry points exist and fail on a NULL index without a device;
Index.search_sets refuses a malformed set_lims before the library is reached; `match` is in the usage texts, refuses a plain database
before any model is loaded and, on a gridded one, gets as far as the model."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def test_new_entry_points_on_a_null_index(clip_lib, capfd):
    L = clip_lib.lib()
    for name in ("clip_amd_index_search_sets", "clip_amd_index_search_sets_device", "clip_amd_index_search_ids_sets",
                 "clip_amd_test_index_sets_block", "clip_amd_bench_search_sets"):
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
    q = np.zeros(8, dtype=np.float32)
    ids = np.zeros(2, dtype=np.int64)
    lims = np.array([0, 2], dtype=np.int64)
    dist = np.full(4, -3.0, dtype=np.float32)
    out = np.full(4, -3, dtype=np.int64)
    qrows = np.full(4, -3, dtype=np.int32)
    fp, ip, qp = dist.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int64)), qrows.ctypes.data_as(C.POINTER(C.c_int32))
    lp = lims.ctypes.data_as(C.POINTER(C.c_int64))
    capfd.readouterr()
    assert L.clip_amd_index_search_sets(None, q.ctypes.data_as(C.POINTER(C.c_float)), 2, lp, 1, 4, None, None, fp, ip, qp) is False
    assert L.clip_amd_index_search_sets_device(None, None, 2, lp, 1, 4, None, None, None, None, None) is False
    assert L.clip_amd_index_search_ids_sets(None, ids.ctypes.data_as(C.POINTER(C.c_int64)), 2, lp, 1, 4, 0, None, None, fp, ip, qp) is False
    assert capfd.readouterr().err.count("index is NULL") == 3
    assert L.clip_amd_test_index_sets_block(None, 128) == -1
    assert np.all(dist == -3.0) and np.all(out == -3) and np.all(qrows == -3)


def test_bench_hook_without_a_device():
    code = "import clip_cpp_amd as c; print('MICROS', c.bench_search_sets('f16', 1024, 64, 4, 5, 5, 5, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("MICROS")[1]) == -1.0


def test_set_lims_are_checked_before_the_library(clip_lib):
    ix = object.__new__(clip_lib.Index)                  # no handle: a call that reached the library would raise "the index is closed"
    ix.dim = 4
    ix.handle = None
    q = np.zeros((6, 4), dtype=np.float32)
    for bad in ([1, 6], [0, 4, 3, 6], [0, 5], [0, 7], [], [[0, 6]], [0.0, 6.0], 6):
        with pytest.raises(ValueError):
            ix.search_sets(q, bad, 5)
        with pytest.raises(ValueError):
            ix.search_ids_sets(np.arange(6), bad, 5, exclude_own=False)
        with pytest.raises(ValueError):
            ix.search_sets_device(0, 6, bad, 5, None, None, 0, 0, 0)
    with pytest.raises(RuntimeError, match="closed"):
        ix.search_sets(q, [0, 0, 6, 6], 5)               # a well-formed set_lims goes on to the library
    lims = clip_lib.Index._set_lims(np.array([0, 2, 2, 6], dtype=np.int32), 6)
    assert lims.dtype == np.int64 and lims.tolist() == [0, 2, 2, 6]


def _search(*args):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def _gridded_database(d):
    """a database whose model does not exist, with a hand-written images.regions: a run that got as far as loading the model says so"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "images.paths"), "w") as f:
        f.write("no/such/model.gguf\nimg/a.png\n")
    with open(os.path.join(d, "images.index"), "wb") as f:
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 8, 1, 5))
    with open(os.path.join(d, "images.regions"), "w") as f:
        f.write("grid 2\n0 0 0 10 10\n0 0 0 5 5\n0 5 0 5 5\n0 0 5 5 5\n0 5 5 5 5\n")


def test_match_usage(capsys):
    from clip_cpp_amd import image_search
    assert image_search.main([]) == 1
    out = capsys.readouterr().out
    assert "match [options] [IMAGE]" in out and "{build|search|dedup}" in out
    assert "match  [-m MODEL]" in image_search.__doc__ and "Index.knn_graph_grouped" in image_search.__doc__
    with pytest.raises(SystemExit):
        image_search.main(["match", "-h"])
    out = capsys.readouterr().out
    assert "Usage: python -m clip_cpp_amd.image_search match" in out and "-n N, --results N" in out
    assert image_search._parse(["--db", "x"], False, match=True)["rest"] == []
    p = image_search._parse(["--db", "x", "a.png", "-n", "3"], False, match=True)
    assert p["rest"] == ["a.png"] and p["results"] == 3 and p["db"] == "x"
    assert image_search._parse(["a.png", "b.png"], False, match=True) is None
    for flag in (["--like", "a.png"], ["-d", "0.2"], ["--in", "x"], ["--grid", "2"]):
        assert image_search._parse(flag, False, match=True) is None, flag
    r = _search("match", "a.png", "b.png")
    assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search match" in r.stdout


def test_match_routing_without_a_model(tmp_path):
    g, plain = tmp_path / "g", tmp_path / "plain"
    _gridded_database(g)
    _gridded_database(plain)
    os.remove(plain / "images.regions")
    # a plain database: refused by name, with the commands that serve it, before any model is loaded
    for extra in ([], ["img/a.png"], ["some/file.png"]):
        r = _search("match", "--db", plain, *extra)
        assert r.returncode == 1, (extra, r.stdout[-1000:], r.stderr[-1000:])
        assert str(plain) in r.stderr and "was not built with --grid" in r.stderr and "search --like" in r.stderr and "neighbors" in r.stderr
        assert "Unable to load model" not in r.stdout
    # a gridded one: every form gets as far as the model, which does not exist
    for extra in ([], ["img/a.png"], ["some/file.png"]):
        r = _search("match", "--db", g, *extra)
        assert r.returncode == 1 and "Unable to load model from no/such/model.gguf" in r.stdout, (extra, r.stdout[-1000:], r.stderr[-1000:])
        assert "--grid" not in r.stderr
    # a regions file that is not one is refused by name
    (g / "images.regions").write_text("no header\n")
    r = _search("match", "--db", g)
    assert r.returncode == 1 and "images.regions" in r.stderr and "Unable to load model" not in r.stdout
    assert (plain / "images.paths").read_text() == "no/such/model.gguf\nimg/a.png\n"
