"""CPU tier of k-NN voting (clip_amd_index_vote*, Index.vote*, `image_search file` / `audit`): the numpy definition the GPU tests compare
against, on hand-made rankings; the new entry points exist and fail on a NULL index without a device; Index.vote* refuse bad k, m and
labels before the library is reached; `file` and `audit` are in the usage texts, refuse a gridded database before any model is loaded and
name an unknown path of a --labels file."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from vote_common import same_votes, vote_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
SYMBOLS = ("clip_amd_index_vote", "clip_amd_index_vote_device", "clip_amd_index_vote_ids", "clip_amd_index_vote_graph",
           "clip_amd_index_vote_graph_device", "clip_amd_test_index_vote_block", "clip_amd_bench_vote_graph")


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def test_definition_on_hand_made_rankings():
    labels = np.array([7, 7, 3, 3, 9, -1, 2 ** 31 - 1], dtype=np.int64)
    dist = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, np.inf]], dtype=np.float32)
    ids = np.array([[2, 0, 1, 3, 4, -1]], dtype=np.int64)
    # ranks: class 3 at 0 and 3, class 7 at 1 and 2, class 9 at 4: a 2 : 2 tie goes to the class with the nearer member
    c, v, d, i = vote_of(dist, ids, labels, 5, 3)
    assert c.tolist() == [[3, 7, 9]] and v.tolist() == [[2, 2, 1]] and i.tolist() == [[2, 0, 4]]
    assert d.tolist() == [[np.float32(0.1), np.float32(0.2), np.float32(0.5)]]
    assert c.dtype == np.int32 and v.dtype == np.int32 and d.dtype == np.float32 and i.dtype == np.int64
    # k = 3 cuts the list after ranks 0 ... 2: class 7 has two entries, class 3 one
    c, v, d, i = vote_of(dist, ids, labels, 3, 3)
    assert c.tolist() == [[7, 3, -1]] and v.tolist() == [[2, 1, 0]] and i.tolist() == [[0, 2, -1]] and d[0, 2] == INF
    # k = 1: the nearest neighbour's class
    c, v, d, i = vote_of(dist, ids, labels, 1, 1)
    assert c.tolist() == [[3]] and v.tolist() == [[1]] and i.tolist() == [[2]] and d.tolist() == [[np.float32(0.1)]]
    # all labels distinct, m = k: the ranking itself with votes all 1
    distinct = np.array([50, 40, 30, 20, 2 ** 31 - 1, 0, 1], dtype=np.int64)
    got = vote_of(dist, ids, distinct, 6, 6)
    assert got[0].tolist() == [[30, 50, 40, 20, 2 ** 31 - 1, -1]] and got[1].tolist() == [[1, 1, 1, 1, 1, 0]]
    assert got[3].tolist() == ids.tolist() and same_votes((got[0], got[1], got[2], got[3]), (got[0], got[1], dist, ids))
    # an empty list
    c, v, d, i = vote_of(np.full((1, 4), np.inf, dtype=np.float32), np.full((1, 4), -1, dtype=np.int64), labels, 4, 2)
    assert c.tolist() == [[-1, -1]] and v.tolist() == [[0, 0]] and i.tolist() == [[-1, -1]] and np.all(d == INF)


def test_new_entry_points_on_a_null_index(clip_lib, capfd):
    L = clip_lib.lib()
    for name in SYMBOLS:
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
    q = np.zeros(8, dtype=np.float32)
    ids = np.zeros(2, dtype=np.int64)
    labels = np.zeros(4, dtype=np.int32)
    cls = np.full(4, -3, dtype=np.int32)
    votes = np.full(4, -3, dtype=np.int32)
    dist = np.full(4, -3.0, dtype=np.float32)
    out = np.full(4, -3, dtype=np.int64)
    i32p = C.POINTER(C.c_int32)
    outs = (cls.ctypes.data_as(i32p), votes.ctypes.data_as(i32p), dist.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int64)))
    lp = labels.ctypes.data_as(i32p)
    capfd.readouterr()
    assert L.clip_amd_index_vote(None, q.ctypes.data_as(C.POINTER(C.c_float)), 2, 2, 2, lp, None, *outs) is False
    assert L.clip_amd_index_vote_device(None, None, 2, 2, 2, None, None, None, None, None, None) is False
    assert L.clip_amd_index_vote_ids(None, ids.ctypes.data_as(C.POINTER(C.c_int64)), 2, 2, 2, 1, lp, None, *outs) is False
    assert L.clip_amd_index_vote_graph(None, 2, 2, lp, None, *outs) is False
    assert L.clip_amd_index_vote_graph_device(None, 2, 2, None, None, None, None, None, None) is False
    assert capfd.readouterr().err.count("index is NULL") == 5
    assert L.clip_amd_test_index_vote_block(None, 128) == -1
    assert np.all(cls == -3) and np.all(votes == -3) and np.all(dist == -3.0) and np.all(out == -3)


def test_bench_hook_without_a_device():
    code = "import clip_cpp_amd as c; print('MICROS', c.bench_vote_graph('f16', 1024, 64, 5, 1, 8, 0, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("MICROS")[1]) == -1.0


def test_arguments_are_checked_before_the_library(clip_lib):
    ix = object.__new__(clip_lib.Index)                  # no handle: a call that reached the library would raise "the index is closed"
    ix.dim = 4
    ix.handle = None
    ix.__class__ = type("SixRows", (clip_lib.Index,), {"__len__": lambda self: 6})
    q = np.zeros((3, 4), dtype=np.float32)
    good = np.array([0, 1, -1, 5, 2 ** 31 - 1, 0])
    calls = {
        "vote": lambda k, m, lab: ix.vote(q, k, lab, m=m),
        "vote_ids": lambda k, m, lab: ix.vote_ids([0, 1], k, lab, m=m),
        "vote_graph": lambda k, m, lab: ix.vote_graph(k, lab, m=m),
    }
    for name, call in calls.items():
        for k, m in ((5, 0), (5, 6), (1025, 1), (0, 0), (0, 1)):
            with pytest.raises(ValueError):
                call(k, m, good)
        for bad in (good[:5], np.append(good, 1), np.array([0, 1, -2, 5, 7, 0]), np.array([0, 1, 2 ** 31, 5, 7, 0]), good.astype(np.float32), None):
            with pytest.raises(ValueError):
                call(5, 2, bad)
        with pytest.raises(RuntimeError, match="closed"):
            call(5, 5, good)                             # well-formed arguments go on to the library
    for k, m in ((5, 0), (5, 6), (1025, 1)):
        with pytest.raises(ValueError):
            ix.vote_device(0, 3, k, 0, 0, 0, 0, 0, m=m)
        with pytest.raises(ValueError):
            ix.vote_graph_device(k, 0, 0, 0, 0, 0, m=m)
    lab, _ = ix._labels(np.array([0, 1, -1, 5, 2 ** 31 - 1, 0], dtype=np.int64))
    assert lab.dtype == np.int32 and lab.tolist() == [0, 1, -1, 5, 2 ** 31 - 1, 0]


def _search(*args):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def _database(d, gridded):
    """a database whose model does not exist: a run that got as far as loading the model says so"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "images.paths"), "w") as f:
        f.write("no/such/model.gguf\ncats/a.png\ncats/b.png\ndogs/c.png\n")
    with open(os.path.join(d, "images.index"), "wb") as f:
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 8, 1, 3))
    if gridded:
        with open(os.path.join(d, "images.regions"), "w") as f:
            f.write("grid 2\n")


def test_usage(capsys):
    from clip_cpp_amd import image_search
    assert image_search.main([]) == 1
    out = capsys.readouterr().out
    assert "file [options] IMAGE [IMAGE ...]" in out and "audit [options]" in out and "{build|search|dedup}" in out
    assert "file   [-m MODEL]" in image_search.__doc__ and "audit  [-m MODEL]" in image_search.__doc__ and "Index.vote_graph" in image_search.__doc__
    for command in ("file", "audit"):
        with pytest.raises(SystemExit):
            image_search.main([command, "-h"])
        out = capsys.readouterr().out
        assert "Usage: python -m clip_cpp_amd.image_search %s" % command in out and "--labels FILE" in out and "-k K" in out
    p = image_search._parse_vote(["--db", "x", "-k", "7", "-n", "2", "--in", "a/", "--in", "b/", "q.png", "r.png"], True)
    assert p["rest"] == ["q.png", "r.png"] and p["k"] == 7 and p["results"] == 2 and p["in"] == ["a/", "b/"] and p["db"] == "x"
    p = image_search._parse_vote([], False)
    assert p["k"] == 10 and p["labels"] is None and image_search._parse_vote([], True) is None
    assert image_search._parse_vote(["x.png"], True)["results"] == 3
    for bad in (["-k", "0"], ["-k", "1025"], ["-k", "x"], ["-n", "3"], ["x.png"], ["--like", "x"]):
        assert image_search._parse_vote(bad, False) is None, bad
    r = _search("audit", "stray.png")
    assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search audit" in r.stdout


def test_labels_from_folders_and_from_a_file(tmp_path):
    from clip_cpp_amd import image_search
    paths = ["cats/a.png", "dogs/c.png", "cats/b.png", "top.png", "cats/sub/d.png"]
    labels, names = image_search.read_labels(paths)
    assert labels.dtype == np.int32 and labels.tolist() == [0, 1, 0, 2, 3] and names == ["cats", "dogs", "", "cats/sub"]
    f = tmp_path / "labels.tsv"
    f.write_text("pets\tcats/a.png\nwild life\ttop.png\n\npets\tdogs/c.png\n")
    labels, names = image_search.read_labels(paths, str(f))
    assert labels.tolist() == [0, 0, -1, 1, -1] and names == ["pets", "wild life"]
    f.write_text("pets\tcats/a.png\npets\tcats/zebra.png\n")
    with pytest.raises(ValueError, match="cats/zebra.png"):
        image_search.read_labels(paths, str(f))
    f.write_text("no tab here\n")
    with pytest.raises(ValueError, match="label<TAB>path"):
        image_search.read_labels(paths, str(f))
    lines = image_search.vote_lines([1, 0, -1], [3, 2, 0], [0.25, 0.5, np.inf], [1, 2, -1], 5, ["cats", "dogs"], paths)
    assert lines == ["  3/5 0.250000 dogs ~ dogs/c.png", "  2/5 0.500000 cats ~ cats/b.png"]


def test_routing_without_a_model(tmp_path):
    g, plain = tmp_path / "g", tmp_path / "plain"
    _database(g, True)
    _database(plain, False)
    for command, extra in (("file", ["cats/a.png"]), ("file", ["some/file.png"]), ("audit", [])):
        r = _search(command, "--db", g, *extra)
        assert r.returncode == 1, (command, r.stdout[-1000:], r.stderr[-1000:])
        assert str(g) in r.stderr and "--grid" in r.stderr and "`%s`" % command in r.stderr and "Unable to load model" not in r.stdout
        # a plain database gets as far as the model, which does not exist
        r = _search(command, "--db", plain, *extra)
        assert r.returncode == 1 and "Unable to load model from no/such/model.gguf" in r.stdout, (command, r.stdout[-1000:], r.stderr[-1000:])
        # a labels file with a path the database does not hold: named, before any model is loaded
        bad = tmp_path / "bad.tsv"
        bad.write_text("pets\tcats/a.png\npets\tcats/zebra.png\n")
        r = _search(command, "--db", plain, "--labels", bad, *extra)
        assert r.returncode == 1 and "cats/zebra.png" in r.stderr and "Unable to load model" not in r.stdout
    assert (plain / "images.paths").read_text() == "no/such/model.gguf\ncats/a.png\ncats/b.png\ndogs/c.png\n"
