"""CPU tier of distinct search (Index.search_distinct / search_ids_distinct, `search --distinct R`): the option parsing and help texts,
the refusal of a gridded database before any model is loaded, the argument checks that need no device, the new entry points on NULL
arguments, and the plain-Python definition of the walk (tests/distinct_common.py) on hand-written cases."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from distinct_common import collapse, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clip_amd_index_search_distinct", "clip_amd_index_search_distinct_device", "clip_amd_index_search_ids_distinct",
       "clip_amd_test_index_distinct_block", "clip_amd_bench_search_distinct"]


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def _search(*argv):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in argv]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def _parse(argv, **kw):
    from clip_cpp_amd import image_search
    return image_search._parse(list(argv), kw.pop("build", False), **kw)


def test_distinct_parsing(capsys):
    p = _parse(["--distinct", "0.05", "a", "red", "apple"])
    assert p is not None and p["distinct"] == 0.05 and p["rest"] == ["a", "red", "apple"] and p["results"] == 5 and p["max_distance"] is None
    p = _parse(["--distinct", "0.05", "-n", "3", "--in", "pics/", "--like", "pics/a.png"])
    assert p["distinct"] == 0.05 and p["results"] == 3 and p["in"] == ["pics/"] and p["like"] == "pics/a.png"
    assert "distinct" not in _parse(["a", "cat"])                         # a plain search is what it was
    assert _parse(["--distinct", "0.05", "-d", "0.2", "a cat"]) is None
    assert _parse(["-d", "0.2", "--distinct", "0.05", "a cat"]) is None
    assert "--distinct and -d cannot be combined" in capsys.readouterr().out
    assert _parse(["--distinct"]) is None                                 # without a value
    assert _parse(["--distinct", "close", "a cat"]) is None
    assert _parse(["--distinct", "nan", "a cat"]) is None
    for mode in ({"build": True}, {"dedup": True}, {"neighbors": True}):
        assert _parse(["--distinct", "0.05", "dir"], **mode) is None, mode
        assert "unrecognized argument: --distinct" in capsys.readouterr().out


def test_help_and_docstring(capsys):
    from clip_cpp_amd import image_search
    image_search._help(False, dict(threads=4, verbose=1, db=".", results=5))
    out = capsys.readouterr().out
    assert "--distinct R" in out and "not the whole index" in out and "(+N)" in out
    image_search._help(False, dict(verbose=1, db=".", results=5), neighbors=True)
    assert "--distinct" not in capsys.readouterr().out
    assert "--distinct R" in image_search.__doc__ and "(+%d)" in image_search.__doc__


def _database(d, gridded):
    os.makedirs(d, exist_ok=True)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\n")
    with open(d / "images.index", "wb") as f:                             # header only: nothing reads the rows before the check
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 8, 1, 5 if gridded else 1))
    if gridded:
        (d / "images.regions").write_text("grid 2\n0 0 0 10 10\n0 0 0 5 5\n0 5 0 5 5\n0 0 5 5 5\n0 5 5 5 5\n")


def test_gridded_database_is_refused_before_the_model(tmp_path):
    g, plain = tmp_path / "g", tmp_path / "plain"
    _database(g, True)
    _database(plain, False)
    for argv in (["search", "--db", g, "--distinct", "0.05", "a cat"], ["search", "--db", g, "--distinct", "0.05", "--like", "img/a.png"]):
        r = _search(*argv)
        assert r.returncode == 1, (r.stdout[-1000:], r.stderr[-1000:])
        assert "was built with --grid" in r.stderr and "`search --distinct` does not support such a database yet" in r.stderr
        assert str(g) in r.stderr and "Unable to load model" not in r.stdout
    r = _search("search", "--db", plain, "--distinct", "0.05", "a cat")     # a plain database gets as far as the model, which does not exist
    assert r.returncode == 1 and "Unable to load model" in r.stdout and "--grid" not in r.stderr


def test_usage_errors_print_the_usage(tmp_path):
    _database(tmp_path / "d", False)
    for extra in (["--distinct", "0.05", "-d", "0.1", "a cat"], ["--distinct"], ["--distinct", "x", "a cat"]):
        r = _search("search", "--db", tmp_path / "d", *extra)
        assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search search" in r.stdout, extra


def test_python_argument_checks_need_no_device(clip_lib):
    ix = clip_lib.Index.__new__(clip_lib.Index)                           # no context, no handle: a check that passed would say "closed"
    ix.dim, ix.handle = 8, None
    q = np.zeros((3, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="queries must be"):
        ix.search_distinct(np.zeros((3, 7), dtype=np.float32), 5, 0.05)
    with pytest.raises(ValueError, match="queries must be"):
        ix.search_distinct(np.zeros((2, 3, 8), dtype=np.float32), 5, 0.05)
    with pytest.raises(ValueError, match="k = 6 exceeds pool = 5"):
        ix.search_distinct(q, 6, 0.05, pool=5)
    with pytest.raises(ValueError, match="radius is NaN"):
        ix.search_distinct(q, 5, float("nan"))
    with pytest.raises(ValueError, match="pool = 1025 outside"):
        ix.search_distinct(q, 5, 0.05, pool=1025)
    with pytest.raises(ValueError, match="pool = -1 outside"):
        ix.search_ids_distinct([0, 1], 5, 0.05, pool=-1)
    with pytest.raises(ValueError, match="k = 0 outside"):
        ix.search_ids_distinct([0, 1], 0, 0.05)
    with pytest.raises(ValueError, match="k = 1025 outside"):
        ix.search_distinct(q, 1025, 0.05)
    with pytest.raises(ValueError, match="radius is NaN"):
        ix.search_distinct_device(0, 1, 5, float("nan"), 0, 0, 0)
    for call in (lambda: ix.search_distinct(q, 5, 0.05), lambda: ix.search_distinct(q[0], 1024, -1.0, pool=0),
                 lambda: ix.search_ids_distinct([0], 5, 0.05, pool=5)):
        with pytest.raises(RuntimeError, match="closed"):                 # the checks passed: only the handle is missing
            call()


def test_new_entry_points_reject_null_arguments(clip_lib):
    L = clip_lib.lib()
    for name in NEW:
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
    assert L.clip_amd_index_search_distinct(None, None, 1, 5, 0.05, 0, None, None, None, None) is False
    assert L.clip_amd_index_search_distinct_device(None, None, 1, 5, 0.05, 0, None, None, None, None) is False
    assert L.clip_amd_index_search_ids_distinct(None, None, 1, 5, 0.05, 0, 1, None, None, None, None) is False
    assert L.clip_amd_test_index_distinct_block(None, 3) == -1
    code = "import clip_cpp_amd as c; print('us', c.bench_search_distinct('f16', 1024, 64, 4, 5, 64, 0.01, 4, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def test_walk_on_hand_written_cases():
    a, b, c, d, e = 10, 4, 7, 2, 9
    # a chain a - b - c: b is dropped for a, and being dropped it does not drop c
    assert walk([a, b, c], {(b, a), (b, c)}, 5) == ([a, c], [1, 0])
    assert collapse([a, b, c], {(b, a), (b, c)}, 5) == [a]                # the connected component is a different answer
    # pairs are (lower id, higher id) whatever the ranks
    assert walk([a, b], {(a, b)}, 5) == ([a, b], [0, 0])
    # nothing near: the first k
    assert walk([a, b, c, d], set(), 2) == ([a, b], [0, 0])
    # k reached early: the walk stops, but a count runs over the whole pool, behind the k-th kept member too
    assert walk([a, b, c, d, e], {(d, a), (e, a), (b, c)}, 1) == ([a], [2])
    assert walk([a, b, c, d, e], {(d, a), (e, a), (b, c)}, 2) == ([a, b], [2, 1])
    assert walk([a, b, c, d, e], {(d, a), (e, a), (b, c)}, 5) == ([a, b], [2, 1])
    # a member near two kept ones is counted once, for the first
    assert walk([a, b, c], {(c, a), (b, c)}, 5) == ([a, b], [1, 0])
    # everything near everything: one hit with count = members - 1; the -1 tail is not a member
    ids = [a, b, c, d, -1, -1]
    every = {(min(x, y), max(x, y)) for x in ids[:4] for y in ids[:4] if x != y}
    assert walk(ids, every, 3) == ([a], [3])
    assert walk([-1, -1], set(), 3) == ([], [])
