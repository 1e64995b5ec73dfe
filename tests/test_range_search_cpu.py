"""CPU tier of range search / near-duplicate pairs and the `dedup` command: the NULL-index refusals of the new entry points, the grouping
function of `dedup` on hand-made pair lists, and the option and database checks of `dedup` and `search -d` that run before any device
work."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          env=_host_only_env(), cwd=ROOT, timeout=300)


def test_new_entry_points_reject_a_null_index(clip_lib, capfd):
    L = clip_lib.lib()
    lims = np.full(4, -7, dtype=np.int64)
    lp = lims.ctypes.data_as(C.POINTER(C.c_int64))
    q = np.ones((1, 32), np.float32)
    d = np.full(8, -2.0, np.float32)
    ids = np.full(8, -3, np.int64)
    fp = q.ctypes.data_as(C.POINTER(C.c_float))
    assert L.clip_amd_index_range_search(None, fp, 1, 0.5, lp, d.ctypes.data_as(C.POINTER(C.c_float)),
                                         ids.ctypes.data_as(C.POINTER(C.c_int64)), 8) == -1
    assert L.clip_amd_index_range_search(None, None, 0, 0.5, lp, None, None, 0) == -1
    assert L.clip_amd_index_pairs(None, 0.5, lp, None, None, 0) == -1
    assert L.clip_amd_index_pairs(None, float("nan"), None, None, None, -1) == -1
    assert np.all(lims == -7) and np.all(d == -2.0) and np.all(ids == -3)
    err = capfd.readouterr().err
    assert "clip_amd_index_range_search: index is NULL" in err and "clip_amd_index_pairs: index is NULL" in err
    assert clip_lib.bench_range("f16", 1000, 32, 0, 0.1, iters=0) < 0      # no device, or (on a GPU machine) iters < 1


def test_duplicate_groups_of_hand_made_pair_lists():
    from clip_cpp_amd.image_search import duplicate_groups
    assert duplicate_groups([], [], []) == []
    assert duplicate_groups(np.array([3]), np.array([8]), np.array([0.25], np.float32)) == [[(3, 0.25), (8, 0.25)]]
    got = duplicate_groups([0, 2, 5, 1, 7], [3, 3, 6, 4, 9], [0.01, 0.02, 0.03, 0.04, 0.05])
    assert got == [[(0, 0.01), (2, 0.02), (3, 0.01)], [(1, 0.04), (4, 0.04)], [(5, 0.03), (6, 0.03)], [(7, 0.05), (9, 0.05)]]
    # two components joined by a later pair; the group keys on its lowest id, members in id order, each with its nearest pair
    got = duplicate_groups([4, 1, 2, 10], [5, 2, 5, 11], [0.1, 0.2, 0.3, 0.0])
    assert got == [[(1, 0.2), (2, 0.2), (4, 0.1), (5, 0.1)], [(10, 0.0), (11, 0.0)]]
    # a chain: every member reaches the others through the edges, not directly
    got = duplicate_groups([6, 7, 8], [7, 8, 9], [0.3, 0.1, 0.2])
    assert got == [[(6, 0.3), (7, 0.1), (8, 0.1), (9, 0.2)]]


def test_dedup_help_and_usage_errors(tmp_path):
    r = _cli("dedup", "-h")
    assert r.returncode == 0
    assert "-d R, --max-distance R" in r.stdout and "Default: 0.05" in r.stdout and "not a tuned value" in r.stdout
    for args in (["dedup", "extra"], ["dedup", "-d"], ["dedup", "-d", "abc"], ["dedup", "-d", "nan"], ["dedup", "-n", "5"],
                 ["dedup", "--bogus"]):
        r = _cli(*args, "--db", tmp_path)
        assert r.returncode != 0 and "Usage: python -m clip_cpp_amd.image_search dedup" in r.stdout, (args, r.stdout)
    r = _cli()
    assert r.returncode != 0 and "{build|search|dedup}" in r.stdout
    r = _cli("search", "-h")
    assert r.returncode == 0 and "-d R, --max-distance R" in r.stdout
    assert "-n N, --results N: Number of results to display. Default: 5" in r.stdout
    r = _cli("search", "--db", tmp_path, "-d", "x", "cat")
    assert r.returncode != 0 and "Usage" in r.stdout
    r = _cli("search", "--db", tmp_path, "-d", "0.1", "-n", "3", "cat")
    assert r.returncode != 0 and "-n and -d cannot be combined" in r.stdout and "Usage" in r.stdout


def test_dedup_without_database_fails(tmp_path):
    r = _cli("dedup", "--db", tmp_path)
    assert r.returncode != 0
    assert "main: Unable to load model from" in r.stdout
    assert "images.paths" in r.stderr


def test_dedup_with_mismatched_or_missing_index_fails(tmp_path):
    (tmp_path / "images.paths").write_text("model.gguf\nimg/a.jpg\nimg/b.jpg\n")
    r = _cli("dedup", "--db", tmp_path)
    assert r.returncode != 0 and "images.index" in r.stderr
    with open(tmp_path / "images.index", "wb") as f:        # a valid header that holds 3 rows against 2 paths
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 4, 0, 3) + b"\0" * 48)
    r = _cli("dedup", "--db", tmp_path, "-d", "0.1")
    assert r.returncode != 0
    assert "main: index files size missmatch" in r.stdout
    r = _cli("search", "--db", tmp_path, "-d", "0.1", "a", "cat")
    assert r.returncode != 0 and "main: index files size missmatch" in r.stdout
