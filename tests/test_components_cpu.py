"""CPU tier of connected components (clip_amd_index_components) and `dedup --prune`: the pure-numpy grouping of image_search.py against the
union-find of duplicate_groups, option parsing and help text, and the declarations of the two new entry points.  Needs no device."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

from clip_cpp_amd import image_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def test_component_groups_hand_made():
    #          0     1    2     3    4     5     6    7
    labels = [0, 1, 0, 3, -1, 3, 0, 7]
    near = [0.25, INF, 0.5, 0.125, INF, 0.125, 0.25, INF]
    got = image_search.component_groups(labels, near)
    assert got == [[(0, 0.25), (2, 0.5), (6, 0.25)], [(3, 0.125), (5, 0.125)]]
    assert all(type(i) is int and type(d) is float for g in got for i, d in g)
    assert image_search.component_groups([], []) == []
    assert image_search.component_groups([0, 1, -1], [INF, INF, INF]) == []
    # a negative distance (a tiny negative f32 is a legal distance) and groups that interleave
    got = image_search.component_groups([0, 1, 0, 1], np.array([-1e-7, 0.0, -1e-7, 0.0], dtype=np.float32))
    assert got == [[(0, float(np.float32(-1e-7))), (2, float(np.float32(-1e-7)))], [(1, 0.0), (3, 0.0)]]


def labels_and_nearest(n, i, j, d):
    """labels (lowest id of the component, label propagation to the fixed point) and nearest distance per row from an edge list, in numpy"""
    labels = np.arange(n, dtype=np.int64)
    while True:
        nxt = labels.copy()
        np.minimum.at(nxt, i, labels[j])
        np.minimum.at(nxt, j, labels[i])
        nxt = nxt[nxt]
        if np.array_equal(nxt, labels):
            break
        labels = nxt
    near = np.full(n, np.inf, dtype=np.float32)
    np.minimum.at(near, i, d)
    np.minimum.at(near, j, d)
    return labels, near


def test_component_groups_equals_duplicate_groups_on_random_edge_lists():
    rng = np.random.default_rng(2024)
    for trial in range(300):
        n = int(rng.integers(1, 60))
        m = int(rng.integers(0, 2 * n))
        a = rng.integers(0, n, m)
        b = rng.integers(0, n, m)
        keep = a != b
        i, j = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
        d = rng.choice(np.array([-1e-7, 0.0, 0.01, 0.02, 0.03], dtype=np.float32), i.size) if trial % 2 else \
            rng.random(i.size, dtype=np.float32)
        labels, near = labels_and_nearest(n, i, j, d)
        if trial % 3 == 0 and n > 2:               # rows that are not eligible carry -1 and are on no edge
            off = np.setdiff1d(np.arange(n), np.concatenate([i, j]))[:2]
            labels[off] = -1
        assert image_search.component_groups(labels, near) == image_search.duplicate_groups(i, j, d), trial


def test_dedup_prune_parsing_and_help():
    p = image_search._parse(["--db", "x", "-d", "0.1", "--prune"], build=False, dedup=True)
    assert p["prune"] is True and p["db"] == "x" and p["max_distance"] == 0.1
    assert image_search._parse(["--prune"], build=False, dedup=True)["prune"] is True
    assert "prune" not in image_search._parse([], build=False, dedup=True)          # (as --grid: the key exists only when given)
    for other in (dict(build=False), dict(build=True), dict(build=False, update=True), dict(build=False, neighbors=True)):
        buf = io.StringIO()
        with redirect_stdout(buf):
            assert image_search._parse(["--prune", "x"], **other) is None          # only dedup knows it
        assert "unrecognized argument: --prune" in buf.getvalue()
    buf = io.StringIO()
    with redirect_stdout(buf), pytest.raises(SystemExit) as e:
        image_search._parse(["-h"], build=False, dedup=True)
    assert e.value.code == 0
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("  --prune")]
    assert len(lines) == 1 and "lowest id" in lines[0] and "never touched" in lines[0]
    assert "[--prune]" in image_search.__doc__ and "removed, %d kept" in image_search.__doc__


def test_header_and_ctypes_table_name_the_entry_points():
    import clip_cpp_amd
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    for name in ("clip_amd_index_components", "clip_amd_index_components_device"):
        assert re.search(r"\b%s\(struct clip_amd_index \* ix, float radius, const uint64_t \* (d_)?allow," % name, header), name
        assert name in clip_cpp_amd.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert callable(clip_cpp_amd.Index.components) and callable(clip_cpp_amd.Index.components_device)
