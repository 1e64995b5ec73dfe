"""CPU tier of the single-linkage tree (clip_amd_index_linkage) and `image_search groups` / `levels`: the oracle of tests/linkage_common.py
against the contract's definition by brute force on tiny graphs with ties, a host model of the kernels' pick rule (per row the minimum
(d, lowest other id); per component the minimum d, then the minimum (lo, hi) among the rows that attain it; mutual picks broken by the
lower label) against the oracle, the conventions of cut_linkage, the pure parts of the two commands, option parsing, refusals that need
no model, and the declarations of the entry points."""
import os
import re
import struct

import numpy as np
import pytest

from clip_cpp_amd import image_search
from linkage_common import forest_by_definition, kruskal, labels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_graph(rng, n, levels):
    """every pair of n rows with a distance out of `levels` values: heavy ties (levels == 1: all equal)"""
    i, j = np.triu_indices(n, 1)
    d = (rng.integers(0, levels, len(i)) / np.float32(4)).astype(np.float32)
    return i.astype(np.int64), j.astype(np.int64), d


def boruvka_model(n, i, j, d, link=np.inf):
    """the rounds of k_linkage.hip on the host, with the same keys and the same two-step choice; returns the sorted forest"""
    comp = list(range(n))
    pairs = [(float(x), int(a), int(b)) for a, b, x in zip(i, j, d) if x <= np.float32(link)]
    edges = []
    rounds = 0
    while (1 << rounds) < n:
        rounds += 1
    for _ in range(rounds):
        key = [None] * n                              # per row: (d, lowest other id) over the pairs that leave its component
        for x, a, b in pairs:
            if comp[a] != comp[b]:
                key[a] = min(key[a], (x, b)) if key[a] else (x, b)
                key[b] = min(key[b], (x, a)) if key[b] else (x, a)
        cmin, cedge = {}, {}
        for r in range(n):
            if key[r]:
                cmin[comp[r]] = min(cmin.get(comp[r], np.inf), key[r][0])
        for r in range(n):
            if key[r] and key[r][0] == cmin[comp[r]]:
                e = (min(r, key[r][1]), max(r, key[r][1]))
                cedge[comp[r]] = min(cedge.get(comp[r], e), e)
        parent = list(comp)
        for c, (lo, hi) in cedge.items():
            t = comp[hi] if comp[lo] == c else comp[lo]
            if cedge.get(t) == (lo, hi) and c < t:
                continue                              # mutual: the lower label stays the root
            parent[c] = t
            edges.append((cmin[c], lo, hi))
        for r in range(n):                            # flatten
            x = parent[r]
            seen = 0
            while parent[x] != x:
                x = parent[x]
                seen += 1
                assert seen <= n, "a cycle"
            comp[r] = x
    edges.sort()
    return (np.array([e[1] for e in edges], dtype=np.int64), np.array([e[2] for e in edges], dtype=np.int64),
            np.array([e[0] for e in edges], dtype=np.float32))


def same_forest(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("seed", range(60))
def test_oracle_is_the_definition_on_tiny_graphs_with_ties(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 9))
    i, j, d = random_graph(rng, n, (1, 2, 3, 5)[seed % 4])
    for link in (np.inf, 0.25, 0.0, -1.0):
        want = forest_by_definition(n, i, j, d, link)
        got = kruskal(n, i, j, d, link)
        assert same_forest(got, want)
        assert np.array_equal(labels_of(n, got[0], got[1]), labels_of(n, i[d <= link], j[d <= link]))     # spans every component
    full = kruskal(n, i, j, d)
    assert len(full[0]) == n - 1


@pytest.mark.parametrize("seed", range(300))
def test_the_kernels_pick_rule_gives_the_oracles_forest(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 40))
    levels = (1, 2, 3, 8)[seed % 4]                   # 1: every distance equal
    i, j, d = random_graph(rng, n, levels)
    keep = rng.random(len(i)) < (1.0, 0.5, 0.2)[seed % 3]         # a pair list with holes is still a graph
    i, j, d = i[keep], j[keep], d[keep]
    for link in (np.inf, 0.25):
        assert same_forest(boruvka_model(n, i, j, d, link), kruskal(n, i, j, d, link))


def test_all_equal_distances_give_the_star_of_row_0():
    i, j, d = random_graph(np.random.default_rng(0), 30, 1)
    lo, hi, dd = kruskal(30, i, j, d)
    assert np.all(lo == 0) and np.array_equal(hi, np.arange(1, 30)) and np.all(dd == 0)
    assert same_forest(boruvka_model(30, i, j, d), (lo, hi, dd))


def test_cut_linkage_conventions(clip_lib):
    cut = clip_lib.cut_linkage
    # rows 1 - 4 - 2 a chain, 3 - 6 a pair, 0 single, 5 not eligible; the edges in the edge order
    lo = np.array([1, 3, 2, 1], dtype=np.int64)
    hi = np.array([4, 6, 4, 3], dtype=np.int64)
    d = np.array([0.1, 0.2, 0.2, 0.5], dtype=np.float32)
    eligible = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)
    every = cut(7, lo, hi, d, eligible=eligible)
    assert every.dtype == np.int64 and every.tolist() == [0, 1, 1, 1, 1, -1, 1]
    assert cut(7, lo, hi, d, radius=0.2, eligible=eligible).tolist() == [0, 1, 1, 3, 1, -1, 3]       # <=: both edges at 0.2 are kept
    assert cut(7, lo, hi, d, radius=np.nextafter(np.float32(0.2), np.float32(0)), eligible=eligible).tolist() == [0, 1, 2, 3, 1, -1, 6]
    assert cut(7, lo, hi, d, radius=-1.0, eligible=eligible).tolist() == [0, 1, 2, 3, 4, -1, 6]
    assert cut(7, lo, hi, d, radius=0.2).tolist() == [0, 1, 1, 3, 1, 5, 3]                           # no eligible: every row counts
    assert cut(7, lo, hi, d, n_groups=2, eligible=eligible).tolist() == every.tolist()               # the forest has two trees
    assert cut(7, lo, hi, d, n_groups=3, eligible=eligible).tolist() == [0, 1, 1, 3, 1, -1, 3]
    assert cut(7, lo, hi, d, n_groups=4, eligible=eligible).tolist() == [0, 1, 1, 3, 1, -1, 6]       # (0.2, 2, 4) goes before (0.2, 3, 6)
    assert cut(7, lo, hi, d, n_groups=6, eligible=eligible).tolist() == [0, 1, 2, 3, 4, -1, 6]
    shuffled = np.array([2, 0, 3, 1])                                                                # the device form's order is its own
    assert cut(7, lo[shuffled], hi[shuffled], d[shuffled], n_groups=4, eligible=eligible).tolist() == [0, 1, 1, 3, 1, -1, 6]
    assert cut(3, [], [], []).tolist() == [0, 1, 2] and cut(0, [], [], []).shape == (0,)
    for bad in (dict(n_groups=1), dict(n_groups=7), dict(n_groups=0), dict(radius=0.2, n_groups=3), dict(radius=float("nan"))):
        with pytest.raises(ValueError):
            cut(7, lo, hi, d, eligible=eligible, **bad)
    with pytest.raises(ValueError):
        cut(7, lo, hi, d, eligible=np.array([1, 1, 1, 0, 1, 0, 1], dtype=bool))                      # an edge at a row outside E
    with pytest.raises(ValueError):
        cut(7, hi, lo, d)                                                                            # lo < hi
    with pytest.raises(ValueError):
        cut(4, lo, hi, d)
    with pytest.raises(ValueError):
        cut(7, lo, hi, d[:3])


def test_cut_linkage_equals_the_components_of_the_pair_list():
    import clip_cpp_amd
    rng = np.random.default_rng(5)
    n = 60
    i, j, d = random_graph(rng, n, 12)
    keep = rng.random(len(i)) < 0.08
    i, j, d = i[keep], j[keep], d[keep]
    lo, hi, dd = kruskal(n, i, j, d)
    for radius in np.unique(d).tolist() + [-1.0, 0.1, 9.0]:
        near = d <= np.float32(radius)
        assert np.array_equal(clip_cpp_amd.cut_linkage(n, lo, hi, dd, radius=radius), labels_of(n, i[near], j[near]))
    trees = n - len(lo)
    for groups in (trees, trees + 1, n - 1, n):
        labels = clip_cpp_amd.cut_linkage(n, lo, hi, dd, n_groups=groups)
        assert len(np.unique(labels)) == groups


def test_tree_groups_and_level_rows():
    paths = 8
    # two bursts {0, 2, 5} and {1, 4}, far singles 3, 6, 7; the whole tree, sorted
    lo = np.array([0, 1, 2, 0, 3, 3, 5], dtype=np.int64)
    hi = np.array([2, 4, 5, 1, 6, 7, 6], dtype=np.int64)
    d = np.array([0.01, 0.02, 0.03, 0.4, 0.5, 0.5, 0.9], dtype=np.float32)
    groups, kept, cut = image_search.tree_groups(paths, lo, hi, d, 5)
    assert groups == [[(0, pytest.approx(0.01)), (2, pytest.approx(0.01)), (5, pytest.approx(0.03))],
                      [(1, pytest.approx(0.02)), (4, pytest.approx(0.02))]]
    assert kept == pytest.approx(0.03) and cut == pytest.approx(0.4)
    groups, kept, cut = image_search.tree_groups(paths, lo, hi, d, 5, min_size=1)
    assert [len(g) for g in groups] == [3, 2, 1, 1, 1] and [g[0][0] for g in groups] == [0, 1, 3, 6, 7] and groups[2] == [(3, np.inf)]
    groups, kept, cut = image_search.tree_groups(paths, lo, hi, d, 1)
    assert [len(g) for g in groups] == [8] and cut == np.inf and kept == pytest.approx(0.9)
    groups, kept, cut = image_search.tree_groups(paths, lo, hi, d, 8)
    assert groups == [] and kept == -np.inf and cut == pytest.approx(0.01)
    with pytest.raises(ValueError):
        image_search.tree_groups(paths, lo, hi, d, 9)
    table = image_search.level_rows(paths, lo, hi, d, 7)
    assert [r[1:] for r in table] == [(1, 2, 2), (2, 4, 2), (2, 5, 3), (1, 5, 5), (2, 8, 5), (1, 8, 8)]      # the two edges at 0.5: one row
    assert [r[0] for r in table] == pytest.approx([0.01, 0.02, 0.03, 0.4, 0.5, 0.9])
    table = image_search.level_rows(paths, lo, hi, d, 2)
    assert [r[1:] for r in table] == [(2, 5, 3), (1, 8, 8)]
    assert image_search.level_rows(paths, lo, hi, d, 100) == image_search.level_rows(paths, lo, hi, d, 7)
    assert image_search.level_rows(1, [], [], [], 5) == []
    for rows in (1, 3, 20):                                                                          # always monotone, always ends at one group
        t = image_search.level_rows(paths, lo, hi, d, rows)
        assert t[-1][1:] == (1, 8, 8)
        assert all(a[0] < b[0] and a[2] <= b[2] and a[3] <= b[3] for a, b in zip(t, t[1:]))


def test_option_parsing():
    G = lambda argv: image_search._parse(argv, build=False, groups=True)
    V = lambda argv: image_search._parse(argv, build=False, levels=True)
    p = G(["--db", "x", "-n", "12", "--in", "a/", "--in", "b/", "--min", "3", "-v", "0"])
    assert (p["db"], p["results"], p["in"], p["min_size"], p["verbose"]) == ("x", 12, ["a/", "b/"], 3, 0)
    assert G(["-n", "4"])["min_size"] == 2
    assert G([]) is None and G(["--db", "x"]) is None                  # -n is the question
    assert G(["-n", "0"]) is None and G(["-n", "x"]) is None
    assert G(["-n", "4", "extra"]) is None and G(["-n", "4", "-d", "0.1"]) is None and G(["-n", "4", "-t", "2"]) is None
    p = V(["--db", "x"])
    assert p["results"] == image_search.LEVEL_ROWS and p["in"] == []
    assert V(["-n", "7", "--in", "a/"])["results"] == 7
    assert V(["-n", "0"]) is None and V(["--min", "2"]) is None and V(["q"]) is None and V(["-d", "0.1"]) is None
    assert image_search._parse(["--min", "2", "q"], build=False) is None        # search has no --min


def test_usage_texts(capsys):
    assert image_search.main(["groups"]) == 1
    out = capsys.readouterr().out
    assert "image_search groups [options] -n N" in out and "--min M" in out and "--in <prefix>" in out
    for cmd, usage in (("groups", "image_search groups [options] -n N"), ("levels", "image_search levels [options]")):
        with pytest.raises(SystemExit) as e:
            image_search.main([cmd, "-h"])
        assert e.value.code == 0 and usage in capsys.readouterr().out
    assert image_search.main(["nothing"]) == 1
    out = capsys.readouterr().out
    assert "image_search groups [options] -n N" in out and "image_search levels [options]" in out
    doc = image_search.__doc__
    assert "image_search groups [-m MODEL] [-v N] [--db DIR] -n N [--in PREFIX]... [--min M]" in doc
    assert "image_search levels [-m MODEL] [-v N] [--db DIR] [--in PREFIX]... [-n ROWS]" in doc
    assert "Index.linkage" in doc and "longest link kept %f, cut at %f" in doc and "main: %d images, %d levels" in doc


def test_refusals_before_any_model_load(tmp_path, capsys):
    d = tmp_path / "db"
    os.makedirs(d)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\nimg/b.png\nother/c.png\n")
    (d / "images.regions").write_text("grid 2\n")
    for argv in (["groups", "--db", str(d), "-n", "2"], ["levels", "--db", str(d)]):
        assert image_search.main(argv) == 1
        got = capsys.readouterr()
        assert "`%s` does not support such a database yet" % argv[0] in got.err and "Unable to load model" not in got.out
    os.remove(d / "images.regions")
    with open(d / "images.index", "wb") as fh:       # a header is all _read_db looks at: 3 rows
        fh.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 32, 1, 3))
    for argv in (["groups", "--db", str(d), "-n", "2"], ["levels", "--db", str(d)]):
        assert image_search.main(argv) == 1          # a run that got as far as loading the model says so on stdout
        assert "Unable to load model" in capsys.readouterr().out


def test_wrapper_rejects_a_nan_before_the_library(clip_lib):
    class Unreachable(clip_lib.Index):
        def __init__(self):                    # no handle: every library call would need one
            pass

        def __len__(self):
            return 10

        def _live(self):
            raise AssertionError("the library was reached")

    ix = Unreachable()
    with pytest.raises(ValueError, match="NaN"):
        ix.linkage(float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        ix.linkage_device(1, 1, 1, 1, link=float("nan"))
    with pytest.raises(ValueError):
        ix.linkage(allow=np.ones(9, dtype=bool))
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.linkage(0.5, allow=[0, 1, 9])
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.linkage_device(1, 1, 1, 1)


def test_entry_points_are_declared_and_refuse_without_an_index(clip_lib, capfd):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    assert re.search(r"int64_t clip_amd_index_linkage\(struct clip_amd_index \* ix, float link, const uint64_t \* allow, int64_t \* lo, "
                     r"int64_t \* hi, float \* distances\);", header)
    assert re.search(r"bool clip_amd_index_linkage_device\(struct clip_amd_index \* ix, float link, const uint64_t \* d_allow, int64_t \* d_lo, "
                     r"int64_t \* d_hi,\s+float \* d_distances, int64_t \* d_count\);", header)
    assert re.search(r"float clip_amd_bench_linkage\(int dtype, int64_t n, int dim, int copies, int iters\);", header)
    for name in ("clip_amd_index_linkage", "clip_amd_index_linkage_device", "clip_amd_bench_linkage"):
        assert name in clip_lib.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert "Device memory beyond the index: 32 bytes per row" in header
    assert callable(clip_lib.Index.linkage) and callable(clip_lib.Index.linkage_device) and callable(clip_lib.cut_linkage)
    assert callable(clip_lib.bench_linkage)
    L = clip_lib.lib()
    lo = np.full(4, -7, dtype=np.int64)
    hi = np.full(4, -7, dtype=np.int64)
    dist = np.full(4, -7, dtype=np.float32)
    i64p, f32p = L.clip_amd_index_linkage.argtypes[3], L.clip_amd_index_linkage.argtypes[5]
    capfd.readouterr()
    assert L.clip_amd_index_linkage(None, 0.5, None, lo.ctypes.data_as(i64p), hi.ctypes.data_as(i64p), dist.ctypes.data_as(f32p)) == -1
    assert L.clip_amd_index_linkage_device(None, 0.5, None, lo.ctypes.data, hi.ctypes.data, dist.ctypes.data, lo.ctypes.data) is False
    assert capfd.readouterr().err.count("index is NULL") == 2
    assert np.all(lo == -7) and np.all(hi == -7) and np.all(dist == -7)


def test_build_lists_name_the_kernel_file():
    mk = re.search(r"^KERNELS := (.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1).split()
    src = re.search(r"^HIP_SOURCES = \[(.*)\]$", open(os.path.join(ROOT, "clip_cpp_amd", "build.py")).read(), re.M).group(1)
    src = [s.strip().strip('"')[:-4] for s in src.split(",")]
    assert "k_linkage" in mk and mk.index("k_linkage") == src.index("k_linkage")
    assert os.path.exists(os.path.join(ROOT, "clip_cpp_amd", "csrc", "k_linkage.hip"))
