"""CPU tier of the mutual-reachability tree (clip_amd_index_linkage_core, Index.linkage_core, cut_linkage_sized, `groups --core`): the
oracle of tests/linkage_core_common.py against the contract's definition on tiny graphs where ties are the rule, the rounds of
k_linkage.hip on the host over the weights, cut_linkage_sized against a brute force over every level, the option parsing, and the entry
points on a NULL index and on arguments the wrapper refuses before the library."""
import os
import re

import numpy as np
import pytest

from clip_cpp_amd import image_search
from linkage_core_common import core_by_definition, core_distances, core_kruskal, kruskal, labels_of, mutual_reach
from test_linkage_cpu import boruvka_model, random_graph, same_forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mutual_reach_is_the_f32_maximum():
    i, j = np.array([0, 0, 1]), np.array([1, 2, 2])
    d = np.array([0.5, 0.25, 2.0], dtype=np.float32)
    core = np.array([0.375, np.inf, -np.inf], dtype=np.float32)
    w = mutual_reach(i, j, d, core)
    assert w.dtype == np.float32 and w.tolist() == [np.inf, 0.375, np.inf]
    assert mutual_reach(i, j, d, np.full(3, -np.inf)).tolist() == d.tolist()


@pytest.mark.parametrize("seed", range(60))
def test_oracle_is_the_definition_on_tiny_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 13))
    i, j, d = random_graph(rng, n, (1, 2, 3, 5)[seed % 4])
    k = int(rng.integers(0, n + 2))                   # k >= n: every core distance is +inf
    core = core_distances(n, i, j, d, k)
    if seed % 5 == 0:
        core[rng.integers(0, n)] = np.inf             # +inf next to finite ones
    assert np.all(np.isinf(core)) == (k >= n or k == 0) or seed % 5 == 0
    for link in (np.inf, 0.5, 0.25, 0.0, -1.0):
        want = core_by_definition(n, i, j, d, core, link)
        assert same_forest(core_kruskal(n, i, j, d, core, link), want)
    full = core_kruskal(n, i, j, d, core)
    assert len(full[0]) == n - 1                      # +inf weights are in the graph at link = inf
    if k == 0 and seed % 5:
        assert same_forest(full, kruskal(n, i, j, d))


def test_all_weights_tied_and_infinite_cores():
    n = 12
    i, j, d = random_graph(np.random.default_rng(0), n, 3)
    for core in (np.full(n, 7.0, dtype=np.float32), np.full(n, np.inf, dtype=np.float32)):     # above every distance: all weights equal
        for forest in (core_kruskal(n, i, j, d, core), core_by_definition(n, i, j, d, core)):
            assert np.all(forest[0] == 0) and np.array_equal(forest[1], np.arange(1, n)) and np.all(forest[2] == core[0])
    core = np.full(n, np.inf, dtype=np.float32)
    assert all(len(a) == 0 for a in core_kruskal(n, i, j, d, core, 100.0))      # +inf weights are in the graph only at link = inf
    core[:4] = -np.inf                                 # four rows with finite weights among them, eight at +inf from everything
    lo, hi, w = core_kruskal(n, i, j, d, core)
    assert same_forest((lo, hi, w), core_by_definition(n, i, j, d, core))
    assert np.all(np.isfinite(w[:3])) and np.all(hi[:3] < 4) and np.all(np.isinf(w[3:]))
    assert np.all(lo[3:] == 0) and np.array_equal(hi[3:], np.arange(4, n))       # ordered by (lo, hi)


@pytest.mark.parametrize("seed", range(100))
def test_the_kernels_pick_rule_gives_the_oracles_forest_under_ties(seed):
    """the rounds of k_linkage.hip (its host model) over the weights: a row's key is (w, lowest outside id at w), and under w every row
    closer to x than core[x] is at the same weight from x"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(2, 40))
    i, j, d = random_graph(rng, n, (2, 3, 8, 50)[seed % 4])
    core = core_distances(n, i, j, d, int(rng.integers(1, 8)))
    w = mutual_reach(i, j, d, core)
    for link in (np.inf, float(np.median(w))):
        use = w <= np.float32(link)
        assert same_forest(boruvka_model(n, i[use], j[use], w[use]), core_kruskal(n, i, j, d, core, link))


def sized_data():
    """5 well-separated bursts of 12 rows and 40 scattered rows, the distances from numpy: (n, i, j, d) over every pair"""
    rng = np.random.default_rng(11)
    dim = 64
    centres = rng.standard_normal((5, dim))
    rows = np.concatenate([c + 0.02 * rng.standard_normal((12, dim)) for c in centres] + [rng.standard_normal((40, dim))])
    rows = rows[rng.permutation(len(rows))]
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    n = len(rows)
    i, j = np.triu_indices(n, 1)
    d = (1.0 - np.einsum("ij,ij->i", rows[i], rows[j])).astype(np.float32)
    return n, i.astype(np.int64), j.astype(np.int64), d


def brute_force_sized(n, lo, hi, d, n_groups, min_size, eligible=None):
    """every distinct level of the tree, each cut from scratch: the largest with exactly n_groups groups of at least min_size rows"""
    best = None
    counts = set()
    for level in np.unique(d):
        labels = labels_of(n, lo[d <= level], hi[d <= level], eligible)
        sizes = np.bincount(labels[labels >= 0], minlength=n)
        count = int(np.count_nonzero(sizes >= min_size))
        counts.add(count)
        if count == n_groups:
            best = (labels, float(level))
    return best, counts


@pytest.mark.parametrize("k", (0, 4))
def test_cut_linkage_sized_equals_a_brute_force_over_every_level(clip_lib, k):
    n, i, j, d = sized_data()
    core = core_distances(n, i, j, d, k)
    lo, hi, w = core_kruskal(n, i, j, d, core)
    assert len(lo) == n - 1
    hit = 0
    for min_size in (1, 2, 5, 12, 13):
        for n_groups in (1, 2, 4, 5, 6, 9, 30, n):
            want, counts = brute_force_sized(n, lo, hi, w, n_groups, min_size)
            if want is None:
                with pytest.raises(ValueError) as e:
                    clip_lib.cut_linkage_sized(n, lo, hi, w, n_groups, min_size=min_size)
                named = [int(t) for t in re.findall(r"\d+", str(e.value).split("occur:")[1])]
                assert named == sorted(counts) and n_groups not in named
                continue
            hit += 1
            labels, radius = clip_lib.cut_linkage_sized(n, lo, hi, w, n_groups, min_size=min_size)
            assert radius == want[1] and np.array_equal(labels, want[0])
            assert np.array_equal(labels, clip_lib.cut_linkage(n, lo, hi, w, radius=radius))
    assert hit >= 8
    # the level the data was built for: two rows of a burst are at about 0.0004, any other two rows at about 1, so at 0.05 the cut is
    # the five bursts and nothing else, and cut_linkage_sized finds a level for (5, 12) and for (5, 2)
    sizes = np.bincount(clip_lib.cut_linkage(n, lo, hi, w, radius=0.05), minlength=n)
    assert sorted(sizes[sizes >= 2].tolist()) == [12] * 5
    assert clip_lib.cut_linkage_sized(n, lo, hi, w, 5, min_size=12)[1] >= 0.0
    labels, _ = clip_lib.cut_linkage_sized(n, lo, hi, w, 5, min_size=2)            # defaults, any edge order, an eligible set
    perm = np.random.default_rng(1).permutation(n - 1)
    again, _ = clip_lib.cut_linkage_sized(n, lo[perm], hi[perm], w[perm], 5)
    assert np.array_equal(labels, again)
    eligible = np.ones(n + 3, dtype=bool)
    eligible[n:] = False
    padded, _ = clip_lib.cut_linkage_sized(n + 3, lo, hi, w, 5, eligible=eligible)
    assert np.array_equal(padded[:n], labels) and np.all(padded[n:] == -1)


def test_cut_linkage_sized_errors(clip_lib):
    n, i, j, d = sized_data()
    lo, hi, w = kruskal(n, i, j, d)
    with pytest.raises(ValueError, match=r"no distance of the tree gives 101 groups of at least 2 rows; the counts that occur: 1, 2"):
        clip_lib.cut_linkage_sized(n, lo, hi, w, 101)
    with pytest.raises(ValueError):
        clip_lib.cut_linkage_sized(n, lo, hi, w[:-1], 3)
    with pytest.raises(ValueError):
        clip_lib.cut_linkage_sized(n, hi, lo, w, 3)
    with pytest.raises(ValueError, match="the counts that occur: none$"):             # no edge at all: the tree has no distance to cut at
        clip_lib.cut_linkage_sized(3, [], [], [], 3, min_size=1)


def test_option_parsing_and_texts(capsys):
    G = lambda argv: image_search._parse(argv, build=False, groups=True)
    V = lambda argv: image_search._parse(argv, build=False, levels=True)
    assert G(["-n", "4"])["core"] is None and V([])["core"] is None
    assert G(["-n", "4", "--core", "5", "--min", "3", "--extents"])["core"] == 5
    assert V(["--core", "0"])["core"] == 0 and V(["--core", "1024"])["core"] == 1024
    assert G(["-n", "4", "--core"]) is None and G(["-n", "4", "--core", "x"]) is None
    for bad in ("-1", "1025"):
        capsys.readouterr()
        assert V(["--core", bad]) is None and G(["-n", "2", "--core", bad]) is None
        assert capsys.readouterr().out.count("--core takes 0 ... 1024") == 2
    assert image_search._parse(["--core", "3", "q"], build=False) is None          # search has no --core
    doc = image_search.__doc__
    assert "[--min M] [--extents] [--core K]" in doc and "[-n ROWS] [--core K]" in doc and "Index.linkage_core" in doc
    assert "cut at radius %f, %d images left unfiled" in doc
    for cmd in ("groups", "levels"):
        with pytest.raises(SystemExit):
            image_search.main([cmd, "-h"])
        assert "--core K" in capsys.readouterr().out


def test_wrapper_refuses_before_the_library(clip_lib):
    class Unreachable(clip_lib.Index):
        def __init__(self):                    # no handle: every library call would need one
            pass

        def __len__(self):
            return 10

        def _live(self):
            raise AssertionError("the library was reached")

    ix = Unreachable()
    for k in (-1, 1025):
        with pytest.raises(ValueError, match="outside 0 ... 1024"):
            ix.linkage_core(k)
        with pytest.raises(ValueError, match="outside 0 ... 1024"):
            ix.linkage_core_device(k, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="NaN"):
        ix.linkage_core(3, float("nan"))
    with pytest.raises(ValueError):
        ix.linkage_core(3, allow=np.ones(9, dtype=bool))
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.linkage_core(3, 0.5, allow=[0, 9])
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.linkage_core_device(0, 1, 1, 1, 1)


def test_entry_points_are_declared_and_refuse_without_an_index(clip_lib, capfd):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    assert re.search(r"int64_t clip_amd_index_linkage_core\(struct clip_amd_index \* ix, int k, float link, const uint64_t \* allow, "
                     r"int64_t \* lo, int64_t \* hi,\s+float \* weights, float \* core\);", header)
    assert re.search(r"bool clip_amd_index_linkage_core_device\(struct clip_amd_index \* ix, int k, float link, const uint64_t \* d_allow, "
                     r"int64_t \* d_lo, int64_t \* d_hi,\s+float \* d_weights, float \* d_core, int64_t \* d_count\);", header)
    assert re.search(r"float clip_amd_bench_linkage_core\(int dtype, int64_t n, int dim, int k, int copies, int iters\);", header)
    for name in ("clip_amd_index_linkage_core", "clip_amd_index_linkage_core_device", "clip_amd_bench_linkage_core"):
        assert name in clip_lib.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert callable(clip_lib.Index.linkage_core) and callable(clip_lib.Index.linkage_core_device)
    assert callable(clip_lib.cut_linkage_sized) and callable(clip_lib.bench_linkage_core)
    L = clip_lib.lib()
    lo = np.full(4, -7, dtype=np.int64)
    hi = np.full(4, -7, dtype=np.int64)
    w = np.full(4, -7, dtype=np.float32)
    core = np.full(5, -7, dtype=np.float32)
    i64p, f32p = L.clip_amd_index_linkage_core.argtypes[4], L.clip_amd_index_linkage_core.argtypes[6]
    capfd.readouterr()
    for k in (0, 3, -1, 1025):
        assert L.clip_amd_index_linkage_core(None, k, 0.5, None, lo.ctypes.data_as(i64p), hi.ctypes.data_as(i64p), w.ctypes.data_as(f32p),
                                             core.ctypes.data_as(f32p)) == -1
        assert L.clip_amd_index_linkage_core_device(None, k, 0.5, None, lo.ctypes.data, hi.ctypes.data, w.ctypes.data, core.ctypes.data,
                                                    lo.ctypes.data) is False
    assert L.clip_amd_index_linkage_core(None, 3, float("nan"), None, None, None, None, None) == -1
    err = capfd.readouterr().err
    assert err.count("clip_amd_index_linkage_core: index is NULL") == 5 and err.count("clip_amd_index_linkage_core_device: index is NULL") == 4
    assert np.all(lo == -7) and np.all(hi == -7) and np.all(w == -7) and np.all(core == -7)
