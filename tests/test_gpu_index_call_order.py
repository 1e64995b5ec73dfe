"""GPU tier: a host form of the exact index gives the same bits whatever the index was asked before.  The host forms share device
workspaces (one results arena, the staging buffers, the block results of search_blocks), so what a call returns must not depend on the
calls before it, on their order, or on the sizes the workspaces had when the index was smaller.  The reference is the library itself
in a clean state: every form on a fresh index that has made no other call.  This is about history, not about values (the other index
tests hold the values), so every comparison is bit for bit.

300 rows of dim 36 (three 128-row tiles; 300 is no multiple of 64, 36 none of 16), 7 of them removed, k = 5; the test hooks cut every
blocked form into at least three blocks, and the k-NN and cross routes are forced to scan and to tiled once each."""
import numpy as np
import pytest

from index_subset_common import DTYPES, open_clip

pytestmark = pytest.mark.gpu

N, DIM, K, NQ = 300, 36, 5, 40
GONE = [0, 5, 63, 64, 129, 257, 298]
RADIUS = 0.05
SMALL_BLOCK = 13                                              # 40 queries: four blocks of the set, distinct and compound forms
VOTE_BLOCK = 128                                              # 300 rows or queries: three blocks of every vote form
ROUTES = {"scan": 1, "tiled": 2}


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    m = open_clip(clip_lib, fixture_cache)
    yield m
    m.close()


def make_data():
    rng = np.random.default_rng(20250)
    rows = rng.standard_normal((N + 500, DIM), dtype=np.float32)
    rows[150:170] = rows[10:30] + 0.02 * rng.standard_normal((20, DIM), dtype=np.float32)      # near-duplicates: pairs within RADIUS
    rows[700:720] = rows[40:60] + 0.02 * rng.standard_normal((20, DIM), dtype=np.float32)
    rows[7] = 0.0
    d = {"rows": rows, "q": rng.standard_normal((NQ, DIM), dtype=np.float32), "big_q": rng.standard_normal((N, DIM), dtype=np.float32)}
    d["q"][:5] = rows[10:15]
    live = np.setdiff1d(np.arange(N), GONE)
    d["ids"] = rng.choice(live, NQ).astype(np.int64)
    d["big_ids"] = rng.choice(live, N).astype(np.int64)
    d["lims"] = np.array([0, 1, 1, 9, 30, 31, NQ], dtype=np.int64)      # an empty set, and sets that straddle blocks of 13
    d["groups"] = (np.arange(N + 500) // 3).astype(np.int32)
    d["labels"] = (np.arange(N + 500) % 7).astype(np.int64)
    d["labels"][::11] = -1
    d["extent_labels"] = (np.arange(N + 500) // 10).astype(np.int64)
    d["compound"] = [[(d["q"][i], "all"), (int(d["ids"][i]), "all"), (d["q"][(i + 1) % NQ], "beyond", 0.1)] for i in range(NQ)]
    return d


DATA = make_data()


def make_index(clip_lib, clip, dtype, route, n=N):
    ix = clip_lib.Index(clip, DIM, dtype)
    ix.add(DATA["rows"][:n])
    assert ix.remove(GONE) == len(GONE)
    set_hooks(clip_lib, ix, route)
    return ix


def set_hooks(clip_lib, ix, route):
    L = clip_lib.lib()
    assert L.clip_amd_test_index_sets_block(ix.handle, SMALL_BLOCK) == SMALL_BLOCK
    assert L.clip_amd_test_index_distinct_block(ix.handle, SMALL_BLOCK) == SMALL_BLOCK
    assert L.clip_amd_test_index_compound_block(ix.handle, SMALL_BLOCK) == SMALL_BLOCK
    assert ix.vote_block(VOTE_BLOCK) == VOTE_BLOCK
    assert L.clip_amd_test_index_knn_route(ix.handle, route) == route
    assert L.clip_amd_test_index_cross_route(ix.handle, route) == route


def forms(src):
    """name -> call(ix): every host form, on the first len(ix) rows' worth of the shared data"""
    D = DATA
    return {
        "search": lambda ix: ix.search(D["q"], K),
        "search_ids": lambda ix: ix.search_ids(D["ids"], K),
        "search_sets": lambda ix: ix.search_sets(D["q"], D["lims"], K, groups=D["groups"][:len(ix)]),
        "search_ids_sets": lambda ix: ix.search_ids_sets(D["ids"], D["lims"], K, groups=D["groups"][:len(ix)], exclude_own=True),
        "search_distinct": lambda ix: ix.search_distinct(D["q"], K, RADIUS),
        "search_compound": lambda ix: ix.search_compound(D["compound"], K),
        "range_search": lambda ix: ix.range_search(D["q"], 0.8),
        "pairs": lambda ix: ix.pairs(RADIUS),
        "components": lambda ix: ix.components(RADIUS),
        "modes": lambda ix: ix.modes(RADIUS, link=0.6),
        "linkage": lambda ix: ix.linkage(),
        "linkage_core": lambda ix: ix.linkage_core(K),
        "extents": lambda ix: ix.extents(D["extent_labels"][:len(ix)]),
        "spread": lambda ix: ix.spread(20),
        "vote": lambda ix: ix.vote(D["big_q"], K, D["labels"][:len(ix)], m=3),
        "vote_ids": lambda ix: ix.vote_ids(D["big_ids"], K, D["labels"][:len(ix)], m=3),
        "vote_graph": lambda ix: ix.vote_graph(K, D["labels"][:len(ix)], m=3),
        "knn_graph": lambda ix: ix.knn_graph(K),
        "search_index": lambda ix: ix.search_index(src, K),
        "search_index_ids": lambda ix: ix.search_index(src, K, ids=D["big_ids"]),
    }


def flat(result):
    """a form's result as a list of arrays (a scalar becomes an array of one)"""
    return [np.asarray(r) for r in (result if isinstance(result, tuple) else (result,))]


def same(got, want):
    got, want = flat(got), flat(want)
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))


@pytest.fixture(scope="module")
def sources(clip, clip_lib):
    """per dtype the index whose rows search_index asks with: the 300 rows, none removed"""
    made = {}
    for dtype in DTYPES:
        made[dtype] = clip_lib.Index(clip, DIM, dtype)
        made[dtype].add(DATA["rows"][:N])
    yield made
    for ix in made.values():
        ix.close()


@pytest.fixture(scope="module")
def references(clip, clip_lib, sources):
    """(dtype, route) -> name -> the form's result on a fresh index that has made no other call; computed once and left unchanged"""
    refs = {}
    for dtype in DTYPES:
        for route in ROUTES.values():
            out = {}
            for name, call in forms(sources[dtype]).items():
                ix = make_index(clip_lib, clip, dtype, route)
                out[name] = call(ix)
                ix.close()
            refs[dtype, route] = out
    return refs


def test_the_cases_do_work(references):
    """the inputs reach what they are meant to: hits, pairs, groups, suppressed copies, edges and votes, on every dtype and route"""
    for ref in references.values():
        assert ref["range_search"][0][-1] > NQ and len(ref["pairs"][0]) >= 15
        assert np.sum(ref["components"][0] != np.arange(N)) >= 15 + len(GONE) and np.all(ref["components"][0][GONE] == -1)
        assert ref["search_distinct"][2].sum() > 0 and np.all(ref["search_sets"][1][1] == -1) and np.all(ref["search_sets"][1][3] >= 0)
        assert len(ref["linkage"][0]) == N - len(GONE) - 1 and len(ref["linkage_core"][0]) == N - len(GONE) - 1
        assert len(ref["spread"][0]) == 20 and np.all(ref["vote_graph"][1][1:5, 0] > 0) and np.all(ref["vote_graph"][0][GONE] == -1)
        assert np.all(ref["knn_graph"][1][GONE] == -1) and np.all(ref["search_index"][1] >= 0) and np.all(ref["search_compound"][1][:, 0] >= 0)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_form_in_order_and_reversed(clip, clip_lib, sources, references, dtype, route):
    ref = references[dtype, ROUTES[route]]
    calls = forms(sources[dtype])
    ix = make_index(clip_lib, clip, dtype, ROUTES[route])
    for order in (list(calls), list(calls)[::-1]):
        for name in order:
            assert same(calls[name](ix), ref[name]), (name, "reversed" if order[0] != "search" else "in order")
    ix.close()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_growth_between_calls(clip, clip_lib, sources, references, dtype, route):
    """components at 300 rows, 500 rows added, then extents, vote_graph and components: each as on a fresh index of the 800 rows"""
    calls = forms(sources[dtype])
    ix = make_index(clip_lib, clip, dtype, ROUTES[route])
    assert same(calls["components"](ix), references[dtype, ROUTES[route]]["components"])
    ix.add(DATA["rows"][N:])
    for name in ("extents", "vote_graph", "components"):
        fresh = make_index(clip_lib, clip, dtype, ROUTES[route], n=N + 500)
        want = calls[name](fresh)
        fresh.close()
        assert len(flat(want)[0]) == N + 500
        assert same(calls[name](ix), want), name
    ix.close()
