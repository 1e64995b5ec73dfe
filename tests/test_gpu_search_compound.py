"""GPU tier of compound queries on the exact index (clip_amd_index_search_compound[_device]; k_compound.hip).  The expected values
never come from the code under test: they are the definition (tests/compound_common.py: compound) applied to the index's own single-term
distances, D = Index.range_search(term vectors, 4.0, allow) scattered into a matrix (those distances are search's bits) and, for stored-row
terms, Index.search_ids(exclude_self=False).  Distances are compared as bits, ids for equality."""
import ctypes as C

import numpy as np
import pytest

from compound_common import ALL, BEYOND, OVER, WITHIN, compound, flatten, make_queries, oracle, planted, query_arrays, query_matrix, same
from index_subset_common import DTYPES, fp, ip, up

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def make_index(clip, clip_lib, rows, dtype):
    ix = clip_lib.Index(clip, rows.shape[1], dtype)
    if len(rows):
        ix.add(rows)
    return ix


def raw_compound(clip_lib, ix, queries=None, k=5, exclude=1, words=None, arrays=None, nq=None, fill=-7):
    """(ok, distances, ids) of one clip_amd_index_search_compound call into outputs pre-filled with `fill`; arrays: the flat arrays
    (terms, term_ids, kinds, bounds, term_lims) instead of a list of queries"""
    terms, term_ids, kinds, bounds, lims = arrays if arrays is not None else flatten(queries, ix.dim)
    nq = len(lims) - 1 if nq is None else nq
    dist = np.full((max(nq, 1), max(k, 1)), fill, dtype=np.float32)
    ids = np.full((max(nq, 1), max(k, 1)), fill, dtype=np.int64)
    ok = clip_lib.lib().clip_amd_index_search_compound(ix.handle, fp(terms), ip(term_ids), kinds.ctypes.data_as(i32p), fp(bounds), ip(lims), nq, k, exclude,
                                                       up(words) if words is not None else None, fp(dist), ip(ids))
    return ok, dist, ids


def untouched(dist, ids, fill=-7):
    return bool(np.all(dist == fill) and np.all(ids == fill))


# (terms per query, queries, k): every value of each list of the issue at least once; 1 / 2, 3 / 4 and 5 / 8 terms take the three scans and
# the padding of each, 17 and 40 queries straddle the block of 16, k = 1024 exceeds every index here
CASES = [(1, 1, 1), (2, 17, 5), (3, 40, 100), (4, 17, 1024), (5, 1, 5), (8, 40, 5), (8, 17, 100)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_definition(clip, clip_lib, dtype, dim):
    for n in (1, 5, 170, 700):                                            # 700 rows at k = 5: three chunks, so the merge tree runs
        rows, dirs = planted(dim, n)
        ix = make_index(clip, clip_lib, rows, dtype)
        for n_terms, nq, k in CASES:
            queries = make_queries(dirs, nq, n_terms)
            got = ix.search_compound(queries, k)
            assert got[0].shape == (nq, k) and got[0].dtype == np.float32 and got[1].dtype == np.int64
            assert same(got, oracle(ix, queries, k)), (n, n_terms, nq, k)
            if k > n:
                assert (got[1][:, n:] == -1).all() and np.isinf(got[0][:, n:]).all()
        # queries of different lengths and all four kinds in one call
        queries = make_queries(dirs, 40, 0, lengths=[1, 2, 3, 5, 8, 4, 7])
        assert {len(q) for q in queries} == {1, 2, 3, 4, 5, 7, 8}
        assert {kind for q in queries for kind in query_arrays(q)[1]} == {ALL, WITHIN, BEYOND, OVER}
        assert same(ix.search_compound(queries, 5), oracle(ix, queries, 5)), n
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_the_data_discriminates(clip, clip_lib, dtype, dim):
    """On the oracle alone: all-of is neither a single term's ranking nor the mean vector's, and every filter kind bites."""
    rows, dirs = planted(dim, 170)
    ix = make_index(clip, clip_lib, rows, dtype)
    queries = make_queries(dirs, 16, 3) + make_queries(dirs, 16, 2, seed=1)
    all_of = over = beyond = within = 0
    for query in queries:
        whats, kinds, bounds = query_arrays(query)
        kinds, bounds = np.array(kinds), np.array(bounds)
        D = query_matrix(ix, query)
        top = set(compound(D, kinds, bounds, 5)[1].tolist())
        if (kinds == ALL).all():
            singles = [set(compound(D[t:t + 1], [ALL], [0], 5)[1].tolist()) for t in range(len(kinds))]
            mean = np.mean([w / np.linalg.norm(w) for w in whats], axis=0).astype(np.float32)
            of_mean = set(ix.search(mean[None, :], 5)[1][0].tolist())
            all_of += all(s != top for s in singles) and of_mean != top
        for kind in (OVER, BEYOND):
            if (kinds == kind).any():
                keep = kinds != kind
                unfiltered = set(compound(D[keep], kinds[keep], bounds[keep], 5)[1].tolist())
                removed = bool(unfiltered - set(compound(D, kinds, bounds, 170)[1].tolist()))
                over += removed and kind == OVER
                beyond += removed and kind == BEYOND
        if (kinds == WITHIN).any():
            within += (compound(D, kinds, bounds, 100)[1] >= 0).sum() < 100
    assert all_of >= 1 and over >= 1 and beyond >= 1 and within >= 1, (all_of, over, beyond, within)
    assert same(ix.search_compound(queries, 5), oracle(ix, queries, 5))
    assert same(ix.search_compound(queries, 100), oracle(ix, queries, 100))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_come_lower_id_first(clip, clip_lib, dtype):
    dim = 36
    rows, dirs = planted(dim, 85)
    ix = make_index(clip, clip_lib, np.concatenate([rows, rows]), dtype)   # every row twice: ids r and r + 85
    queries = make_queries(dirs, 8, 3)
    got = ix.search_compound(queries, 20)
    assert same(got, oracle(ix, queries, 20))
    for c in range(0, 8, 4):                                              # the queries without a filter: both copies, the lower id first
        assert np.array_equal(got[1][c, 0::2] + 85, got[1][c, 1::2])
        assert np.array_equal(got[0][c, 0::2].view(np.uint32), got[0][c, 1::2].view(np.uint32))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities(clip, clip_lib, dtype):
    dim = 36
    rows, dirs = planted(dim, 170)
    ix = make_index(clip, clip_lib, rows, dtype)
    allow = np.arange(170) % 3 != 1
    vecs = np.stack([q[0][0] for q in make_queries(dirs, 20, 1)])
    for a in (None, allow):
        assert same(ix.search_compound([[(v, "all")] for v in vecs], 10, allow=a), ix.search(vecs, 10, allow=a))      # a single all-term: search
    ids = [3, 99, 3, 169, 0]
    assert same(ix.search_compound([[(i, "all")] for i in ids], 10, allow=allow), ix.search_ids(ids, 10, exclude_self=True, allow=allow))
    assert same(ix.search_compound([[(i, "all")] for i in ids], 10, exclude_terms=False), ix.search_ids(ids, 10, exclude_self=False))
    # a result depends neither on the other queries of the call, nor on their order, nor on the padding, nor on the cut into blocks
    queries = make_queries(dirs, 19, 0, lengths=[2, 1, 3, 2])
    base = ix.search_compound(queries, 7)
    assert same(base, oracle(ix, queries, 7))
    for c in (0, 5, 18):
        alone = ix.search_compound([queries[c]], 7)
        assert same(alone, (base[0][c:c + 1], base[1][c:c + 1])), c
    order = np.random.default_rng(3).permutation(19)
    got = ix.search_compound([queries[c] for c in order], 7)
    assert same(got, (base[0][order], base[1][order]))
    longer = make_queries(dirs, 5, 8, seed=2)                             # the same queries next to 8-term ones: the widest scan
    got = ix.search_compound(longer + queries, 7)
    assert same((got[0][5:], got[1][5:]), base)
    L = clip_lib.lib()
    for block in (1, 16):
        assert L.clip_amd_test_index_compound_block(ix.handle, block) == block
        assert same(ix.search_compound(queries, 7), base), block
    assert L.clip_amd_test_index_compound_block(ix.handle, 0) == 0
    assert L.clip_amd_test_index_compound_block(ix.handle, -1) == -1 and L.clip_amd_test_index_compound_block(ix.handle, 1025) == -1
    assert same(ix.search_compound(queries, 7), base)                     # run to run
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_split_across_add_calls(clip, clip_lib, dtype):
    dim = 36
    rows, dirs = planted(dim, 170)
    one = make_index(clip, clip_lib, rows, dtype)
    parts = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 50), (50, 170)):
        parts.add(rows[lo:hi])
    queries = make_queries(dirs, 9, 4)
    assert same(one.search_compound(queries, 12), parts.search_compound(queries, 12))
    for ix in (one, parts):
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_path_compact_and_save(clip, clip_lib, dtype, tmp_path):
    dim = 36
    n = 700
    rows, dirs = planted(dim, n)
    ix = make_index(clip, clip_lib, rows, dtype)
    queries = make_queries(dirs, 18, 0, lengths=[3, 2, 5, 4])
    rng = np.random.default_rng(17)
    gone = rng.permutation(n)[:n // 10]
    assert ix.remove(gone) == len(gone)
    got = ix.search_compound(queries, 9)
    assert same(got, oracle(ix, queries, 9)) and not np.isin(got[1], gone).any()
    allow = (np.arange(n) // 16) % 2 == 0                                 # whole 16-row groups without an eligible row: the skip path
    allow[rng.permutation(n)[:100]] = False
    got = ix.search_compound(queries, 9, allow=allow)
    assert same(got, oracle(ix, queries, 9, allow=allow))
    assert allow[got[1][got[1] >= 0]].all() and not np.isin(got[1], gone).any()
    before = ix.search_compound(queries, 9)
    new_ids = np.append(ix.compact(), -1)                                  # (new_ids[-1] == -1 maps the empty id)
    after = ix.search_compound(queries, 9)
    assert same(after, oracle(ix, queries, 9))
    assert same(after, (before[0], new_ids[before[1]]))
    ix.save(str(tmp_path / "c.index"))
    ix.close()
    iy = clip_lib.Index.load(clip, str(tmp_path / "c.index"))
    assert same(iy.search_compound(queries, 9), after)
    iy.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_id_terms(clip, clip_lib, dtype):
    import torch
    dim = 36
    n = 170
    rows, dirs = planted(dim, n)
    ix = make_index(clip, clip_lib, rows, dtype)
    vq = make_queries(dirs, 6, 3)
    ids = [5, 160, 5, 33, 0, 169]
    by_id = [[(ids[c], "all")] + q[1:] for c, q in enumerate(vq)]
    by_vec = [[(rows[ids[c]], "all")] + q[1:] for c, q in enumerate(vq)]
    if dtype != "i8":                                                     # a vector term and the id of the row it was added as: the same bits
        assert same(ix.search_compound(by_id, 10, exclude_terms=False), ix.search_compound(by_vec, 10))
    for exclude in (True, False):
        got = ix.search_compound(by_id, 10, exclude_terms=exclude)
        assert same(got, oracle(ix, by_id, 10, exclude_terms=exclude)), exclude
        assert not exclude or not any(ids[c] in got[1][c] for c in range(6))
    # an id as a filter term: within 0.5 of stored row 33, ranked by a vector; the row itself is excluded or not
    filt = [[(vq[0][0][0], "all"), (33, "within", 0.5)], [(vq[1][0][0], "all"), (33, "over")]]
    for exclude in (True, False):
        assert same(ix.search_compound(filt, 10, exclude_terms=exclude), oracle(ix, filt, 10, exclude_terms=exclude))
    # a removed or out-of-range id: the host form returns false and leaves the outputs untouched, the device form gives an all-empty row
    assert ix.remove([42]) == 1
    good = ix.search_compound(by_id, 10)
    for bad in (42, n, 2 ** 40):
        broken = [list(q) for q in by_id]
        broken[2] = [broken[2][1], (bad, "over"), broken[2][2]]
        ok, dist, out = raw_compound(clip_lib, ix, broken, 10)
        assert ok is False and untouched(dist, out), bad
        with pytest.raises(RuntimeError):
            ix.search_compound(broken, 10)
        terms, term_ids, kinds, bounds, lims = flatten(broken, dim)
        tq = torch.from_numpy(terms).cuda()
        td = torch.full((6, 10), -7, dtype=torch.float32, device="cuda")
        ti = torch.full((6, 10), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.search_compound_device(tq.data_ptr(), term_ids, kinds, bounds, lims, 10, td.data_ptr(), ti.data_ptr())
        clip.synchronize()
        dist, out = td.cpu().numpy(), ti.cpu().numpy()
        assert (out[2] == -1).all() and np.isinf(dist[2]).all(), bad
        rest = [0, 1, 3, 4, 5]
        assert same((dist[rest], out[rest]), (good[0][rest], good[1][rest])), bad
    ix.close()


def test_refusals_leave_the_outputs_untouched(clip, clip_lib):
    dim = 36
    rows, dirs = planted(dim, 170)
    ix = make_index(clip, clip_lib, rows, "f16")
    empty = clip_lib.Index(clip, dim, "f16")
    queries = make_queries(dirs, 3, 3)
    ok, dist, ids = raw_compound(clip_lib, ix, queries, 5)
    assert ok and not untouched(dist, ids) and same((dist, ids), oracle(ix, queries, 5))
    for k in (0, 1025):
        ok, dist, ids = raw_compound(clip_lib, ix, queries, k)
        assert ok is False and untouched(dist, ids), k
    ok, dist, ids = raw_compound(clip_lib, empty, queries, 5)             # an empty index
    assert ok is False and untouched(dist, ids)
    terms, term_ids, kinds, bounds, lims = flatten(queries, dim)
    v = queries[0][0][0]
    nine = flatten([[(v, "all")] * 9], dim)
    no_all = flatten([[(v, "within", 0.5), (v, "over")]], dim)
    nan_bound = flatten([[(v, "all"), (v, "beyond", float("nan"))]], dim)
    kind7 = (terms, term_ids, np.where(np.arange(len(kinds)) == 4, 7, kinds).astype(np.int32), bounds, lims)
    negative = (terms, term_ids, np.where(np.arange(len(kinds)) == 4, -1, kinds).astype(np.int32), bounds, lims)
    decreasing = (terms, term_ids, kinds, bounds, np.array([0, 5, 3, 9], dtype=np.int64))
    not_zero = (terms, term_ids, kinds, bounds, np.array([1, 3, 6, 9], dtype=np.int64))
    no_terms = (terms, term_ids, kinds, bounds, np.array([0, 3, 3, 9], dtype=np.int64))
    for name, arrays in (("nine", nine), ("no_all", no_all), ("nan", nan_bound), ("kind7", kind7), ("negative", negative), ("decreasing", decreasing),
                         ("not_zero", not_zero), ("no_terms", no_terms)):
        ok, dist, ids = raw_compound(clip_lib, ix, k=5, arrays=arrays)
        assert ok is False and untouched(dist, ids), name
    for nq in (0, -1):
        ok, dist, ids = raw_compound(clip_lib, ix, k=5, arrays=(terms, term_ids, kinds, bounds, lims), nq=nq)
        assert ok is False and untouched(dist, ids), nq
    L = clip_lib.lib()
    dist = np.full((3, 5), -7, dtype=np.float32)
    out = np.full((3, 5), -7, dtype=np.int64)
    kp = kinds.ctypes.data_as(i32p)
    assert L.clip_amd_index_search_compound(ix.handle, None, ip(term_ids), kp, fp(bounds), ip(lims), 3, 5, 1, None, fp(dist), ip(out)) is False
    assert L.clip_amd_index_search_compound(ix.handle, fp(terms), None, None, fp(bounds), ip(lims), 3, 5, 1, None, fp(dist), ip(out)) is False
    assert L.clip_amd_index_search_compound(ix.handle, fp(terms), None, kp, fp(bounds), None, 3, 5, 1, None, fp(dist), ip(out)) is False
    assert L.clip_amd_index_search_compound(ix.handle, fp(terms), None, kp, fp(bounds), ip(lims), 3, 5, 1, None, None, ip(out)) is False
    assert L.clip_amd_index_search_compound(ix.handle, fp(terms), None, kp, None, ip(lims), 3, 5, 1, None, fp(dist), ip(out)) is False      # filters need bounds
    assert untouched(dist, out)
    a_bound = np.where(kinds == ALL, np.float32("nan"), bounds).astype(np.float32)      # the bound of an all-term is not read
    ok, dist, ids = raw_compound(clip_lib, ix, k=5, arrays=(terms, term_ids, kinds, a_bound, lims))
    assert ok and same((dist, ids), oracle(ix, queries, 5))
    with pytest.raises(RuntimeError):
        empty.search_compound(queries, 5)
    for i in (ix, empty):
        i.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form(clip, clip_lib, dtype):
    import torch
    dim, k = 36, 10
    n = 700
    rows, dirs = planted(dim, n)
    ix = make_index(clip, clip_lib, rows, dtype)
    queries = make_queries(dirs, 21, 0, lengths=[2, 8, 1, 4, 3])
    queries[4] = [(77, "all")] + queries[4][1:]
    host = ix.search_compound(queries, k)
    assert same(host, oracle(ix, queries, k))
    terms, term_ids, kinds, bounds, lims = flatten(queries, dim)
    tq = torch.from_numpy(terms).cuda()
    td = torch.empty((21, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((21, k), dtype=torch.int64, device="cuda")
    L = clip_lib.lib()
    for block in (0, 5):                                                  # one pass, and passes of 5, 5, 5, 5 and 1 queries
        assert L.clip_amd_test_index_compound_block(ix.handle, block) == block
        td.fill_(-7)
        ti.fill_(-7)
        torch.cuda.synchronize()
        ix.search_compound_device(tq.data_ptr(), term_ids, kinds, bounds, lims, k, td.data_ptr(), ti.data_ptr())
        clip.synchronize()
        assert same((td.cpu().numpy(), ti.cpu().numpy()), host), block
    assert L.clip_amd_test_index_compound_block(ix.handle, 0) == 0
    allow = np.arange(n) % 4 != 1
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ix.search_compound_device(tq.data_ptr(), term_ids, kinds, bounds, lims, k, td.data_ptr(), ti.data_ptr(), exclude_terms=False, d_allow=tw.data_ptr())
    clip.synchronize()
    assert same((td.cpu().numpy(), ti.cpu().numpy()), ix.search_compound(queries, k, allow=allow, exclude_terms=False))
    ix.close()


def test_bench_hook(clip_lib):
    assert clip_lib.bench_search_compound("f16", 3000, 64, 4, 2, 5, iters=2) > 0
    assert clip_lib.bench_search_compound("i8", 3000, 64, 17, 8, 100, iters=1) > 0
    assert clip_lib.bench_search_compound("f32", 3000, 64, 1, 3, 5, iters=1) > 0
    assert clip_lib.bench_search_compound("f16", 3000, 64, 4, 9, 5, iters=1) == -3.0        # more than 8 terms
    assert clip_lib.bench_search_compound("f16", 3000, 64, 0, 2, 5, iters=1) == -3.0
