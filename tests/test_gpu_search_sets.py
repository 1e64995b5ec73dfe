"""GPU tier of the query-set searches of the exact index (clip_amd_index_search_sets[_device], clip_amd_index_search_ids_sets,
Index.knn_graph_grouped; k_sets.hip and the own-group flag of k_group.hip).  The expected values never come from the code under test:
they are the full rankings of the existing entry points (Index.search with k = size, Index.search_ids with an allowed set) with the
definition applied here in numpy: per set every (query row, stored row) pair ordered by distance, stored row, query row; a pair is kept
when its key (the group of the stored row, or the row itself) has not appeared earlier; cut to k.  Distances are compared as bits."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES, fp, ip

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
BIG = 2 ** 31 - 1
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


def same(a, b):
    """two (distances, ids, qrows) results are the same bits"""
    return (a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], dtype=np.int64), np.asarray(b[2], dtype=np.int64)))


def fold(ranked, lims, k, groups):
    """the definition: ranked = (distances [nq, L], ids [nq, L]), every query row's eligible stored rows (-1 padded)"""
    dist, ids = ranked
    ns = len(lims) - 1
    out_d = np.full((ns, k), np.inf, dtype=np.float32)
    out_i = np.full((ns, k), -1, dtype=np.int64)
    out_q = np.full((ns, k), -1, dtype=np.int32)
    for s in range(ns):
        b, e = int(lims[s]), int(lims[s + 1])
        if e <= b:
            continue
        d, r = dist[b:e].ravel(), ids[b:e].ravel()
        q = np.repeat(np.arange(b, e), dist.shape[1])
        real = r >= 0
        d, r, q = d[real], r[real], q[real]
        order = np.lexsort((q, r, d))                       # distance, then stored row, then query row
        d, r, q = d[order], r[order], q[order]
        key = r if groups is None else np.asarray(groups, dtype=np.int64)[r]
        first = np.sort(np.unique(key, return_index=True)[1])[:k]
        out_d[s, :len(first)], out_i[s, :len(first)], out_q[s, :len(first)] = d[first], r[first], q[first]
    return out_d, out_i, out_q


def random_groups(rng, n, max_rows=8):
    """groups of 1 ... max_rows rows scattered over the ids (not contiguous), numbered sparsely up to 2^31 - 1 (which is used)"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, max_rows + 1)))
    labels = rng.permutation(np.unique(rng.integers(0, BIG, size=4 * len(sizes) + 8)))[:len(sizes)]
    labels[-1] = BIG
    g = np.repeat(labels, sizes)[:n]
    return rng.permutation(g).astype(np.int32)


def lims_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def data(dim, n, nq, seed=0):
    rng = np.random.default_rng(131 * dim + n + seed)
    return rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32), rng


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_definition(clip, clip_lib, dtype, dim):
    rng = np.random.default_rng(dim)
    # a leading, two adjacent and a trailing empty set; one set of 70 rows, more than the 64 queries of a scan workgroup
    sizes = [0, 3, 9] + rng.integers(0, 10, size=14).tolist() + [0, 0, 70] + rng.integers(1, 10, size=14).tolist() + [1, 0]
    lims = lims_of(sizes)
    nq = int(lims[-1])
    assert 180 <= nq <= 300
    for n in (1, 5, 129, 600):
        rows, q, rng = data(dim, n, nq)
        ix = make_index(clip, clip_lib, rows, dtype)
        full = ix.search(q, n)
        shapes = {"none": None, "distinct": np.arange(n, dtype=np.int32)[::-1].copy(), "one": np.full(n, 7, dtype=np.int32),
                  "random": random_groups(rng, n)}
        for k in (1, 5, 100, 1024):
            for name, g in shapes.items():
                got = ix.search_sets(q, lims, k, groups=g)
                assert got[2].dtype == np.int32 and got[0].shape == (len(sizes), k)
                assert same(got, fold(full, lims, k, g)), (n, k, name)
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_sets_of_one_row(clip, clip_lib, dtype, dim):
    n, nq = 600, 37
    rows, q, rng = data(dim, n, nq, seed=1)
    g = random_groups(rng, n)
    ix = make_index(clip, clip_lib, rows, dtype)
    lims = np.arange(nq + 1)
    for k in (1, 20, 1024):
        want_q = np.repeat(np.arange(nq)[:, None], k, axis=1)
        d, i = ix.search_grouped(q, k, g)
        assert same(ix.search_sets(q, lims, k, groups=g), (d, i, np.where(i >= 0, want_q, -1))), k
        d, i = ix.search(q, k)
        assert same(ix.search_sets(q, lims, k), (d, i, np.where(i >= 0, want_q, -1))), k
    ix.close()


@pytest.mark.parametrize("dtype,dim", [(t, 36) for t in DTYPES] + [("f16", 512)])
def test_pass_and_block_boundaries(clip, clip_lib, dtype, dim):
    """1100 query rows: more than the 1024 of one pass, so sets straddle the pass and the single set of 1100 is longer than one; with the
    block hook at 128 rows they straddle the query blocks of the host form as well"""
    n, nq = 600, 1100
    rows, q, rng = data(dim, n, nq, seed=2)
    g = random_groups(rng, n)
    sizes = []
    while sum(sizes) < nq:
        sizes.append(min(int(rng.integers(1, 71)), nq - sum(sizes)))
    lims = lims_of(sizes)
    cut = len(sizes) // 2
    ix = make_index(clip, clip_lib, rows, dtype)
    full = ix.search(q, n)
    for k in (5, 1024):
        for groups in (g, None):
            want, want_one = fold(full, lims, k, groups), fold(full, [0, nq], k, groups)
            for block in (0, 128):
                assert clip_lib.lib().clip_amd_test_index_sets_block(ix.handle, block) == block
                got = ix.search_sets(q, lims, k, groups=groups)
                assert same(got, want), (k, block)
                assert same(ix.search_sets(q, [0, nq], k, groups=groups), want_one), (k, block)
            # the same sets split across two calls at a set boundary
            a = ix.search_sets(q[:lims[cut]], lims[:cut + 1], k, groups=groups)
            b = ix.search_sets(q[lims[cut]:], lims[cut:] - lims[cut], k, groups=groups)
            joined = (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], np.where(b[2] >= 0, b[2] + lims[cut], -1)]))
            assert same(got, joined), k
    ix.close()


def grouped_layouts(rng):
    """name -> groups: 40 contiguous groups of 5 rows; 60 scattered groups of 1 ... 7 rows with sparse labels"""
    sizes = rng.integers(1, 8, size=60)
    labels = np.sort(rng.choice(BIG, size=60, replace=False))
    labels[-1] = BIG
    return {"contiguous5": np.repeat(np.arange(40, dtype=np.int32) + 3, 5), "scattered": rng.permutation(np.repeat(labels, sizes)).astype(np.int32)}


def ranked_without_own(ix, ids, groups, allow=None):
    """every stored row of `ids` against the rows outside its own group: search_ids with an allowed set, one call per group"""
    n = len(ix)
    dist = np.full((len(ids), n), np.inf, dtype=np.float32)
    out = np.full((len(ids), n), -1, dtype=np.int64)
    for grp in np.unique(groups[ids]):
        sel = np.flatnonzero(groups[ids] == grp)
        ok = groups != grp if allow is None else (groups != grp) & allow
        dist[sel], out[sel] = ix.search_ids(ids[sel], n, exclude_self=False, allow=ok)
    return dist, out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_stored_row_sets(clip, clip_lib, dtype, dim):
    rng = np.random.default_rng(5 + dim)
    for name, g in grouped_layouts(rng).items():
        n = len(g)
        rows = rng.standard_normal((n, dim), dtype=np.float32)
        ix = make_index(clip, clip_lib, rows, dtype)
        ids = rng.integers(0, n, size=150)                  # any order, duplicates
        sizes = []
        while sum(sizes) < len(ids):
            sizes.append(min(int(rng.integers(0, 12)), len(ids) - sum(sizes)))
        lims = lims_of(sizes + [0])
        for k in (3, 64):
            for groups in (g, None):
                got = ix.search_ids_sets(ids, lims, k, groups=groups, exclude_own=False)
                assert same(got, fold(ix.search_ids(ids, n, exclude_self=False), lims, k, groups)), (name, k)
            got = ix.search_ids_sets(ids, lims, k, groups=g, exclude_own=True)
            assert same(got, fold(ranked_without_own(ix, ids, g), lims, k, g)), (name, k)
            assert not (g[np.maximum(got[1], 0)] == g[ids[np.maximum(got[2], 0)]])[got[1] >= 0].any()
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_allow_and_removed_rows(clip, clip_lib, dtype, capfd):
    n, dim, nq = 600, 36, 60
    rows, q, rng = data(dim, n, nq, seed=3)
    g = random_groups(rng, n)
    ix = make_index(clip, clip_lib, rows, dtype)
    removed = rng.choice(n, n // 4, replace=False)
    assert ix.remove(removed) == len(removed)
    allow = rng.random(n) < 0.6
    lims = lims_of([7, 0, 20, 1, 32])
    for k in (5, 100):
        for al in (allow, None):
            assert same(ix.search_sets(q, lims, k, groups=g, allow=al), fold(ix.search(q, n, allow=al), lims, k, g)), k
    live = np.flatnonzero(ix.live_mask())
    ids = rng.choice(live, nq)
    got = ix.search_ids_sets(ids, lims, 5, groups=g, exclude_own=True, allow=allow)
    assert same(got, fold(ranked_without_own(ix, ids, g, allow), lims, 5, g))
    assert not np.isin(got[1], removed).any() and allow[got[1][got[1] >= 0]].all()
    # a removed or out-of-range id: false, the id named, the outputs untouched
    L = clip_lib.lib()
    for bad in (int(removed[0]), n, -1):
        ids2 = ids.astype(np.int64).copy()
        ids2[11] = bad
        dist = np.full((5, 5), -3.0, dtype=np.float32)
        out = np.full((5, 5), -3, dtype=np.int64)
        qr = np.full((5, 5), -3, dtype=np.int32)
        capfd.readouterr()
        assert L.clip_amd_index_search_ids_sets(ix.handle, ip(ids2), nq, ip(lims), 5, 5, 1, g.ctypes.data_as(i32p), None, fp(dist), ip(out),
                                                qr.ctypes.data_as(i32p)) is False
        assert ("id %d (entry 11)" % bad) in capfd.readouterr().err
        assert np.all(dist == -3.0) and np.all(out == -3) and np.all(qr == -3)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_ties(clip, clip_lib, dtype, dim):
    n = 300
    rows, q, rng = data(dim, n, 6, seed=4)
    rows[[10, 20, 200]] = q[0]          # the same stored vector three times
    q[3] = q[0]                         # ... and the same query row twice inside one set
    q[5] = q[0]                         # ... and once more in another set
    g = np.arange(n, dtype=np.int32)
    g[200] = g[20]
    ix = make_index(clip, clip_lib, rows, dtype)
    full = ix.search(q, n)
    lims = lims_of([4, 2])
    for k in (1, 3, 64):
        for groups in (None, g):
            assert same(ix.search_sets(q, lims, k, groups=groups), fold(full, lims, k, groups)), k
    d, i, qr = ix.search_sets(q, lims, 3)
    assert i[0].tolist() == [10, 20, 200] and qr[0].tolist() == [0, 0, 0]              # lower stored row first, then the lower query row
    assert i[1].tolist() == [10, 20, 200] and qr[1].tolist() == [5, 5, 5]
    d, i, qr = ix.search_sets(q, lims, 3, groups=g)
    assert i[0, :2].tolist() == [10, 20] and qr[0, :2].tolist() == [0, 0] and i[0, 2] not in (10, 20, 200)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_graph_grouped(clip, clip_lib, dtype):
    dim = 36
    rng = np.random.default_rng(9)
    for name, g in grouped_layouts(rng).items():
        n = len(g)
        rows = rng.standard_normal((n, dim), dtype=np.float32)
        ix = make_index(clip, clip_lib, rows, dtype)
        for removed in (None, np.concatenate([np.flatnonzero(g == g[0]), rng.choice(n, 9, replace=False)])):
            if removed is not None:
                ix.remove(removed)
            live = np.flatnonzero(ix.live_mask())
            order = live[np.argsort(g[live], kind="stable")]
            want_labels, counts = np.unique(g[order], return_counts=True)
            lims = lims_of(counts)
            ranked = ranked_without_own(ix, order, g)
            for k in (3, 64):
                labels, dist, ids, qids = ix.knn_graph_grouped(k, g)
                assert np.array_equal(labels, want_labels) and np.all(np.diff(labels) > 0)
                wd, wi, wq = fold(ranked, lims, k, g)
                assert same((dist, ids, qids), (wd, wi, np.where(wq >= 0, order[np.maximum(wq, 0)], -1))), (name, k)
                assert np.all(ids[:, len(labels) - 1:] == -1) and np.all(ids[:, :min(k, len(labels) - 1)] >= 0)      # every other group once
                assert np.array_equal(g[np.maximum(qids, 0)][ids >= 0], np.repeat(labels[:, None], k, axis=1)[ids >= 0])
        ix.close()


def test_bad_arguments(clip, clip_lib, capfd):
    n, dim = 40, 36
    rows, q, rng = data(dim, n, 6, seed=6)
    ix = make_index(clip, clip_lib, rows, "f16")
    L = clip_lib.lib()
    good = np.arange(n, dtype=np.int32)
    bad = good.copy()
    bad[17] = -1
    ids = np.arange(6, dtype=np.int64)

    def call(lims, k, groups, by_id=False, own=0, null_out=False):
        lims = np.asarray(lims, dtype=np.int64)
        ns = len(lims) - 1
        dist = np.full((ns, max(k, 1)), -3.0, dtype=np.float32)
        out = np.full((ns, max(k, 1)), -3, dtype=np.int64)
        qr = np.full((ns, max(k, 1)), -3, dtype=np.int32)
        gp = groups.ctypes.data_as(i32p) if groups is not None else None
        qp = None if null_out else qr.ctypes.data_as(i32p)
        if by_id:
            ok = L.clip_amd_index_search_ids_sets(ix.handle, ip(ids), 6, ip(lims), ns, k, own, gp, None, fp(dist), ip(out), qp)
        else:
            ok = L.clip_amd_index_search_sets(ix.handle, fp(q), 6, ip(lims), ns, k, gp, None, fp(dist), ip(out), qp)
        return ok, bool(np.all(dist == -3.0) and np.all(out == -3) and np.all(qr == -3))

    for by_id in (False, True):
        assert call([1, 3, 6], 5, good, by_id) == (False, True)            # does not start at 0
        assert call([0, 4, 3, 6], 5, good, by_id) == (False, True)         # decreases
        assert call([0, 3, 5], 5, good, by_id) == (False, True)            # does not end at the query rows
        assert call([0, 3, 6], 5, bad, by_id) == (False, True)             # a negative group
        assert call([0, 3, 6], 0, good, by_id) == (False, True)
        assert call([0, 3, 6], 1025, good, by_id) == (False, True)
        assert call([0, 3, 6], 5, good, by_id, null_out=True) == (False, True)
        assert call([0, 3, 6], 5, good, by_id)[0] is True
        assert call([0, 3, 6], 5, None, by_id)[0] is True
    capfd.readouterr()
    assert call([0, 3, 6], 5, None, True, own=1) == (False, True)          # exclude_own without groups
    assert "exclude_own needs groups" in capfd.readouterr().err
    assert call([0, 3, 6], 5, good, True, own=1)[0] is True
    for bad_lims in ([1, 6], [0, 4, 3, 6], [0, 5], [[0, 6]], [0.0, 6.0]):
        with pytest.raises(ValueError):
            ix.search_sets(q, bad_lims, 5)
    with pytest.raises(ValueError):
        ix.search_sets(q, [0, 6], 5, groups=bad)
    with pytest.raises(ValueError):
        ix.search_ids_sets(ids, [0, 6], 5)                                 # exclude_own is the default and needs groups
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form(clip, clip_lib, dtype):
    import torch
    n, dim, k = 600, 36, 20
    sizes = [0, 5, 70, 0, 1, 17, 0]
    lims = lims_of(sizes)
    nq = int(lims[-1])
    rows, q, rng = data(dim, n, nq, seed=7)
    g = random_groups(rng, n)
    allow = rng.random(n) < 0.5
    ix = make_index(clip, clip_lib, rows, dtype)
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    td = torch.empty((len(sizes), k), dtype=torch.float32, device="cuda")
    ti = torch.empty((len(sizes), k), dtype=torch.int64, device="cuda")
    tr = torch.empty((len(sizes), k), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for groups, tgp, al, twp in ((g, tg.data_ptr(), None, None), (g, tg.data_ptr(), allow, tw.data_ptr()), (None, None, allow, tw.data_ptr())):
        ix.search_sets_device(tq.data_ptr(), nq, lims, k, tgp, twp, td.data_ptr(), ti.data_ptr(), tr.data_ptr())
        clip.synchronize()
        assert same((td.cpu().numpy(), ti.cpu().numpy(), tr.cpu().numpy()), ix.search_sets(q, lims, k, groups=groups, allow=al))
    ix.close()
