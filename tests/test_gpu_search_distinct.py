"""GPU tier of distinct search on the exact index (clip_amd_index_search_distinct[_device], clip_amd_index_search_ids_distinct;
k_distinct.hip).  The expected values never come from the code under test: they are the definition (tests/distinct_common.py: walk)
applied to the index's own results: the pool L = Index.search(q, P, allow), the near relation from Index.search_ids of L's members among
L's members (the entry whose query id is lower than its row id), then the walk.  Distances are compared as bits, ids and counts for
equality."""
import ctypes as C

import numpy as np
import pytest

from distinct_common import collapse, expected, near_pairs, pair_distances, planted, same, walk
from index_subset_common import DTYPES, fp, ip, make_x, make_y, up

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
R = 0.05
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


def queries(dim, nq, rows, seed=0):
    """random directions, and every third one a stored row plus noise (so that its burst or chain leads the pool)"""
    rng = np.random.default_rng(31 * dim + nq + seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    for t in range(0, nq, 3):
        r = rows[int(rng.integers(len(rows)))]
        q[t] = r + 0.05 / np.sqrt(dim) * rng.standard_normal(dim).astype(np.float32)
    return q


def oracle(ix, q, k, radius, pool, allow=None, cache=None):
    return expected(ix, ix.search(q, pool, allow=allow), k, radius, cache)


def raw_distinct(clip_lib, ix, q, k, radius, pool, words=None, fill=-7):
    """(ok, distances, ids, counts) of one clip_amd_index_search_distinct call into outputs pre-filled with `fill`"""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, ix.dim)
    rows = max(len(q), 1)
    dist = np.full((rows, max(k, 1)), fill, dtype=np.float32)
    ids = np.full((rows, max(k, 1)), fill, dtype=np.int64)
    cnt = np.full((rows, max(k, 1)), fill, dtype=np.int32)
    ok = clip_lib.lib().clip_amd_index_search_distinct(ix.handle, fp(q), len(q), k, radius, pool, up(words) if words is not None else None, fp(dist),
                                                       ip(ids), cnt.ctypes.data_as(i32p))
    return ok, dist, ids, cnt


def untouched(dist, ids, cnt, fill=-7):
    return bool(np.all(dist == fill) and np.all(ids == fill) and np.all(cnt == fill))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_definition(clip, clip_lib, dtype, dim):
    rows, _ = planted(dim)
    for n in (1, 5, 170):
        ix = make_index(clip, clip_lib, rows[:n], dtype)
        q = queries(dim, 5, rows[:n])
        cache = {}
        for k, pool in ((1, 1), (1, 17), (5, 64), (5, 100), (100, 256), (1024, 1024)):
            got = ix.search_distinct(q, k, R, pool=pool)
            assert got[0].shape == (5, k) and got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int32
            assert same(got, oracle(ix, q, k, R, pool, cache=cache)), (n, k, pool)
        if n == 170:
            # the data set discriminates: with the whole index in the pool every query suppresses something, and the greedy walk is not
            # the collapse of connected components (a chain is one component, but its ends are not near each other)
            L = ix.search(q, 256)
            exp = expected(ix, L, 170, R, cache)
            assert same(ix.search_distinct(q, 170, R, pool=256), exp)
            for t in range(5):
                assert exp[2][t].sum() > 0, t
                near = near_pairs(ix, L[1][t][L[1][t] >= 0], R)
                assert walk(L[1][t], near, 170)[0] != collapse(L[1][t], near, 170), t
            # the automatic pool: min(1024, max(64, 8 k))
            for k in (1, 5, 9, 200):
                assert same(ix.search_distinct(q, k, R), oracle(ix, q, k, R, min(1024, max(64, 8 * k)), cache=cache)), k
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_seventy_queries(clip, clip_lib, dtype):
    dim = 36
    rows, _ = planted(dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    q = queries(dim, 70, rows, seed=1)                                    # the wider query tile of the scan
    assert same(ix.search_distinct(q, 10, R, pool=80), oracle(ix, q, 10, R, 80, cache={}))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_shorter_than_the_index(clip, clip_lib, dtype):
    dim = 36
    rows, _ = planted(dim)
    rng = np.random.default_rng(5)
    rows = np.concatenate([rows, rng.standard_normal((1330, dim)).astype(np.float32)])[rng.permutation(1500)]
    ix = make_index(clip, clip_lib, rows, dtype)
    q = queries(dim, 3, rows, seed=2)
    got = ix.search_distinct(q, 100, R, pool=1024)
    assert same(got, oracle(ix, q, 100, R, 1024))
    assert (got[1] >= 0).all()
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_radius_edges(clip, clip_lib, dtype, dim):
    rows, kind = planted(dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    q = queries(dim, 5, rows, seed=3)
    plain = ix.search(q, 20)
    got = ix.search_distinct(q, 20, -1.0, pool=64)                        # R < 0: search, bit for bit, counts 0
    assert same(got, (plain[0], plain[1], np.zeros((5, 20), dtype=np.int32)))
    got = ix.search_distinct(q, 3, 4.0, pool=100)                         # a very large R: the pool's first member, count = members - 1
    assert np.array_equal(got[1][:, 0], plain[1][:, 0]) and (got[1][:, 1:] == -1).all() and np.isinf(got[0][:, 1:]).all()
    assert np.array_equal(got[2], np.tile(np.array([99, 0, 0], dtype=np.int32), (5, 1)))
    assert same(got, oracle(ix, q, 3, 4.0, 100))
    # the <= rule at one pair: the query is a chain member a (rank 0, kept) and b its best-ranked chain mate.  R = the pair's f32 distance
    # from the oracle suppresses b; at the f32 value just below the pair is not near, and b is listed unless another kept member is near it.
    chain = np.flatnonzero(kind == 2)
    d = pair_distances(ix, chain)
    checked = 0
    for a in chain[:12]:
        L = ix.search(rows[a][None, :], 64)
        if L[1][0, 0] != a:
            continue
        mates = [int(b) for b in L[1][0, 1:] if b >= 0 and d.get((min(a, b), max(a, b)), 9.0) <= np.float32(R)]
        if not mates:
            continue
        b = mates[0]
        dab = np.float32(d[(min(a, b), max(a, b))])
        below = np.nextafter(dab, np.float32(-np.inf), dtype=np.float32)
        at = ix.search_distinct(rows[a][None, :], 64, float(dab), pool=64)
        under = ix.search_distinct(rows[a][None, :], 64, float(below), pool=64)
        assert same(at, oracle(ix, rows[a][None, :], 64, float(dab), 64)) and same(under, oracle(ix, rows[a][None, :], 64, float(below), 64))
        assert at[1][0, 0] == a and b not in at[1][0] and at[2][0, 0] >= 1
        near_below = near_pairs(ix, L[1][0][L[1][0] >= 0], float(below))
        assert (min(a, b), max(a, b)) not in near_below
        if not any((min(c, b), max(c, b)) in near_below for c in under[1][0] if c >= 0 and c != b):
            assert b in under[1][0]
            checked += 1
    assert checked >= 1
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("way", ["remove", "allow", "both"])
def test_removed_rows_and_allow(clip, clip_lib, dtype, way):
    dim = 36
    rows, kind = planted(dim)
    n = len(rows)
    plain = make_index(clip, clip_lib, rows, dtype)
    burst = np.flatnonzero(kind == 1)
    q = np.concatenate([rows[burst[:3]], queries(dim, 3, rows, seed=4)])
    first = plain.search_distinct(q, 10, R, pool=64)
    best = first[1][:3, 0]                                                # each burst query's best member, a suppressor
    assert (first[2][:3, 0] >= 1).all()
    elig = np.ones(n, dtype=bool)
    elig[best] = False
    elig[np.random.default_rng(9).permutation(n)[:30]] = False
    x, allow = make_x(clip_lib, clip, rows, dtype, elig, way)
    y, m = make_y(clip_lib, clip, rows, dtype, elig)
    got = x.search_distinct(q, 10, R, pool=64, allow=allow)
    assert same(got, oracle(x, q, 10, R, 64, allow=allow))
    ref = y.search_distinct(q, 10, R, pool=64)
    assert same(got, (ref[0], m[ref[1]], ref[2]))                         # the index of the eligible rows only, ids mapped
    near = near_pairs(plain, np.arange(n), R)
    for t in range(3):                                                    # the best member is gone and a mate it suppressed is listed
        mates = [b for b in range(n) if elig[b] and (min(b, best[t]), max(b, best[t])) in near]
        assert best[t] not in got[1][t] and (not mates or any(b in got[1][t] for b in mates))
    for ix in (plain, x, y):
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_ids_distinct(clip, clip_lib, dtype):
    dim = 36
    rows, _ = planted(dim)
    n = len(rows)
    ix = make_index(clip, clip_lib, rows, dtype)
    ids = np.array([3, 99, 3, 169, 0, 42], dtype=np.int64)
    for k, pool in ((5, 64), (20, 0), (170, 256)):
        got = ix.search_ids_distinct(ids, k, R, pool=pool, exclude_self=False)
        assert same(got, ix.search_distinct(rows[ids], k, R, pool=pool))
        got = ix.search_ids_distinct(ids, k, R, pool=pool)                # the own row: neither a hit nor a suppressor
        for t, i in enumerate(ids):
            allow = np.ones(n, dtype=bool)
            allow[i] = False
            one = ix.search_distinct(rows[i][None, :], k, R, pool=pool, allow=allow)
            assert same((got[0][t:t + 1], got[1][t:t + 1], got[2][t:t + 1]), one) and i not in got[1][t]
    allow = np.arange(n) % 3 != 0
    got = ix.search_ids_distinct(ids, 10, R, pool=64, allow=allow)
    L = ix.search_ids(ids, 64, exclude_self=True, allow=allow)
    assert same(got, expected(ix, L, 10, R))
    # a removed or out-of-range id: false, the outputs untouched
    assert ix.remove([42]) == 1
    L_ = clip_lib.lib()
    for bad in ([3, 42], [3, n], [-1]):
        a = np.array(bad, dtype=np.int64)
        dist = np.full((len(a), 5), -7, dtype=np.float32)
        out = np.full((len(a), 5), -7, dtype=np.int64)
        cnt = np.full((len(a), 5), -7, dtype=np.int32)
        assert L_.clip_amd_index_search_ids_distinct(ix.handle, ip(a), len(a), 5, R, 64, 1, None, fp(dist), ip(out), cnt.ctypes.data_as(i32p)) is False
        assert untouched(dist, out, cnt), bad
    with pytest.raises(RuntimeError):
        ix.search_ids_distinct([3, 42], 5, R)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_blocks_calls_and_device_form(clip, clip_lib, dtype):
    import torch
    dim, k, pool = 36, 10, 100
    rows, _ = planted(dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    q = queries(dim, 8, rows, seed=6)
    auto = ix.search_distinct(q, k, R, pool=pool)
    assert same(auto, oracle(ix, q, k, R, pool))
    L = clip_lib.lib()
    assert L.clip_amd_test_index_distinct_block(ix.handle, 3) == 3
    assert same(ix.search_distinct(q, k, R, pool=pool), auto)             # blocks of 3, 3 and 2 queries
    tq = torch.from_numpy(q).cuda()
    td = torch.empty((8, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((8, k), dtype=torch.int64, device="cuda")
    tc = torch.empty((8, k), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_distinct_device(tq.data_ptr(), 8, k, R, td.data_ptr(), ti.data_ptr(), tc.data_ptr(), pool=pool)      # blocked device form
    clip.synchronize()
    assert same((td.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()), auto)
    assert L.clip_amd_test_index_distinct_block(ix.handle, 0) == 0
    assert L.clip_amd_test_index_distinct_block(ix.handle, -1) == -1 and L.clip_amd_test_index_distinct_block(ix.handle, 4097) == -1
    ids_auto = ix.search_ids_distinct(np.arange(8), k, R, pool=pool)
    assert L.clip_amd_test_index_distinct_block(ix.handle, 3) == 3
    assert same(ix.search_ids_distinct(np.arange(8), k, R, pool=pool), ids_auto)
    assert L.clip_amd_test_index_distinct_block(ix.handle, 0) == 0
    parts = [ix.search_distinct(q[:5], k, R, pool=pool), ix.search_distinct(q[5:], k, R, pool=pool)]      # two calls
    assert same(tuple(np.concatenate([a, b]) for a, b in zip(*parts)), auto)
    allow = np.arange(len(rows)) % 4 != 1
    tw = torch.from_numpy(clip_lib.allow_words(allow, len(rows)).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ix.search_distinct_device(tq.data_ptr(), 8, k, R, td.data_ptr(), ti.data_ptr(), tc.data_ptr(), pool=pool, d_allow=tw.data_ptr())
    clip.synchronize()
    assert same((td.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()), ix.search_distinct(q, k, R, pool=pool, allow=allow))
    assert same(ix.search_distinct(q, k, R, pool=pool), auto)             # run to run
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_save_and_load(clip, clip_lib, dtype, tmp_path):
    dim = 36
    rows, _ = planted(dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    q = queries(dim, 4, rows, seed=7)
    before = ix.search_distinct(q, 20, R, pool=128)
    ix.save(str(tmp_path / "x.index"))
    ix.close()
    iy = clip_lib.Index.load(clip, str(tmp_path / "x.index"))
    assert same(iy.search_distinct(q, 20, R, pool=128), before)
    iy.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_duplicates_and_zero_vectors(clip, clip_lib, dtype):
    dim = 36
    rng = np.random.default_rng(11)
    v, w = rng.standard_normal(dim).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    zero = np.zeros(dim, dtype=np.float32)
    rows = np.stack([w, v, zero, v, w, v, zero, v, zero])                  # v four times (ids 1, 3, 5, 7), w twice, three zero vectors
    ix = make_index(clip, clip_lib, rows, dtype)
    q = np.stack([v, w])
    L = ix.search(q, 9)
    assert L[1][0, :4].tolist() == [1, 3, 5, 7]                           # ties in L: lower id first
    for radius in (-1.0, 0.0, 5e-3, 0.999, 1.0, 2.5):
        got = ix.search_distinct(q, 9, radius, pool=9)
        assert same(got, expected(ix, L, 9, radius)), radius
    got = ix.search_distinct(q, 9, 5e-3, pool=9)
    assert got[1][0, 0] == 1 and got[2][0, 0] == 3 and not {3, 5, 7} & set(got[1][0].tolist())
    # a zero vector is at distance exactly 1 from everything, the other zero vectors included: suppressed only at R >= 1
    zeros = {2, 6, 8}
    assert zeros <= set(ix.search_distinct(q, 9, 0.999, pool=9)[1][0].tolist())
    at_one = ix.search_distinct(q, 9, 1.0, pool=9)
    assert len(zeros & set(at_one[1][0].tolist())) <= 1
    ix.close()


def test_bad_arguments_leave_the_outputs_untouched(clip, clip_lib):
    dim = 36
    rows, _ = planted(dim)
    ix = make_index(clip, clip_lib, rows, "f16")
    empty = clip_lib.Index(clip, dim, "f16")
    q = queries(dim, 2, rows)
    ok, *outs = raw_distinct(clip_lib, ix, q, 5, R, 64)
    assert ok and not untouched(*outs)
    ok, *outs = raw_distinct(clip_lib, empty, q, 5, R, 64)                # an empty index
    assert ok is False and untouched(*outs)
    ok, *outs = raw_distinct(clip_lib, ix, q[:0], 5, R, 64)               # n_queries == 0
    assert ok is False and untouched(*outs)
    for k, radius, pool in ((0, R, 64), (1025, R, 0), (6, R, 5), (5, float("nan"), 64), (5, R, 1025), (5, R, -1)):
        ok, *outs = raw_distinct(clip_lib, ix, q, k, radius, pool)
        assert ok is False and untouched(*outs), (k, radius, pool)
    L = clip_lib.lib()
    dist = np.full((2, 5), -7, dtype=np.float32)
    out = np.full((2, 5), -7, dtype=np.int64)
    cnt = np.full((2, 5), -7, dtype=np.int32)
    assert L.clip_amd_index_search_distinct(ix.handle, fp(q), -1, 5, R, 64, None, fp(dist), ip(out), cnt.ctypes.data_as(i32p)) is False
    assert L.clip_amd_index_search_distinct(ix.handle, None, 2, 5, R, 64, None, fp(dist), ip(out), cnt.ctypes.data_as(i32p)) is False
    assert L.clip_amd_index_search_distinct(ix.handle, fp(q), 2, 5, R, 64, None, fp(dist), ip(out), None) is False
    assert untouched(dist, out, cnt)
    with pytest.raises(RuntimeError):
        empty.search_distinct(q, 5, R)
    for i in (ix, empty):
        i.close()


def test_bench_hook(clip_lib):
    assert clip_lib.bench_search_distinct("f16", 3000, 64, 4, 5, 64, 0.01, copies=4, iters=2) > 0
    assert clip_lib.bench_search_distinct("i8", 3000, 64, 4, 5, 0, 0.01, copies=4, iters=1) > 0
    assert clip_lib.bench_search_distinct("f16", 3000, 64, 4, 65, 64, 0.01, copies=4, iters=1) == -3.0      # k > pool
    assert clip_lib.bench_search_distinct("f16", 3000, 64, 4, 5, 64, 0.01, copies=0, iters=1) == -3.0
