"""GPU tier of the searches whose queries are stored rows (clip_amd_index_search_ids, clip_amd_index_knn_graph; k_search.hip's gather and
self-excluding scan, k_graph.hip's tiled kernel): a search by id against the search by the vector that was added, self exclusion against a
cleared allow bit, the k-NN graph on both routes against the search by id, all of it bit for bit; the graph against numpy; removal and
compaction; the device-pointer form; bad arguments."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "f32", "i8"]


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
    ix.add(rows)
    return ix


def same(a, b):
    """two (distances, ids) results are the same bits"""
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def set_route(clip_lib, ix, route):
    assert clip_lib.lib().clip_amd_test_index_knn_route(ix.handle, route) == route


def graph_on(clip_lib, ix, k, route):
    set_route(clip_lib, ix, route)
    try:
        return ix.knn_graph(k)
    finally:
        set_route(clip_lib, ix, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim, n", [(36, 300), (512, 1000)])
def test_by_id_equals_by_vector(clip, clip_lib, dtype, dim, n):
    rows = np.random.default_rng(dim + n).standard_normal((n, dim), dtype=np.float32)
    ix = make_index(clip, clip_lib, rows, dtype)
    ids = np.array([0, n - 1, n // 2, n // 2, 17])
    for k in (5, 1024):                                      # 1024 > n: the tail
        got = ix.search_ids(ids, k, exclude_self=False)
        assert same(got, ix.search(rows[ids], k))
        assert np.array_equal(got[1][:, 0], ids)             # (random rows: nothing else is near)
        assert np.all(got[1][:, n:] == -1) and np.all(np.isposinf(got[0][:, n:]))
    if n == 300:                                             # 1030 queries: two passes over the query chunks
        many = np.concatenate([np.arange(n), np.random.default_rng(1).integers(0, n, 730)])
        assert same(ix.search_ids(many, 3, exclude_self=False), ix.search(rows[many], 3))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim, n", [(36, 300), (512, 1000)])
def test_self_exclusion_equals_a_cleared_bit(clip, clip_lib, dtype, dim, n):
    rows = np.random.default_rng(2 * dim + n).standard_normal((n, dim), dtype=np.float32)
    mid = n // 2
    rows[3] = rows[17]                                       # exact copies of a query row at a lower and a higher id: ties on both sides of self
    rows[n - 5] = rows[17]
    rows[mid - 7] = rows[mid]
    rows[mid + 9] = rows[mid]
    rows[40] = 0.0                                           # two zero rows: at distance exactly 1 from everything
    rows[41] = 0.0
    ix = make_index(clip, clip_lib, rows, dtype)
    sub = np.random.default_rng(3).random(n) < 0.6           # an allowed set that ...
    for i in (0, 3, 17, 40, mid, mid + 9, n - 5, n - 1):
        but_i = np.ones(n, dtype=np.bool_)
        but_i[i] = False
        for k in (n, 1, 5):                                  # k = n: exactly one empty slot at the end
            got = ix.search_ids([i], k, True)
            assert same(got, ix.search(rows[i:i + 1], k, allow=but_i)), (i, k)
            assert i not in got[1]
            if k == n:
                assert got[1][0, n - 1] == -1 and got[1][0, n - 2] >= 0
        a = sub.copy()
        a[i] = False                                         # ... excludes the query row itself: the query need not be allowed
        assert same(ix.search_ids([i], 5, True, allow=a), ix.search(rows[i:i + 1], 5, allow=a)), i
        a[i] = True                                          # allowed or not, self exclusion wins
        assert same(ix.search_ids([i], 5, True, allow=a), ix.search(rows[i:i + 1], 5, allow=a & but_i)), i
    ix.close()


GRAPH_SHAPES = [(36, 1), (36, 2), (36, 127), (36, 128), (36, 129), (36, 300), (36, 1000), (512, 4099)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim, n", GRAPH_SHAPES)
def test_graph_equals_by_id_on_both_routes(clip, clip_lib, dtype, dim, n):
    """The tiled route splits the rows of a query tile across workgroups, at least 4 k and 256 rows each in whole tiles of 128, until there
    is one workgroup per compute unit: n = 1000 at k = 1 and 5 gives 4 chunks of 256 rows per query tile (a full merge tree of two levels),
    n = 4099 at k = 100 gives chunks of 640 rows, 7 of them (an odd count: a list without a partner at the first merge level)."""
    rows = np.random.default_rng(dim + 3 * n).standard_normal((n, dim), dtype=np.float32)
    if n >= 300:
        rows[n - 1] = rows[130]                              # a tie across tiles
    ix = make_index(clip, clip_lib, rows, dtype)
    for k in (1, 5, 100) + ((1024,) if n == 1000 else ()):
        want = ix.search_ids(np.arange(n), k, True)
        assert not np.any(want[1] == np.arange(n)[:, None])
        assert np.all((want[1][:, :min(k, n - 1)] >= 0)) and np.all(want[1][:, n - 1:] == -1)
        assert same(graph_on(clip_lib, ix, k, 1), want), ("scan route", k)
        assert same(graph_on(clip_lib, ix, k, 2), want), ("tiled route", k)
        assert same(ix.knn_graph(k), want), ("automatic route", k)
    ix.close()


def stored_values(index, tmp_path):
    """what the index stores, unpadded, from its own file"""
    p = str(tmp_path / "rows.index")
    index.save(p)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    return np.memmap(p, dtype={0: np.float32, 1: np.float16, 3: np.int8}[dt], mode="r", offset=28, shape=(n, dim))


def check(dist, ids, refd, k, dim):
    """distances within tol of the float64 reference; ids = the exact top-k except among entries within tol of the k-th; sorted, tie rule
    (the helper of tests/test_gpu_search.py)"""
    tol = dim * 2.0 ** -24 + 1e-6
    nq, n = refd.shape
    kk = min(k, n)
    assert dist.shape == (nq, k) and ids.shape == (nq, k)
    assert np.all(ids[:, kk:] == -1) and np.all(np.isinf(dist[:, kk:])) and np.all(dist[:, kk:] > 0)
    for i in range(nq):
        d, g = dist[i, :kk].astype(np.float64), ids[i, :kk]
        assert np.all((g >= 0) & (g < n)) and len(set(g.tolist())) == kk
        assert np.all(np.abs(d - refd[i, g]) <= tol), np.abs(d - refd[i, g]).max()
        assert np.all(np.diff(d) >= 0)
        same_d = np.diff(d) == 0
        assert np.all(np.diff(g)[same_d] > 0), "equal distances must come lower id first"
        top = np.argpartition(refd[i], kk - 1)[:kk] if kk < n else np.arange(n)
        kth = refd[i, top].max()
        want = set(top.tolist())
        for x in set(g.tolist()) ^ want:
            assert abs(refd[i, x] - kth) <= tol, (i, x, refd[i, x], kth)
        np.testing.assert_allclose(d, np.sort(refd[i, top]), atol=tol, rtol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_against_numpy(clip, clip_lib, tmp_path, dtype):
    """float64 over the stored values with the diagonal at +inf; i8: the cosine of the stored integer vectors (their dot is exact in
    float64), as tests/test_gpu_search_i8.py does"""
    n, dim, k = 1000, 512, 5
    rows = np.random.default_rng(11).standard_normal((n, dim), dtype=np.float32)
    ix = make_index(clip, clip_lib, rows, dtype)
    v = np.asarray(stored_values(ix, tmp_path), dtype=np.float64)
    if dtype == "i8":
        nrm = np.sqrt((v * v).sum(1))[:, None]
        v = np.where(nrm > 0, v / np.where(nrm > 0, nrm, 1), 0)
    refd = 1.0 - v @ v.T
    np.fill_diagonal(refd, np.inf)
    for route in (1, 2):
        dist, ids = graph_on(clip_lib, ix, k, route)
        check(dist, ids, refd, k, dim)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_removal_and_compaction(clip, clip_lib, dtype):
    n, dim = 1000, 36
    rows = np.random.default_rng(21).standard_normal((n, dim), dtype=np.float32)
    gone = np.concatenate([np.arange(256, 384), np.arange(512, 528),          # a whole aligned group of 128, one of 16
                           np.random.default_rng(22).choice(np.setdiff1d(np.arange(n), np.arange(256, 384)), 50, replace=False)])
    gone = np.unique(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    ix = make_index(clip, clip_lib, rows, dtype)
    assert ix.remove(gone) == gone.size
    fresh = make_index(clip, clip_lib, rows[keep], dtype)
    with pytest.raises(RuntimeError):
        ix.search_ids([int(gone[0])], 5)
    for k in (5, 100):
        fd, fi = fresh.knn_graph(k)
        for route in (1, 2):
            dist, ids = graph_on(clip_lib, ix, k, route)
            assert np.all(ids[gone] == -1) and np.all(np.isposinf(dist[gone]))
            assert not np.isin(ids, gone).any()
            assert np.array_equal(dist[keep].view(np.uint32), fd.view(np.uint32)), (k, route)
            assert np.array_equal(ids[keep], np.where(fi >= 0, keep[np.maximum(fi, 0)], -1)), (k, route)
            assert same((dist[keep], ids[keep]), ix.search_ids(keep, k, True))
    new_ids = ix.compact()
    assert np.array_equal(new_ids[keep], np.arange(keep.size)) and np.all(new_ids[gone] == -1)
    for route in (1, 2):
        assert same(graph_on(clip_lib, ix, 5, route), fresh.knn_graph(5))
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form(clip, clip_lib, dtype):
    import torch
    n, dim, k = 1000, 36, 7
    rows = np.random.default_rng(31).standard_normal((n, dim), dtype=np.float32)
    ix = make_index(clip, clip_lib, rows, dtype)
    ix.remove([500])
    ids = np.array([0, 999, 17, 17, 333, 501], dtype=np.int64)
    allow = np.random.default_rng(32).random(n) < 0.5
    words = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64)).cuda()

    def device(idv, exclude, d_allow):
        t_ids = torch.from_numpy(idv).cuda()
        td = torch.full((idv.size, k), -7.0, dtype=torch.float32, device="cuda")
        ti = torch.full((idv.size, k), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.search_ids_device(t_ids.data_ptr(), idv.size, k, td.data_ptr(), ti.data_ptr(), exclude_self=exclude, d_allow=d_allow)
        clip.synchronize()
        torch.cuda.synchronize()                             # the stream finished clean
        return td.cpu().numpy(), ti.cpu().numpy()

    for exclude in (True, False):
        assert same(device(ids, exclude, None), ix.search_ids(ids, k, exclude))
        assert same(device(ids, exclude, words.data_ptr()), ix.search_ids(ids, k, exclude, allow=allow))
    bad = np.array([0, n, 17, 500, -1, 2 ** 40, 333], dtype=np.int64)      # out of range, removed: all-empty rows, the others unchanged
    dist, out = device(bad, True, None)
    good = np.array([0, 2, 6])
    assert same((dist[good], out[good]), ix.search_ids(bad[good], k, True))
    for t in (1, 3, 4, 5):
        assert np.all(out[t] == -1) and np.all(np.isposinf(dist[t]))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments(clip, clip_lib, dtype):
    n, dim = 300, 36
    rows = np.random.default_rng(41).standard_normal((n, dim), dtype=np.float32)
    ix = make_index(clip, clip_lib, rows, dtype)
    ix.remove([123])
    want = ix.search_ids([5, 200], 4)
    L = clip_lib.lib()
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    dist = np.full((2, 1025), 123.5, dtype=np.float32)
    out = np.full((2, 1025), -99, dtype=np.int64)

    def call(idv, k, d=dist, o=out):
        a = np.asarray(idv, dtype=np.int64)
        return L.clip_amd_index_search_ids(ix.handle, a.ctypes.data_as(i64p), a.size, k, 1, None, d.ctypes.data_as(f32p) if d is not None else None,
                                           o.ctypes.data_as(i64p) if o is not None else None)

    for idv, k in (([5, 200], 0), ([5, 200], 1025), ([5, -1], 4), ([n, 5], 4), ([5, 123], 4)):
        assert not call(idv, k), (idv, k)
        with pytest.raises(RuntimeError):
            ix.search_ids(idv, k)
    assert not call([5, 200], 4, None, out) and not call([5, 200], 4, dist, None)
    assert not L.clip_amd_index_knn_graph(ix.handle, 0, dist.ctypes.data_as(f32p), out.ctypes.data_as(i64p))
    assert not L.clip_amd_index_knn_graph(ix.handle, 1025, dist.ctypes.data_as(f32p), out.ctypes.data_as(i64p))
    assert not L.clip_amd_index_knn_graph(ix.handle, 4, None, None)
    for k in (0, 1025):
        with pytest.raises(RuntimeError):
            ix.knn_graph(k)
    assert np.all(dist == 123.5) and np.all(out == -99), "a failed call wrote to the caller's arrays"
    assert call([], 4, None, None)                           # no ids: succeeds, launches nothing
    assert same(ix.search_ids([5, 200], 4), want)            # a valid call after the failures
    ix.close()
