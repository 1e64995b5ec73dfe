"""GPU tier of the search of one index with the rows of another (clip_amd_index_search_index: the gather + scan route and the CROSS
instantiations of k_graph.hip's tiled kernel) and of clip_amd_index_append: both routes against the search by the vectors that were added,
bit for bit, at the query-tile and chunk edges; the mask on the candidate side; ix is src; ids given; the result against float64 numpy;
bad arguments; append against add."""
import struct

import numpy as np
import pytest

from index_subset_common import DTYPES, WAYS, eligible_sets, fp, ip, make_x, make_y

pytestmark = pytest.mark.gpu

SRC_SIZES = [1, 127, 128, 129, 300]          # query-tile edges
IX_SIZES = [1, 5, 129, 1000]


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
    """two (distances, ids) results are the same bits"""
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def cross_on(clip_lib, ix, src, k, route, **kw):
    L = clip_lib.lib()
    assert L.clip_amd_test_index_cross_route(ix.handle, route) == route
    try:
        return ix.search_index(src, k, **kw)
    finally:
        assert L.clip_amd_test_index_cross_route(ix.handle, 0) == 0


def planted(dim, n_src, n_ix, seed=0):
    """(rows of src, rows of ix): random rows; ix holds copies of src's row 0 at a low id and at its last id (from 129 rows on that is
    another tile of 128: a tie across tiles) and two zero rows; src's row 1 is a zero row (distance exactly 1 to everything: every
    candidate ties)."""
    rng = np.random.default_rng(1000 * dim + 10 * n_src + n_ix + seed)
    a = rng.standard_normal((n_src, dim), dtype=np.float32)
    b = rng.standard_normal((n_ix, dim), dtype=np.float32)
    if n_src > 1:
        a[1] = 0.0
    if n_ix >= 5:
        b[1] = a[0]
        b[n_ix - 1] = a[0]
        b[2] = 0.0
        b[3] = 0.0
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [36, 512])
def test_both_routes_equal_search_by_vector(clip, clip_lib, dtype, dim):
    """every size(src) x size(ix): more queries than rows and fewer both occur (a kernel that clamps a tile's last queries with the
    candidate store's count reads the wrong rows there); k > size(ix): the tail"""
    for n_ix in IX_SIZES:
        for n_src in SRC_SIZES:
            a, b = planted(dim, n_src, n_ix)
            src, ix = make_index(clip, clip_lib, a, dtype), make_index(clip, clip_lib, b, dtype)
            for k in (1, 5, 100) + ((1024,) if n_ix == 1000 else ()):
                want = ix.search(a, k)
                assert np.all(want[1][:, n_ix:] == -1) and np.all(np.isposinf(want[0][:, n_ix:])) and np.all(want[1][:, :min(k, n_ix)] >= 0)
                if n_ix >= 5 and k >= 5:
                    assert want[1][0, :2].tolist() == [1, n_ix - 1] and want[0][0, 0] == want[0][0, 1]      # the copies: a tie, lower id first
                    if n_src > 1:
                        assert np.all(want[0][1, :5] == 1.0) and want[1][1, :5].tolist() == [0, 1, 2, 3, 4]  # the zero query
                assert same(cross_on(clip_lib, ix, src, k, 1), want), ("scan route", n_src, n_ix, k)
                assert same(cross_on(clip_lib, ix, src, k, 2), want), ("tiled route", n_src, n_ix, k)
                assert same(ix.search_index(src, k), want), ("automatic route", n_src, n_ix, k)
            src.close()
            ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_chunk_count(clip, clip_lib, dtype):
    """4099 rows at k = 100: the tiled route splits them into 9 chunks of 512 rows, the scan route into 11 of 384: odd counts, a list
    without a partner at the first level of the merge tree"""
    a, b = planted(512, 300, 4099)
    src, ix = make_index(clip, clip_lib, a, dtype), make_index(clip, clip_lib, b, dtype)
    want = ix.search(a, 100)
    assert want[1][0, :2].tolist() == [1, 4098]
    assert same(cross_on(clip_lib, ix, src, 100, 1), want)
    assert same(cross_on(clip_lib, ix, src, 100, 2), want)
    src.close()
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("way", WAYS)
def test_mask_on_the_candidate_side(clip, clip_lib, dtype, way):
    """X restricted to E (by removal, by allow, by both) returns what a fresh index Y of the eligible rows returns, ids mapped"""
    n, n_src, dim, k = 1000, 129, 36, 5
    a, b = planted(dim, n_src, n, seed=1)
    src = make_index(clip, clip_lib, a, dtype)
    for name, elig in eligible_sets(n).items():
        x, allow = make_x(clip_lib, clip, b, dtype, elig, way)
        y, m = make_y(clip_lib, clip, b, dtype, elig)
        yd, yi = y.search(a, k)
        want = (yd, m[yi])
        for route in (1, 2):
            assert same(cross_on(clip_lib, x, src, k, route, allow=allow), want), (name, route)
        assert same(cross_on(clip_lib, y, src, k, 2), (yd, yi)), name            # (Y itself, "none": an empty index)
        x.close()
        y.close()
    src.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_index_searched_with_itself(clip, clip_lib, dtype):
    n, dim = 300, 36
    a, _ = planted(dim, n, 1)
    a[n - 1] = a[0]
    ix = make_index(clip, clip_lib, a, dtype)
    allow = np.random.default_rng(5).random(n) < 0.5
    for k in (1, 5, 1024):
        want = ix.search_ids(np.arange(n), k, exclude_self=False)
        for route in (1, 2):
            assert same(cross_on(clip_lib, ix, ix, k, route), want), (k, route)
    want = ix.search_ids(np.arange(n), 5, exclude_self=False, allow=allow)
    for route in (1, 2):
        assert same(cross_on(clip_lib, ix, ix, 5, route, allow=allow), want), route
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_given(clip, clip_lib, dtype):
    a, b = planted(36, 300, 1000, seed=2)
    src, ix = make_index(clip, clip_lib, a, dtype), make_index(clip, clip_lib, b, dtype)
    ids = np.array([299, 0, 17, 17, 1, 128, 0])                          # unordered, duplicates
    many = np.concatenate([np.arange(300), np.random.default_rng(1).integers(0, 300, 730)])      # 1030: two passes over the query chunks
    allow = np.random.default_rng(6).random(1000) < 0.3
    for route in (0, 2):                                                   # (ids always take the scan route)
        assert same(cross_on(clip_lib, ix, src, 5, route, ids=ids), ix.search(a[ids], 5))
        assert same(cross_on(clip_lib, ix, src, 3, route, ids=many), ix.search(a[many], 3))
        assert same(cross_on(clip_lib, ix, src, 5, route, ids=ids, allow=allow), ix.search(a[ids], 5, allow=allow))
    got = ix.search_index(src, 5, ids=[])
    assert got[0].shape == (0, 5) and got[1].shape == (0, 5)
    src.close()
    ix.close()


def stored_values(index, path):
    """what the index stores, unpadded, from its own file"""
    index.save(path)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(path, "rb").read(28)[8:])
    return np.array(np.memmap(path, dtype={0: np.float32, 1: np.float16, 3: np.int8}[dt], mode="r", offset=28, shape=(n, dim)), dtype=np.float64)


def check(dist, ids, refd, k, dim):
    """distances within tol of the float64 reference; ids = the exact top-k except among entries within tol of the k-th; sorted, tie rule
    (the helper of tests/test_gpu_search.py, its tolerance unchanged)"""
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


def test_against_numpy(clip, clip_lib, tmp_path):
    """independent of `search`: float64 over the values the two indexes store (f32: the normalised rows, read back from their files)"""
    dim = 36
    a, b = planted(dim, 300, 1000, seed=3)
    src, ix = make_index(clip, clip_lib, a, "f32"), make_index(clip, clip_lib, b, "f32")
    refd = 1.0 - stored_values(src, str(tmp_path / "src.index")) @ stored_values(ix, str(tmp_path / "ix.index")).T
    for route in (1, 2):
        for k in (1, 5, 100):
            dist, ids = cross_on(clip_lib, ix, src, k, route)
            check(dist, ids, refd, k, dim)
    src.close()
    ix.close()


def test_bad_arguments(clip, clip_lib, fixture_cache, capfd):
    from oracle import fixtures
    L = clip_lib.lib()
    n, dim = 300, 36
    a, b = planted(dim, 40, n, seed=4)
    ix, src = make_index(clip, clip_lib, b, "f16"), make_index(clip, clip_lib, a, "f16")
    other_dim = make_index(clip, clip_lib, a[:, :32].copy(), "f16")
    other_dtype = make_index(clip, clip_lib, a, "i8")
    holed = make_index(clip, clip_lib, a, "f16")
    assert holed.remove([7]) == 1
    clip2 = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    foreign = make_index(clip2, clip_lib, a, "f16")
    empty = clip_lib.Index(clip, dim, "f16")
    dist = np.full((40, 1025), 123.5, dtype=np.float32)
    out = np.full((40, 1025), -99, dtype=np.int64)

    def call(s, idv, k, d=dist, o=out):
        idp, n_ids = None, 0
        if idv is not None:
            idv = np.asarray(list(idv) + [0], dtype=np.int64)[:len(idv)]      # (never a NULL pointer, also without ids)
            idp, n_ids = ip(idv), idv.size
        capfd.readouterr()
        ok = L.clip_amd_index_search_index(ix.handle, s.handle, idp, n_ids, k, None, fp(d) if d is not None else None, ip(o) if o is not None else None)
        return ok, capfd.readouterr().err

    cases = [(other_dim, None, 4, "32-dimensional"), (other_dtype, None, 4, "dtype 3"), (foreign, None, 4, "different contexts"),
             (holed, None, 4, "1 removed rows"), (src, [5, -1], 4, "id -1 (entry 1)"), (src, [40, 5], 4, "id 40 (entry 0)"),
             (src, None, 0, "k = 0"), (src, [1], 1025, "k = 1025")]
    for s, idv, k, message in cases:
        ok, err = call(s, idv, k)
        assert ok is False and message in err and "clip_amd_index_search_index:" in err, (message, err)
        with pytest.raises(RuntimeError):
            ix.search_index(s, k, ids=idv)
    assert "compact" in call(holed, None, 4)[1]
    assert call(src, None, 4, None, out)[0] is False and call(src, None, 4, dist, None)[0] is False
    assert np.all(dist == 123.5) and np.all(out == -99), "a failed call wrote to the caller's arrays"
    # append: the same requirements, plus ix != src; nothing changes
    for s, message in ((ix, "to itself"), (other_dtype, "dtype 3"), (other_dim, "32-dimensional"), (holed, "1 removed rows"), (foreign, "different contexts")):
        capfd.readouterr()
        assert L.clip_amd_index_append(ix.handle, s.handle, None) == -1
        assert message in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            ix.append(s)
        assert len(ix) == n and ix.live == n
    # no queries succeed and launch nothing: n_ids = 0, an empty src
    assert call(src, [], 4, None, None) == (True, "")
    assert call(empty, None, 4, None, None) == (True, "")
    assert np.all(dist == 123.5) and np.all(out == -99)
    assert same(ix.search_index(src, 4), ix.search(a, 4))                 # a valid call after the failures
    for x in (ix, src, other_dim, other_dtype, holed, foreign, empty):
        x.close()
    clip2.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_append_equals_add(clip, clip_lib, tmp_path, dtype):
    dim = 36
    ra, rb = planted(dim, 1100, 300, seed=5)      # 1100 rows: b lands behind the capacity a's store was allocated with
    a, b = make_index(clip, clip_lib, ra, dtype), make_index(clip, clip_lib, rb, dtype)
    both = make_index(clip, clip_lib, ra, dtype)
    both.add(rb)
    before = b.search(ra[:9], 7)
    new_ids = a.append(b)
    assert np.array_equal(new_ids, np.arange(len(rb)) + len(ra)) and len(a) == 1400 and a.live == 1400
    a.save(str(tmp_path / "a.index"))
    both.save(str(tmp_path / "both.index"))
    assert (tmp_path / "a.index").read_bytes() == (tmp_path / "both.index").read_bytes()
    q = np.concatenate([ra[:40], rb[:40], np.random.default_rng(9).standard_normal((20, dim), dtype=np.float32)])
    for k in (1, 5, 1024):
        assert same(a.search(q, k), both.search(q, k)), k
    assert same(a.knn_graph(5), both.knn_graph(5))
    assert len(b) == 300 and same(b.search(ra[:9], 7), before)           # src is unchanged
    # an empty index: appended, nothing happens; appended to, it becomes the other
    empty = clip_lib.Index(clip, dim, dtype)
    assert a.append(empty).shape == (0,) and clip_lib.lib().clip_amd_index_append(a.handle, empty.handle, None) == 0 and len(a) == 1400
    assert np.array_equal(empty.append(b), np.arange(300)) and same(empty.search(q, 5), b.search(q, 5))
    for x in (a, b, both, empty):
        x.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_append_into_an_index_with_removed_rows(clip, clip_lib, dtype):
    dim = 36
    ra, rb = planted(dim, 300, 200, seed=6)
    gone = np.array([0, 5, 128, 299])
    keep = np.setdiff1d(np.arange(300), gone)
    a, b = make_index(clip, clip_lib, ra, dtype), make_index(clip, clip_lib, rb, dtype)
    assert a.remove(gone) == 4
    a.append(b)
    assert len(a) == 500 and a.live == 496 and not a.live_mask()[gone].any() and a.live_mask().sum() == 496
    fresh = make_index(clip, clip_lib, np.concatenate([ra[keep], rb]), dtype)
    m = np.append(np.concatenate([keep, np.arange(300, 500)]), -1)
    q = np.concatenate([ra[:20], rb[:20]])
    for k in (5, 1024):
        fd, fi = fresh.search(q, k)
        assert same(a.search(q, k), (fd, m[fi])), k
    new_ids = a.compact()
    assert np.array_equal(new_ids[300:], np.arange(296, 496))
    assert same(a.search(q, 5), fresh.search(q, 5))
    for x in (a, b, fresh):
        x.close()
