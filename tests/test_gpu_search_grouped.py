"""GPU tier of the grouped search of the exact index (clip_amd_index_search_grouped[_device], k_group.hip): each group at most once in a
result, represented by its best row.  The expected result is the definition applied to the project's own search: the full ranked list
(search with k = size, or k = 1024 where that provably holds enough groups) with the later rows of a group that was seen before dropped,
cut to k and padded with -1 / +inf; compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES, fp, ip

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
BIG = 2 ** 31 - 1


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


def dedup(ranked, groups, k):
    """the definition: of a ranked (distances, ids) list per query keep the rows whose group has not appeared earlier, cut to k, pad"""
    dist, ids = ranked
    out_d = np.full((len(ids), k), np.inf, dtype=np.float32)
    out_i = np.full((len(ids), k), -1, dtype=np.int64)
    for q in range(len(ids)):
        seen, n = set(), 0
        for d, i in zip(dist[q], ids[q]):
            if i < 0 or n == k:
                break
            g = int(groups[i])
            if g in seen:
                continue
            seen.add(g)
            out_d[q, n], out_i[q, n] = d, i
            n += 1
    return out_d, out_i


def random_groups(rng, n, max_rows=8):
    """groups of 1 ... max_rows rows scattered over the ids (not contiguous), numbered sparsely up to 2^31 - 1 (which is used)"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, max_rows + 1)))
    labels = rng.permutation(np.unique(rng.integers(0, BIG, size=4 * len(sizes) + 8)))[:len(sizes)]
    labels[-1] = BIG
    g = np.repeat(labels, sizes)[:n]
    return rng.permutation(g).astype(np.int32)


def rows_and_queries(dim, n, nq, seed=0):
    rng = np.random.default_rng(77 * dim + n + seed)
    return rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32), rng


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_sizes_and_group_shapes(clip, clip_lib, dtype, dim):
    for n in (1, 5, 129, 600, 1000):
        rows, q, rng = rows_and_queries(dim, n, 5)
        ix = make_index(clip, clip_lib, rows, dtype)
        full = ix.search(q, n)
        shapes = {"distinct": np.arange(n, dtype=np.int32)[::-1].copy(), "one": np.full(n, 7, dtype=np.int32), "random": random_groups(rng, n)}
        for k in (1, 5, 100, 1024):
            for name, g in shapes.items():
                got = ix.search_grouped(q, k, g)
                assert same(got, dedup(full, g, k)), (n, k, name)
                if name == "distinct":
                    assert same(got, ix.search(q, k)), (n, k)
                if name == "one":
                    assert np.all(got[1][:, 0] == full[1][:, 0]) and np.all(got[1][:, 1:] == -1) and np.all(np.isposinf(got[0][:, 1:]))
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_flooding_group(clip, clip_lib, dtype, dim):
    """size 1000, k 128: chunks of 512 rows and a candidate capacity of 384, so the selection runs in the middle of the scan, on buffers
    that hold almost nothing but the flooding group"""
    n, k = 1000, 128
    rows, q, rng = rows_and_queries(dim, n, 3, seed=1)
    rows[100:800] = q[0] + 0.01 * rng.standard_normal((700, dim), dtype=np.float32)
    g = np.arange(n, dtype=np.int32) + 5000
    g[100:800] = 3
    ix = make_index(clip, clip_lib, rows, dtype)
    got = ix.search_grouped(q, k, g)
    assert same(got, dedup(ix.search(q, n), g, k))
    assert 100 <= got[1][0, 0] < 800 and np.all(got[1][0] >= 0)                     # the group once, at the head, 127 others behind it
    assert np.all((got[1][0, 1:] < 100) | (got[1][0, 1:] >= 800))
    assert all(len(set(g[r].tolist())) == k for r in got[1])
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_ties(clip, clip_lib, dtype, dim):
    n = 600
    rows, q, rng = rows_and_queries(dim, n, 2, seed=2)
    q[1] = rows[0]
    rows[[10, 20]] = q[0]              # the same vector in two groups
    rows[[30, 40]] = q[0] * 2.0        # ... and twice in one group (same direction: the same stored row)
    rows[[255, 256]] = q[0]            # copies on both sides of a chunk edge (256-row chunks at k <= 64)
    rows[300:320] = 0.0                # zero rows: distance exactly 1, all tie
    g = np.arange(n, dtype=np.int32)
    g[40] = g[30]
    g[256] = g[255]
    g[300:320] = np.repeat(np.arange(900, 910, dtype=np.int32), 2)
    ix = make_index(clip, clip_lib, rows, dtype)
    full = ix.search(q, n)
    for k in (1, 3, 5, 64, 100):
        got = ix.search_grouped(q, k, g)
        assert same(got, dedup(full, g, k)), k
    got = ix.search_grouped(q, 64, g)
    assert got[1][0, :4].tolist() == [10, 20, 30, 255]                              # lower id first; a group's lower id represents it
    assert len(np.unique(got[0][0, :4].view(np.uint32))) == 1
    got = ix.search_grouped(q, n, g)
    zeros = got[1][0][got[0][0] == 1.0]
    assert zeros.tolist() == list(range(300, 320, 2))
    # the two copies across the chunk edge in different groups: both, lower id first
    g2 = g.copy()
    g2[256] = 256
    got = ix.search_grouped(q, 64, g2)
    assert same(got, dedup(full, g2, 64)) and got[1][0, :5].tolist() == [10, 20, 30, 255, 256]
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_many_chunks_odd_merge_tree(clip, clip_lib, dtype, dim):
    n = 5000
    rows, q, rng = rows_and_queries(dim, n, 4, seed=3)
    g = random_groups(rng, n, 8)
    assert np.bincount(np.unique(g, return_inverse=True)[1]).max() <= 8
    ix = make_index(clip, clip_lib, rows, dtype)
    ranked = ix.search(q, 1024)
    for k in (100, 128):
        assert k * 8 <= 1024           # the first k * 8 rows of L hold at least k groups of at most 8 rows: search(1024) is enough
        assert same(ix.search_grouped(q, k, g), dedup(ranked, g, k)), k
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_removed_rows_and_allow(clip, clip_lib, dtype, dim):
    n = 1000
    rows, q, rng = rows_and_queries(dim, n, 4, seed=4)
    g = random_groups(rng, n, 8)
    g[[50, 51, 52]] = 11               # a group without an eligible row
    g[[60, 700]] = 12                  # a group whose best row is removed
    rows[60] = q[0]
    rows[700] = q[0] + 0.05 * rng.standard_normal(dim, dtype=np.float32)
    ix = make_index(clip, clip_lib, rows, dtype)
    removed = np.unique(np.concatenate([rng.choice(n, n // 3, replace=False), [50, 60]]))
    removed = removed[removed != 700]
    assert ix.remove(removed) == len(removed)
    allow = rng.random(n) < 0.7
    allow[[51, 52]] = False
    allow[700] = True
    for k in (5, 100, 1024):
        got = ix.search_grouped(q, k, g, allow=allow)
        assert same(got, dedup(ix.search(q, n, allow=allow), g, k)), k
        assert not np.isin(got[1], [50, 51, 52]).any()
    assert got[1][0, 0] == 700
    no_allow = ix.search_grouped(q, 100, g)
    assert same(no_allow, dedup(ix.search(q, n), g, 100))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_query_splitting_runs_and_device_form(clip, clip_lib, dtype, dim):
    import torch
    n, k, nq = 1000, 20, 37
    rows, q, rng = rows_and_queries(dim, n, nq, seed=5)
    g = random_groups(rng, n, 8)
    ix = make_index(clip, clip_lib, rows, dtype)
    one = ix.search_grouped(q, k, g)
    assert same(one, ix.search_grouped(q, k, g))
    a, b = ix.search_grouped(q[:1], k, g), ix.search_grouped(q[1:], k, g)
    assert same(one, (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])))
    allow = rng.random(n) < 0.5
    tq, tg = torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda()
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_grouped_device(tq.data_ptr(), nq, k, tg.data_ptr(), None, td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert same((td.cpu().numpy(), ti.cpu().numpy()), one)
    ix.search_grouped_device(tq.data_ptr(), nq, k, tg.data_ptr(), tw.data_ptr(), td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert same((td.cpu().numpy(), ti.cpu().numpy()), ix.search_grouped(q, k, g, allow=allow))
    ix.close()


def full_ranking(search, n, allow):
    """every eligible row of each query in the order of `better`, from two searches over complementary halves of the ids (k = 515 and one
    chunk each: no selection runs before the end of the scan), merged here by (distance, id)"""
    lo = np.arange(n) < n // 2
    a, b = search(n // 2, lo & allow), search(n - n // 2, ~lo & allow)
    d, i = np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1)
    key = np.where(i < 0, np.iinfo(np.int64).max, i)
    order = np.stack([np.lexsort((key[r], d[r])) for r in range(len(d))])
    return np.take_along_axis(d, order, axis=1), np.take_along_axis(i, order, axis=1)


def without(ranked, drop):
    """a ranked list per query with the entries where drop[query, slot] holds taken out, padded"""
    dist, ids = ranked
    out_d, out_i = np.full_like(dist, np.inf), np.full_like(ids, -1)
    for r in range(len(ids)):
        keep = ~drop[r] & (ids[r] >= 0)
        out_d[r, :keep.sum()], out_i[r, :keep.sum()] = dist[r][keep], ids[r][keep]
    return out_d, out_i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_selection_in_the_middle_of_the_scan(clip, clip_lib, dtype, dim):
    """The four selections of the scan kernels where they shrink a buffer before the chunk ends.  k = 100: 356 candidate slots and
    chunks of 448 rows, so with the threshold still +inf every query's buffer is shrunk after the fifth iteration of 64 rows whatever
    the data; n = 1030 is three chunks (the last one short, an odd merge tree); 1, 17 and 64 queries take the kernels of 1, 2 and 4 query
    tiles.  Plain, self-excluding (search_ids), grouped and own-group (search_ids_sets over sets of one row), without a mask and with one
    that clears an aligned group of 16 rows (not read at all) and a single row.  Groups of 8 consecutive rows leave fewer than k groups
    in a chunk, so the grouped threshold stays +inf after a shrink; with every row its own group the grouped results must be the plain
    ones bit for bit.  Expected: the definitions above over full_ranking."""
    n, k = 1030, 100
    rows, _, rng = rows_and_queries(dim, n, 1, seed=7)
    ix = make_index(clip, clip_lib, rows, dtype)
    g8, g1 = (np.arange(n) // 8).astype(np.int32), np.arange(n, dtype=np.int32)
    masked = np.ones(n, dtype=bool)
    masked[512:528] = False
    masked[77] = False
    for nq in (1, 17, 64):
        q = rng.standard_normal((nq, dim), dtype=np.float32)
        ids = rng.choice(n, nq, replace=False).astype(np.int64)
        ids[0] = 77                                               # a query row that the mask clears
        lims, qrow = np.arange(nq + 1), np.arange(nq)[:, None]
        for allow in (None, masked):
            al = np.ones(n, dtype=bool) if allow is None else allow
            tag = (nq, allow is not None)
            by_vec = full_ranking(lambda kk, a: ix.search(q, kk, allow=a), n, al)
            by_id = full_ranking(lambda kk, a: ix.search_ids(ids, kk, exclude_self=False, allow=a), n, al)
            assert np.all((by_vec[1] >= 0).sum(axis=1) == al.sum())
            cut = lambda r: (r[0][:, :k], r[1][:, :k])
            plain = ix.search(q, k, allow=allow)
            assert same(plain, cut(by_vec)), tag
            no_self = without(by_id, by_id[1] == ids[:, None])
            assert same(ix.search_ids(ids, k, exclude_self=True, allow=allow), cut(no_self)), tag
            assert same(ix.search_grouped(q, k, g8, allow=allow), dedup(by_vec, g8, k)), tag
            assert same(ix.search_grouped(q, k, g1, allow=allow), plain), tag
            for g in (g8, g1):
                want = dedup(without(by_id, g[np.maximum(by_id[1], 0)] == g[ids][:, None]), g, k)
                got = ix.search_ids_sets(ids, lims, k, groups=g, exclude_own=True, allow=allow)
                assert same(got[:2], want) and np.array_equal(got[2], np.where(want[1] >= 0, qrow, -1)), tag
            assert same(ix.search_ids_sets(ids, lims, k, groups=g1, exclude_own=True, allow=allow)[:2], cut(no_self)), tag
    ix.close()


def test_bad_arguments(clip, clip_lib):
    n, dim = 40, 36
    rows, q, rng = rows_and_queries(dim, n, 2, seed=6)
    ix = make_index(clip, clip_lib, rows, "f16")
    L = clip_lib.lib()
    i32p = C.POINTER(C.c_int32)
    good = np.arange(n, dtype=np.int32)
    bad = good.copy()
    bad[17] = -1

    def call(k, groups):
        dist = np.full((2, max(k, 1)), -3.0, dtype=np.float32)
        ids = np.full((2, max(k, 1)), -3, dtype=np.int64)
        ok = L.clip_amd_index_search_grouped(ix.handle, fp(q), 2, k, groups.ctypes.data_as(i32p) if groups is not None else None, None, fp(dist),
                                             ip(ids))
        return ok, bool(np.all(dist == -3.0) and np.all(ids == -3))

    assert call(5, bad) == (False, True)
    assert call(5, None) == (False, True)
    assert call(0, good) == (False, True)
    assert call(1025, good) == (False, True)
    assert call(5, good)[0] is True
    assert not L.clip_amd_index_search_grouped(None, fp(q), 2, 5, good.ctypes.data_as(i32p), None, None, None)
    with pytest.raises(ValueError):
        ix.search_grouped(q, 5, bad)
    with pytest.raises(ValueError):
        ix.search_grouped(q, 5, good[:-1])
    ix.close()
