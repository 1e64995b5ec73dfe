"""GPU tier of k-NN voting over the exact index (clip_amd_index_vote[_device], _vote_ids, _vote_graph[_device]; k_vote.hip).  The expected
values never come from the code under test: they are the rankings of existing entry points (Index.search / Index.search_ids with the
voters, the live, allowed and labelled rows, as the allowed set) with the definition applied in numpy (vote_common.vote_of: lexsort by
-votes, first rank).  Classes, votes and ids are compared exactly, distances as uint32 bits; no tolerance is involved anywhere."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES
from vote_common import same_votes, vote_of, voters_of

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
BIG = 2 ** 31 - 1
POISON = -77


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


def data(dim, n, nq, seed=0):
    """rows with six exact copies of one row planted (ids spread over the index), queries, labels: 5 classes, one class numbered
    2^31 - 1, about a fifth of the rows unlabelled; the six copies carry six different labels, so equal distances and vote ties occur"""
    rng = np.random.default_rng(977 * dim + n + seed)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    copies = np.array([3, 64, 65, 130, n - 40, n - 1])
    rows[copies] = rows[copies[0]]
    if nq:
        q[0] = rows[copies[0]]                                # a query at distance ~0 of all six
    labels = rng.integers(0, 5, size=n).astype(np.int64)
    labels[rng.random(n) < 0.08] = BIG
    labels[rng.random(n) < 0.2] = -1
    labels[copies] = [0, 1, 2, 3, 4, BIG]
    return rows, q, labels, copies, rng


def expect(ix, q, labels, k, m, allow=None, ranking=None):
    """the definition over Index.search's ranking of the voters (ranking: a longer one computed before, whose first k columns are read)"""
    if ranking is None:
        ranking = ix.search(q, k, allow=voters_of(labels, allow))
    return vote_of(ranking[0], ranking[1], labels, k, m)


def expect_ids(ix, ids, labels, k, m, exclude_self=True, allow=None):
    d, i = ix.search_ids(ids, k, exclude_self=exclude_self, allow=voters_of(labels, allow))
    return vote_of(d, i, labels, k, m)


def expect_graph(ix, labels, k, m, allow=None):
    """row i = vote_ids(i, exclude_self) for a live row, empty for a removed one"""
    n = len(ix)
    live = ix.live_mask()
    c, v = np.full((n, m), -1, dtype=np.int32), np.zeros((n, m), dtype=np.int32)
    d, i = np.full((n, m), np.inf, dtype=np.float32), np.full((n, m), -1, dtype=np.int64)
    ids = np.flatnonzero(live)
    if len(ids):
        c[ids], v[ids], d[ids], i[ids] = expect_ids(ix, ids, labels, k, m, True, allow)
    return c, v, d, i


def set_route(clip_lib, ix, route):
    assert clip_lib.lib().clip_amd_test_index_knn_route(ix.handle, route) == route


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_definition(clip, clip_lib, dtype, dim):
    n, nq = 300, 37
    rows, q, labels, copies, rng = data(dim, n, nq)
    ix = make_index(clip, clip_lib, rows, dtype)
    for allow in (None, rng.random(n) < 0.6):
        ranking = ix.search(q, n, allow=voters_of(labels, allow))
        ties = 0
        for k in (1, 5, 64, 300):
            for m in sorted({1, min(3, k), k}):
                got = ix.vote(q, k, labels, m=m, allow=allow)
                assert got[0].shape == (nq, m) and got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[3].dtype == np.int64
                want = expect(ix, q, labels, k, m, ranking=ranking)
                assert same_votes(got, want), (k, m, allow is not None)
                if m >= 2:
                    ties += int(np.sum((got[1][:, 0] == got[1][:, 1]) & (got[1][:, 0] > 0)))
        assert ties > 0                                       # vote ties were decided by the nearest member
        assert np.all(np.diff(ranking[0][0, :4].view(np.uint32)) == 0) or allow is not None      # the copies: equal distances
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_edges(clip, clip_lib, dtype, dim):
    n, nq = 1500, 5
    rows, q, labels, copies, rng = data(dim, n, nq)
    ix = make_index(clip, clip_lib, rows, dtype)
    # all labels distinct, m = k: search_subset's result with votes all 1
    distinct = rng.permutation(n).astype(np.int64) * 1000
    distinct[7] = BIG
    allow = np.arange(n) % 5 != 2                             # 1200 voters: more than the largest k
    for k in (64, 1024):
        d, i = ix.search(q, k, allow=allow)
        got = ix.vote(q, k, distinct, m=k, allow=allow)
        assert np.all(i >= 0) and np.array_equal(got[0], distinct[i].astype(np.int32)) and np.all(got[1] == 1)
        assert same_votes(got, (got[0], got[1], d, i))
    # k larger than the number of voters: the list is shorter
    few = np.full(n, -1, dtype=np.int64)
    few[[2, 300, 301, 700, 1499, 64, 65]] = [4, 4, 9, 9, 9, BIG, 0]
    got = ix.vote(q, 64, few, m=64)
    assert same_votes(got, expect(ix, q, few, 64, 64)) and np.all(got[1].sum(axis=1) == 7) and np.all(got[0][:, 4:] == -1)
    # no voter at all: all-empty rows
    for none_labels, none_allow in ((np.full(n, -1), None), (labels, np.zeros(n, dtype=bool))):
        got = ix.vote(q, 5, none_labels, m=3, allow=none_allow)
        assert np.all(got[0] == -1) and np.all(got[1] == 0) and np.all(np.isposinf(got[2])) and np.all(got[3] == -1)
    # every voter in one class at k = 1024: the longest run the fold can meet
    one = np.full(n, 123456, dtype=np.int64)
    got = ix.vote(q, 1024, one, m=3)
    d, i = ix.search(q, 1, allow=None)
    assert np.all(got[0][:, 0] == 123456) and np.all(got[1][:, 0] == 1024) and np.all(got[0][:, 1:] == -1) and np.all(got[1][:, 1:] == 0)
    assert same_votes(got, expect(ix, q, one, 1024, 3)) and np.array_equal(got[3][:, :1], i)
    # 1024 distinct classes at k = m = 1024
    got = ix.vote(q, 1024, distinct, m=1024)
    assert same_votes(got, expect(ix, q, distinct, 1024, 1024)) and np.all(got[1] == 1)
    ix.close()
    # an empty index: every row empty
    empty = clip_lib.Index(clip, dim, dtype)
    got = empty.vote(q, 4, np.zeros(0, dtype=np.int64), m=2)
    assert got[0].shape == (nq, 2) and np.all(got[0] == -1) and np.all(got[1] == 0) and np.all(np.isposinf(got[2])) and np.all(got[3] == -1)
    got = empty.vote_graph(4, np.zeros(0, dtype=np.int64), m=2)
    assert got[0].shape == (0, 2)
    empty.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_removed_rows_and_compaction(clip, clip_lib, dtype, dim):
    n, nq, k, m = 300, 11, 20, 4
    rows, q, labels, copies, rng = data(dim, n, nq)
    ix = make_index(clip, clip_lib, rows, dtype)
    gone = rng.permutation(n)[:n // 3]
    assert ix.remove(gone) == len(gone)
    before = ix.vote(q, k, labels, m=m)
    assert same_votes(before, expect(ix, q, labels, k, m))    # (Index.search never returns a removed row)
    assert not np.isin(before[3], gone).any()
    graph_before = ix.vote_graph(k, labels, m=m)
    new_ids = ix.compact()
    kept = new_ids >= 0
    mapped = np.append(new_ids, -1)                           # -1 -> -1
    after = ix.vote(q, k, labels[kept], m=m)
    assert same_votes(after, (before[0], before[1], before[2], mapped[before[3]]))
    graph_after = ix.vote_graph(k, labels[kept], m=m)
    assert same_votes(graph_after, (graph_before[0][kept], graph_before[1][kept], graph_before[2][kept], mapped[graph_before[3][kept]]))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", [300, 1100])
def test_vote_ids_and_graph_on_both_routes(clip, clip_lib, dtype, dim, n):
    k, m = 9, 3
    rows, _, labels, copies, rng = data(dim, n, 0)
    ix = make_index(clip, clip_lib, rows, dtype)
    gone = np.array([0, 5, 129, n - 2])
    assert ix.remove(gone) == len(gone)
    every = np.abs(labels)                                    # every live row a voter: the tiled route's single pass
    allow = rng.random(n) < 0.7
    ids = np.setdiff1d(rng.permutation(n)[:50], gone)
    for lab, al in ((labels, None), (labels, allow), (every, None)):
        want = expect_graph(ix, lab, k, m, al)
        assert np.all(want[0][gone] == -1) and np.all(want[1][gone] == 0)
        unl = np.flatnonzero(~voters_of(lab, al, ix.live_mask()) & ix.live_mask())
        if len(unl):
            assert np.any(want[1][unl] > 0)                   # rows that are no voters still ask
        for route in (1, 2):
            set_route(clip_lib, ix, route)
            got = ix.vote_graph(k, lab, m=m, allow=al)
            assert same_votes(got, want), (route, al is not None)
            ix.vote_block(128)                                # blocks of 128 rows: 300 and 1100 are straddled
            assert same_votes(ix.vote_graph(k, lab, m=m, allow=al), want), (route, "blocked")
            ix.vote_block(0)
        got = ix.vote_ids(ids, k, lab, m=m, allow=al)
        assert same_votes(got, tuple(w[ids] for w in want))
        ix.vote_block(128 if n > 300 else 16)
        assert same_votes(ix.vote_ids(ids, k, lab, m=m, allow=al), got)
        ix.vote_block(0)
        # exclude_self = False: a labelled row votes for itself
        own = ix.vote_ids(ids, k, lab, m=m, exclude_self=False, allow=al)
        assert same_votes(own, expect_ids(ix, ids, lab, k, m, False, al))
        assert not same_votes(own, got)
    set_route(clip_lib, ix, 0)
    nearest = ix.vote_ids(ids, 1, every, m=1, exclude_self=False)
    d, i = ix.search_ids(ids, 1, exclude_self=False)
    assert np.array_equal(nearest[3], i) and np.array_equal(nearest[0][:, 0], every[i[:, 0]].astype(np.int32))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_splitting_and_repeats(clip, clip_lib, dtype):
    n, nq, k, m = 300, 37, 12, 3
    rows, q, labels, copies, rng = data(36, n, nq)
    ix = make_index(clip, clip_lib, rows, dtype)
    whole = ix.vote(q, k, labels, m=m)
    a, b = ix.vote(q[:20], k, labels, m=m), ix.vote(q[20:], k, labels, m=m)
    assert same_votes(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), whole)
    assert same_votes(ix.vote(q, k, labels, m=m), whole)
    ix.vote_block(16)
    assert same_votes(ix.vote(q, k, labels, m=m), whole)
    ix.vote_block(0)
    g = ix.vote_graph(k, labels, m=m)
    assert same_votes(ix.vote_graph(k, labels, m=m), g)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_forms(clip, clip_lib, dtype):
    import torch
    n, nq, dim, k, m = 600, 37, 36, 10, 3
    rows, q, labels, copies, rng = data(dim, n, nq)
    allow = rng.random(n) < 0.6
    ix = make_index(clip, clip_lib, rows, dtype)
    assert ix.remove([1, 200]) == 2
    tq = torch.from_numpy(q).cuda()
    dev_labels = labels.copy()
    dev_labels[labels < 0] = -5                               # device forms: any negative value is unlabelled
    tl = torch.from_numpy(dev_labels.astype(np.int32)).cuda()
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()

    def buffers(rows_out):                                    # [rows_out + 1][m]: the last row is the guard
        return (torch.full((rows_out + 1, m), POISON, dtype=torch.int32, device="cuda"), torch.full((rows_out + 1, m), POISON, dtype=torch.int32, device="cuda"),
                torch.full((rows_out + 1, m), float(POISON), dtype=torch.float32, device="cuda"), torch.full((rows_out + 1, m), POISON, dtype=torch.int64, device="cuda"))

    def check(bufs, rows_out, want):
        got = tuple(b.cpu().numpy() for b in bufs)
        for g in got:
            assert np.all(g[rows_out] == POISON) and not np.any(g[:rows_out] == POISON)
        assert same_votes(tuple(g[:rows_out] for g in got), want)

    torch.cuda.synchronize()
    for al, twp in ((None, None), (allow, tw.data_ptr())):
        bufs = buffers(nq)
        torch.cuda.synchronize()
        ix.vote_device(tq.data_ptr(), nq, k, tl.data_ptr(), *[b.data_ptr() for b in bufs], m=m, d_allow=twp)
        clip.synchronize()
        check(bufs, nq, ix.vote(q, k, labels, m=m, allow=al))
        for route in (1, 2):
            set_route(clip_lib, ix, route)
            bufs = buffers(n)
            torch.cuda.synchronize()
            ix.vote_graph_device(k, tl.data_ptr(), *[b.data_ptr() for b in bufs], m=m, d_allow=twp)
            clip.synchronize()
            check(bufs, n, ix.vote_graph(k, labels, m=m, allow=al))
        set_route(clip_lib, ix, 0)
    ix.close()


def test_refusals(clip, clip_lib, capfd):
    n, nq, dim = 100, 3, 36
    rows, q, labels, copies, rng = data(dim, 200, nq)
    rows, labels = rows[:n], labels[:n]
    ix = make_index(clip, clip_lib, rows, "f16")
    L = clip_lib.lib()
    i32p, i64p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    cls, votes = np.full((n, 4), POISON, dtype=np.int32), np.full((n, 4), POISON, dtype=np.int32)
    dist, out = np.full((n, 4), float(POISON), dtype=np.float32), np.full((n, 4), POISON, dtype=np.int64)
    outs = (cls.ctypes.data_as(i32p), votes.ctypes.data_as(i32p), dist.ctypes.data_as(f32p), out.ctypes.data_as(i64p))
    good = np.ascontiguousarray(labels, dtype=np.int32)
    bad = good.copy()
    bad[17] = -2
    ids = np.array([3, n, 5], dtype=np.int64)
    qp, gp, bp, idp = q.ctypes.data_as(f32p), good.ctypes.data_as(i32p), bad.ctypes.data_as(i32p), ids.ctypes.data_as(i64p)
    capfd.readouterr()
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 4, 4, bp, None, *outs) is False
    assert L.clip_amd_index_vote_ids(ix.handle, idp, 1, 4, 4, 1, bp, None, *outs) is False
    assert L.clip_amd_index_vote_graph(ix.handle, 4, 4, bp, None, *outs) is False
    err = capfd.readouterr().err
    assert err.count("labels[17] = -2") == 3
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 3, 4, gp, None, *outs) is False
    assert L.clip_amd_index_vote_graph(ix.handle, 3, 4, gp, None, *outs) is False
    assert L.clip_amd_index_vote_graph_device(ix.handle, 3, 4, gp, None, *outs) is False      # (refused before any pointer is used)
    assert capfd.readouterr().err.count("m = 4 exceeds k = 3") == 3
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 4, 0, gp, None, *outs) is False
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 1025, 4, gp, None, *outs) is False
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 4, 4, None, None, *outs) is False
    assert L.clip_amd_index_vote(ix.handle, qp, nq, 4, 4, gp, None, outs[0], None, outs[2], outs[3]) is False
    err = capfd.readouterr().err
    assert "m = 0" in err and "k = 1025" in err and "labels is NULL" in err and "NULL" in err.splitlines()[-1]
    assert L.clip_amd_index_vote_ids(ix.handle, idp, 3, 4, 4, 1, gp, None, *outs) is False
    assert "id %d" % n in capfd.readouterr().err
    ix.remove([5])
    assert L.clip_amd_index_vote_ids(ix.handle, idp, 3, 4, 4, 1, gp, None, *outs) is False
    for a in (cls, votes, dist, out):
        assert np.all(a == POISON)
    assert L.clip_amd_index_vote_ids(ix.handle, idp, 1, 4, 4, 1, gp, None, *outs) is True      # the same call with a good id goes through
    assert not np.any(cls[0] == POISON) and np.all(cls[1:] == POISON)
    ix.close()
