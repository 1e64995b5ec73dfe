"""GPU tier of the rank and count queries of the exact index (clip_amd_index_rank[_ids | _device], _count[_device]; k_rank.hip).  The
expected values never come from the code under test: ranks are positions in the complete rankings of Index.search / Index.search_ids
(n <= 1024, so k = n lists every row), insertion points in them for a target outside `allow`, and counts are the segment lengths of
Index.range_search.  Ranks and counts are compared as integers, distances as uint32 bits; no tolerance is involved anywhere."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES

pytestmark = pytest.mark.gpu

DIMS = [36, 512]
N, NQ = 1000, 37                       # four 256-row chunks, the last partial; three 16-column tiles, the last partial
COPIES = np.array([3, 300, 511, 512, 777, N - 1])
POISON = -77


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def setup(clip, clip_lib, dtype, dim):
    """index of N rows with six exact copies of one row planted over the chunks, queries (the first IS that row), targets [NQ, 10]: the
    six copies and four random ids per query"""
    rng = np.random.default_rng(31 * dim)
    rows = rng.standard_normal((N, dim), dtype=np.float32)
    rows[COPIES] = rows[COPIES[0]]
    q = rng.standard_normal((NQ, dim), dtype=np.float32)
    q[0] = rows[COPIES[0]]
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    targets = np.concatenate([np.tile(COPIES, (NQ, 1)), rng.integers(0, N, size=(NQ, 4))], axis=1).astype(np.int64)
    return ix, q, targets, rng


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expect(ranking, targets, allow=None):
    """the definition over complete rankings: ranking(allow) -> (distances, ids) [nq, every row].  A target's distance is the one it has
    in the ranking of every live row; its rank the number of entries of the allowed ranking that come before (distance, id), which for
    a target in that ranking must be its position there.  A target in neither: -1 / +inf."""
    D0, I0 = ranking(None)
    D, I = (D0, I0) if allow is None else ranking(allow)
    ranks = np.full(targets.shape, -1, dtype=np.int64)
    dist = np.full(targets.shape, np.inf, dtype=np.float32)
    for i, j in np.ndindex(*targets.shape):
        t = targets[i, j]
        at = np.flatnonzero(I0[i] == t)
        if t >= 0 and at.size:                                # (-1 pads a ranking shorter than k: no row)
            d = dist[i, j] = D0[i, at[0]]
            ranks[i, j] = np.count_nonzero((I[i] >= 0) & ((D[i] < d) | ((D[i] == d) & (I[i] < t))))
            pos = np.flatnonzero(I[i] == t)
            assert not pos.size or pos[0] == ranks[i, j]
    return ranks, dist


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_definition_csr_and_removed(clip, clip_lib, dtype, dim):
    ix, q, targets, rng = setup(clip, clip_lib, dtype, dim)
    ranking = lambda a: ix.search(q, N, allow=a)
    allow = rng.random(N) < 0.6
    allow[COPIES[:3]], allow[COPIES[3:]] = False, True        # some targets outside the allowed set: insertion points
    for a in (None, allow):
        want = expect(ranking, targets, a)
        got = ix.rank(q, targets, allow=a)
        assert same(got, want)
        # the planted tie: one distance; six consecutive ranks, or, the first three copies not allowed, their common insertion point
        assert len(set(bits(got[1][0, :6]))) == 1 and list(got[0][0, :6] - got[0][0, 0]) == ([0, 1, 2, 3, 4, 5] if a is None else [0, 0, 0, 0, 1, 2])
        # CSR: query 5 has no targets, query 6 has twenty (its own ten twice), the rest their ten: column for column the flat call
        per = [np.empty(0, dtype=np.int64) if i == 5 else np.tile(targets[i], 2 if i == 6 else 1) for i in range(NQ)]
        lims = np.concatenate([[0], np.cumsum([len(p) for p in per])])
        r, d = ix.rank(q, np.concatenate(per), target_lims=lims, allow=a)
        for i in range(NQ):
            seg = slice(lims[i], lims[i + 1])
            assert same((r[seg], d[seg]), tuple(np.tile(w[i], len(per[i]) // 10) for w in want))
    # removed rows (one target among them), target ids -1 and n; through the C entry point over poisoned outputs
    gone = np.concatenate([COPIES[1:2], rng.choice(np.setdiff1d(np.arange(N), COPIES), 50, replace=False)])
    ix.remove(gone)
    t2 = np.concatenate([targets, np.tile([-1, N], (NQ, 1))], axis=1)
    ranks, dist = np.full(t2.shape, POISON, dtype=np.int64), np.full(t2.shape, float(POISON), dtype=np.float32)
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    lims = np.arange(NQ + 1, dtype=np.int64) * t2.shape[1]
    assert clip_lib.lib().clip_amd_index_rank(ix.handle, q.ctypes.data_as(f32p), NQ, np.ascontiguousarray(t2).ctypes.data_as(i64p),
                                              lims.ctypes.data_as(i64p), None, ranks.ctypes.data_as(i64p), dist.ctypes.data_as(f32p)) is True
    assert same((ranks, dist), expect(ranking, t2))
    assert np.all(ranks[:, [1, 10, 11]] == -1) and np.all(np.isinf(dist[:, [1, 10, 11]])) and not np.any(ranks == POISON)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_rank_ids(clip, clip_lib, dtype, dim):
    ix, _, targets, rng = setup(clip, clip_lib, dtype, dim)
    ids = np.concatenate([COPIES[:2], rng.integers(0, N, size=NQ - 2)]).astype(np.int64)
    own = targets == ids[:, None]
    others = np.where(own, (targets + 1) % N, targets)      # exclude_self: a row has no slot in its own list
    assert same(ix.rank_ids(ids, others), expect(lambda a: ix.search_ids(ids, N - 1, allow=a), others))
    assert same(ix.rank_ids(ids, targets, exclude_self=False), expect(lambda a: ix.search_ids(ids, N, exclude_self=False, allow=a), targets))
    ix.remove(ids[4:5])
    keep = ids != ids[4]
    r, d = ix.rank_ids(ids, others)
    assert np.all(r[~keep] == -1) and np.all(np.isinf(d[~keep]))
    assert same((r[keep], d[keep]), expect(lambda a: ix.search_ids(ids[keep], N - 1, allow=a), others[keep]))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_count_and_device_forms(clip, clip_lib, dtype, dim):
    import torch
    ix, q, targets, rng = setup(clip, clip_lib, dtype, dim)
    allow = rng.random(N) < 0.6
    D, _ = ix.search(q, N)
    # radii on the <= boundary (the exact distances of slot 0, of a middle slot, of the planted tie) and 0, negative, 4, +inf
    radii = [D[:, 0], D[:, N // 2], D[0, 0], 0.0, -0.25, 4.0, np.inf]
    for a in (None, allow):
        for r in radii:
            if np.ndim(r) == 0:
                want = np.diff(ix.range_search(q, r, allow=a)[0])
            else:
                want = np.array([np.diff(ix.range_search(q[i:i + 1], r[i], allow=a)[0])[0] for i in range(NQ)])
            assert np.array_equal(ix.count(q, r, allow=a), want)
    assert ix.count(q, D[0, 0])[0] >= 6
    # device forms over poisoned buffers of one slot more: the bytes of the host forms
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(targets).cuda().reshape(-1)
    words = torch.from_numpy(clip_lib.allow_words(allow, N).view(np.int64)).cuda()
    lims = np.arange(NQ + 1, dtype=np.int64) * targets.shape[1]
    dr = torch.full((dt.numel() + 1,), POISON, dtype=torch.int64, device="cuda")
    dd = torch.full((dt.numel() + 1,), float(POISON), dtype=torch.float32, device="cuda")
    ix.rank_device(dq.data_ptr(), NQ, dt.data_ptr(), dr.data_ptr(), dd.data_ptr(), target_lims=lims, d_allow=words.data_ptr())
    rad = torch.from_numpy(np.ascontiguousarray(D[:, N // 2])).cuda()
    dc = torch.full((NQ + 1,), POISON, dtype=torch.int64, device="cuda")
    ix.count_device(dq.data_ptr(), NQ, rad.data_ptr(), dc.data_ptr(), d_allow=words.data_ptr())
    clip.synchronize()
    assert dr[-1].item() == POISON and dd[-1].item() == POISON and dc[-1].item() == POISON
    assert same((dr[:-1].cpu().numpy().reshape(targets.shape), dd[:-1].cpu().numpy().reshape(targets.shape)), ix.rank(q, targets, allow=allow))
    assert np.array_equal(dc[:-1].cpu().numpy(), ix.count(q, D[:, N // 2], allow=allow))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_cases_and_refusals(clip, clip_lib, dtype, capfd):
    ix, q, targets, _ = setup(clip, clip_lib, dtype, 36)
    none = np.empty((0, 36), dtype=np.float32)
    assert ix.rank(none, np.empty(0, dtype=np.int64))[0].shape == (0,) and ix.count(none, 0.5).shape == (0,)
    r, d = ix.rank(q, np.empty(0, dtype=np.int64), target_lims=np.zeros(NQ + 1, dtype=np.int64))
    assert r.shape == (0,) and d.shape == (0,)
    empty = clip_lib.Index(clip, 36, dtype)
    r, d = empty.rank(q, targets[:, 0])
    assert np.all(r == -1) and np.all(np.isinf(d)) and np.all(empty.count(q, np.inf) == 0)
    empty.close()
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L, out = clip_lib.lib(), np.full(NQ, POISON, dtype=np.int64)
    qp, tp, op = q.ctypes.data_as(f32p), np.ascontiguousarray(targets[:, 0]).ctypes.data_as(i64p), out.ctypes.data_as(i64p)
    bad = np.arange(NQ + 1, dtype=np.int64)
    bad[7] = 3                                                   # decreases
    nan = np.full(NQ, np.nan, dtype=np.float32)
    for call in (lambda: L.clip_amd_index_rank(ix.handle, qp, NQ, tp, bad.ctypes.data_as(i64p), None, op, None),
                 lambda: L.clip_amd_index_rank(ix.handle, qp, -1, tp, None, None, op, None),
                 lambda: L.clip_amd_index_rank(ix.handle, qp, NQ, None, None, None, op, None),
                 lambda: L.clip_amd_index_rank(None, qp, NQ, tp, None, None, op, None),
                 lambda: L.clip_amd_index_count(ix.handle, qp, NQ, nan.ctypes.data_as(f32p), None, op),
                 lambda: L.clip_amd_index_count(ix.handle, qp, NQ, None, None, op)):
        assert call() is False and capfd.readouterr().err.strip() and np.all(out == POISON)
    with pytest.raises(ValueError):
        ix.count(q, np.nan)
    ix.close()
