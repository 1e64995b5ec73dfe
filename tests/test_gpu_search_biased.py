"""GPU tier of the biased search of the exact index (k_bias.hip, clip_amd_index_search_biased / _search_ids_biased): bit for bit against
the index's own distances (range_search) + the bias in numpy f32 ordered by (score, id); against a float64 reference over the stored
values; the equivalences with search; the refusals of the host forms."""
import ctypes as C

import numpy as np
import pytest

from bias_common import all_distances, stored64, top_k

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def bits(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


EXACT = [  # dtype, dim, n, nq, k, +inf rows through the device form
    ("f16", 36, 7, 1, 1, False), ("i8", 512, 7, 17, 100, False), ("f32", 36, 7, 70, 100, False),
    ("f16", 512, 1030, 17, 100, False), ("f32", 36, 1030, 70, 100, False), ("i8", 36, 1030, 1, 100, False), ("i8", 512, 1030, 70, 100, True),
    ("f16", 36, 1030, 17, 1024, False), ("f32", 512, 1030, 1, 1024, False), ("i8", 512, 1030, 17, 1024, False),
    ("f16", 36, 65537, 17, 100, False), ("i8", 512, 65537, 1, 1, False),
]


@pytest.mark.parametrize("dtype, dim, n, nq, k, inf_rows", EXACT)
def test_bit_exact_against_range_search(clip, clip_lib, dtype, dim, n, nq, k, inf_rows):
    rng = np.random.default_rng(dim + n + nq + k)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    bias = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    # exact score ties: copies of a row have its distance bits (read back below) and get its bias; query 0 asks for that row, and the
    # copies sit in other 16-row tiles and other chunks, so they tie at the top of its list
    copies = [0, 3, n // 2, n - 1]
    rows[copies] = rows[3]
    bias[copies] = np.float32(-0.3)
    q[0] = rows[3]
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    D = all_distances(ix, q)
    assert len(set(D[0, copies].tolist())) == 1
    if inf_rows:
        import torch
        dropped = rng.permutation(n)[:n // 20]
        bias[dropped] = np.inf
        dq, db = torch.from_numpy(q).cuda(), torch.from_numpy(bias).cuda()
        dd, ds = (torch.empty((nq, k), dtype=torch.float32, device="cuda") for _ in range(2))
        di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        ix.search_biased_device(dq.data_ptr(), nq, k, db.data_ptr(), dd.data_ptr(), ds.data_ptr(), di.data_ptr())
        clip.synchronize()
        dist, scores, ids = dd.cpu().numpy(), ds.cpu().numpy(), di.cpu().numpy()
        assert not np.isin(ids, dropped).any()
    else:
        dist, scores, ids = ix.search_biased(q, k, bias)
    S = D + bias[None, :]                                   # numpy f32: one addition per pair
    want = top_k(S, k)
    rows = np.arange(nq)[:, None]
    empty = want < 0
    assert np.array_equal(ids, want)
    assert bits(scores) == bits(np.where(empty, np.float32(np.inf), S[rows, np.maximum(want, 0)]))
    assert bits(dist) == bits(np.where(empty, np.float32(np.inf), D[rows, np.maximum(want, 0)]))
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_against_float64(clip, clip_lib, tmp_path, dtype):
    dim, n, nq, k = 512, 1030, 17, 100
    rng = np.random.default_rng(2024)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    bias = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    dist, scores, ids = ix.search_biased(q, k, bias)
    rows64, q64 = stored64(ix, q, dtype, str(tmp_path / "rows.index"))
    refd = 1.0 - q64 @ rows64.T
    refs = refd + bias.astype(np.float64)[None, :]
    tol = dim * 2.0 ** -24 + 1e-6
    stol = tol + 2.0 ** -24 * (2 + np.abs(bias).max())
    ambiguous = 0
    for i in range(nq):
        g = ids[i]
        assert len(set(g.tolist())) == k and g.min() >= 0
        assert np.abs(dist[i] - refd[i, g]).max() <= tol and np.abs(scores[i] - refs[i, g]).max() <= stol
        assert np.all(np.diff(scores[i]) >= 0)
        kth = np.sort(refs[i])[k - 1]
        top = set(np.argsort(refs[i])[:k].tolist())
        for x in set(g.tolist()) ^ top:
            assert abs(refs[i, x] - kth) <= stol
        ambiguous += int((np.abs(refs[i, g] - kth) <= stol).sum()) - 1      # (the k-th itself is always in its band)
    assert ambiguous <= 0.02 * nq * k
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "f32", "i8"])
def test_equivalences(clip, clip_lib, dtype):
    dim, n, nq, k = 36, 1030, 70, 100
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    bias = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    allow = rng.random(n) < 0.6
    # no bias and a zero bias are search
    d0, i0 = ix.search(q, k, allow=allow)
    for b in (None, np.zeros(n, dtype=np.float32)):
        d, s, i = ix.search_biased(q, k, b, allow=allow)
        assert bits(d, s, i) == bits(d0, d0, i0)
    # 70 queries in one call and in calls of 1 + 16 + 53
    whole = ix.search_biased(q, k, bias, allow=allow)
    parts = [ix.search_biased(q[a:b], k, bias, allow=allow) for a, b in ((0, 1), (1, 17), (17, 70))]
    assert bits(*whole) == bits(*(np.concatenate(x) for x in zip(*parts)))
    # stored rows as the queries: the same stored rows searched with the row's own bit cleared
    some = np.array([5, 700, 1029, 5], dtype=np.int64)
    # (the other side is the vector form, anchored by the range_search test above, over the vector that was added as that row: search_ids'
    # contract; and without a bias the by-id form is the existing search_ids)
    d1, i1 = ix.search_ids(some, k, exclude_self=True)
    assert bits(*ix.search_ids_biased(some, k, None, exclude_self=True)) == bits(d1, d1, i1)
    by_id = ix.search_ids_biased(some, k, bias, exclude_self=True)
    for t, r in enumerate(some):
        own = np.ones(n, dtype=bool)
        own[r] = False
        one = ix.search_biased(rows[r:r + 1], k, bias, allow=own)
        assert bits(*(x[t:t + 1] for x in by_id)) == bits(*one)
    # removed rows and an allowed subset: an index that never held the other rows
    gone = rng.permutation(n)[:100]
    ix.remove(gone)
    keep = allow.copy()
    keep[gone] = False
    d, s, i = ix.search_biased(q, k, bias, allow=allow)
    small = clip_lib.Index(clip, dim, dtype)
    small.add(rows[keep])
    d2, s2, i2 = small.search_biased(q, k, bias[keep])
    back = np.append(np.flatnonzero(keep), -1)
    assert bits(d, s, i) == bits(d2, s2, back[i2])
    small.close()
    ix.close()


@pytest.mark.parametrize("what", ["nan", "k0", "k1025"])
def test_refusals(clip, clip_lib, what):
    n, dim = 300, 36
    rng = np.random.default_rng(3)
    ix = clip_lib.Index(clip, dim, "f16")
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    q = rng.standard_normal((2, dim), dtype=np.float32)
    bias = np.zeros(n, dtype=np.float32)
    k = {"nan": 5, "k0": 0, "k1025": 1025}[what]
    if what == "nan":
        bias[123] = np.nan
    outs = [np.full((2, max(k, 1)), 7, dtype=t) for t in (np.float32, np.float32, np.int64)]
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    ok = clip_lib.lib().clip_amd_index_search_biased(ix.handle, q.ctypes.data_as(f32p), 2, k, bias.ctypes.data_as(f32p), None, outs[0].ctypes.data_as(f32p),
                                                     outs[1].ctypes.data_as(f32p), outs[2].ctypes.data_as(i64p))
    assert not ok and all(np.all(o == 7) for o in outs)
    ix.close()
