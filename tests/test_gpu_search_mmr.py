"""GPU tier of diversified search on the exact index (k_mmr.hip, both routes).  Expected values: the pool is Index.search(q, P), the pair
distances are Index.search_ids among the pool's members (lower id as the query), and the greedy selection is replayed in numpy: in float32
with separately rounded operations (every bit) and in float64 from the stored values of the index's own file (within a measured margin)."""
import struct

import numpy as np
import pytest

from index_subset_common import DTYPES, fp, ip, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(512, 32, 64, 8), (1030, 68, 130, 17)]       # (rows, dim, pool, k); the second: a ragged last fragment, dim % 64 != 0, pool % 64 != 0
ROUTES = {"resident": 1, "streaming": 2}
NQ = 24
F32 = np.float32

@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()

def bursts(rows, dim, seed):
    """(rows f32 [rows, dim]: bursts of three noisy copies of a seeded unit vector; queries f32 [NQ, dim]: noisy copies of stored rows)"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(((rows + 2) // 3, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    x = np.repeat(base, 3, axis=0)[:rows] + 0.1 / np.sqrt(dim) * rng.standard_normal((rows, dim))
    q = x[rng.choice(rows, NQ, replace=False)] + 0.1 / np.sqrt(dim) * rng.standard_normal((NQ, dim))
    return x.astype(F32), q.astype(F32)

def stored64(index, path):
    """the stored values of the index's own file in float64 (i8: the stored integers over their norm)"""
    index.save(str(path))
    _, dim, dt, n = struct.unpack("<IIIQ", open(path, "rb").read(28)[8:])
    rows = np.asarray(np.memmap(path, dtype={0: np.float32, 1: np.float16, 3: np.int8}[dt], mode="r", offset=28, shape=(n, dim)), dtype=np.float64)
    return rows / np.linalg.norm(rows, axis=1, keepdims=True) if dt == 3 else rows

def greedy(dq, pair, k, lam, mu, f):
    """The contract over one pool in precision f: (picked ranks, gaps, the least best-to-second-best score difference over the picks)"""
    lam, mu = f(lam), f(mu)
    m = np.full(len(dq), np.inf, dtype=f)
    free = np.ones(len(dq), dtype=bool)
    picks, gaps, decided = [], [], np.inf
    for t in range(min(k, len(dq))):
        score = (lam * dq).astype(f) - (mu * (m if t else np.zeros_like(m))).astype(f)
        score[~free] = np.inf
        order = np.argsort(score, kind="stable")              # equal scores: the lower rank
        if free.sum() > 1:
            decided = min(decided, float(score[order[1]] - score[order[0]]))
        x = int(order[0])
        picks.append(x)
        gaps.append(m[x])
        free[x] = False
        m = np.minimum(m, pair[x])
    return picks, gaps, decided


@pytest.fixture(scope="module")
def references():
    cache = {}
    yield cache
    for ref in cache.values():
        ref["ix"].close()

def reference(REFERENCE, clip, clip_lib, tmp_path_factory, dtype, shape):
    """Per (dtype, shape), once: index, queries, search's pools, search_ids' pair distances, both in float64, the largest difference"""
    key = (dtype, shape)
    if key not in REFERENCE:
        rows, dim, pool, k = shape
        x, q = bursts(rows, dim, 7 * rows + dim)
        ix = clip_lib.Index(clip, dim, dtype)
        ix.add(x)
        qx = clip_lib.Index(clip, dim, dtype)                  # a stored row is the prepared query: the queries' stored values
        qx.add(q)
        d = tmp_path_factory.mktemp("mmr")
        r64, q64 = stored64(ix, d / "rows.index"), stored64(qx, d / "queries.index")
        qx.close()
        pd, pi = ix.search(q, pool)
        pairs32, pairs64, dq64, err = [], [], [], 0.0
        for t in range(NQ):
            mem = pi[t]
            allow = np.zeros(rows, dtype=np.bool_)
            allow[mem] = True
            sd, si = ix.search_ids(np.sort(mem), pool - 1, exclude_self=True, allow=allow)
            full = np.zeros((rows, rows), dtype=F32)
            for a, (drow, irow) in zip(np.sort(mem), zip(sd, si)):
                hi = irow > a                                  # the entry of the lower id as the query
                full[a, irow[hi]] = drow[hi]
                full[irow[hi], a] = drow[hi]
            p32 = full[np.ix_(mem, mem)]
            p64 = 1.0 - r64[mem] @ r64[mem].T
            d64 = 1.0 - r64[mem] @ q64[t]
            err = max(err, float(np.abs(p32 - p64)[~np.eye(pool, dtype=bool)].max()), float(np.abs(pd[t] - d64).max()))
            for lst, v in ((pairs32, p32), (pairs64, p64), (dq64, d64)):
                lst.append(v)
        REFERENCE[key] = dict(ix=ix, q=q, pd=pd, pi=pi, pairs32=pairs32, pairs64=pairs64, dq64=dq64, err=err)
    return REFERENCE[key]


@pytest.mark.parametrize("lam", [0.2, 0.5, 0.7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_selection(clip, clip_lib, tmp_path_factory, references, dtype, route, shape, lam):
    rows, dim, pool, k = shape
    ref = reference(references, clip, clip_lib, tmp_path_factory, dtype, shape)
    ix = ref["ix"]
    L = clip_lib.lib()
    assert L.clip_amd_test_index_mmr_route(ix.handle, ROUTES[route]) == ROUTES[route]
    try:
        dist, ids, gaps = ix.search_mmr(ref["q"], k, lam, pool=pool)
    finally:
        assert L.clip_amd_test_index_mmr_route(ix.handle, 0) == 0
    mu = F32(1.0) - F32(lam)
    margin = 4 * ref["err"]              # a score takes two distances with weights <= 1 and two roundings
    print("largest |device distance - float64 distance| %.3g, margin %.3g" % (ref["err"], margin))
    reordered = counted = 0
    for t in range(NQ):
        # (b) the contract in float32: every bit, every query
        picks, g, _ = greedy(ref["pd"][t], ref["pairs32"][t], k, lam, mu, np.float32)
        assert np.array_equal(ids[t], ref["pi"][t][picks]), (t, ids[t], ref["pi"][t][picks])
        assert same_bits(dist[t], ref["pd"][t][picks]) and same_bits(gaps[t], np.asarray(g, dtype=F32)), t
        reordered += picks != list(range(k))
        # (a) float64 from the stored values, where every pick is decided by more than the margin
        picks64, g64, decided = greedy(ref["dq64"][t], ref["pairs64"][t], k, lam, float(mu), np.float64)
        if decided > margin:
            counted += 1
            assert np.array_equal(ids[t], ref["pi"][t][picks64]), t
            assert np.abs(dist[t] - ref["dq64"][t][picks64]).max() <= margin and np.abs(gaps[t][1:] - np.asarray(g64[1:])).max() <= margin, t
    assert counted >= NQ - NQ // 4, (counted, margin)
    assert reordered > NQ // 2, reordered                      # diversification reorders: the test is not search's first k in disguise

def raw_mmr(clip_lib, ix, q, k, lam, pool, fill=-7):
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, ix.dim)
    n = max(len(q), 1)
    dist, ids, gaps = np.full((n, max(k, 1)), fill, F32), np.full((n, max(k, 1)), fill, np.int64), np.full((n, max(k, 1)), fill, F32)
    ok = clip_lib.lib().clip_amd_index_search_mmr(ix.handle, fp(q), len(q), k, lam, pool, None, fp(dist), ip(ids), fp(gaps))
    return ok, bool((dist == fill).all() and (ids == fill).all() and (gaps == fill).all())

def same3(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])

@pytest.mark.parametrize("dtype", DTYPES)
def test_consequences_and_forms(clip, clip_lib, dtype, capfd):
    import torch
    rows, dim, pool, k = 300, 36, 70, 9
    x, _ = bursts(rows, dim, 11)
    x[298] = x[6]                                              # one row stored twice
    q = bursts(rows, dim, 12)[0][:37] + x[:37]
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(x)
    L = clip_lib.lib()
    # a duplicate of a picked row: gap 0 up to the rounding of 1 - dot (f16 values carry 2^-11 each: |row|^2 within 2^-10 of 1; f32 / i8:
    # dim roundings of 2^-24), the bits search_ids reports; it competes on lam * dq alone: nothing picked between the copies scores higher
    dd, di, dg = ix.search_mmr(x[6] + F32(0.02) * x[7], pool, 0.5, pool=pool)
    b = int(np.flatnonzero(di[0] == 298)[0])
    twin = ix.search_ids([6], 1)[0][0, 0]
    assert di[0, 0] == 6 and b > 1 and same_bits(dg[0, b], twin) and abs(twin) <= (2.0 ** -10 if dtype == "f16" else dim * 2.0 ** -24)
    score = (F32(0.5) * dd[0]).astype(F32) - (F32(0.5) * dg[0]).astype(F32)
    assert (score[1:b] <= score[b]).all() and (np.diff(score[1:]) >= 0).all()      # (from the second pick on the picked scores never fall)
    # the hook's "resident" is a demand: a pool that cannot fit the LDS is refused (a passing resident case ran the resident kernel)
    if dtype != "i8":
        assert L.clip_amd_test_index_mmr_route(ix.handle, 1) == 1
        with pytest.raises(RuntimeError):
            ix.search_mmr(q, k, 0.5, pool=1024)
        assert L.clip_amd_test_index_mmr_route(ix.handle, 0) == 0 and L.clip_amd_test_index_mmr_route(ix.handle, 3) == -1
    # lambda = 1: search's first k, bit for bit; lambda = 0: starts at the nearest member, then farthest-first (the gaps never rise)
    sd, si = ix.search(q, pool)
    d1, i1, _ = ix.search_mmr(q, k, 1.0, pool=pool)
    assert same_bits(d1, sd[:, :k]) and np.array_equal(i1, si[:, :k])
    d0, i0, g0 = ix.search_mmr(q, k, 0.0, pool=pool)
    assert np.array_equal(i0[:, 0], si[:, 0]) and (g0[:, 0] == np.inf).all() and (np.diff(g0[:, 1:], axis=1) <= 0).all()
    # 37 queries in one call and one at a time; the device form
    whole = ix.search_mmr(q, k, 0.5, pool=pool)
    for t in range(37):
        assert same3([a[t:t + 1] for a in whole], ix.search_mmr(q[t], k, 0.5, pool=pool)), t
    dq = torch.from_numpy(q).cuda()
    od, oi, og = torch.empty((37, k), device="cuda"), torch.empty((37, k), dtype=torch.int64, device="cuda"), torch.empty((37, k), device="cuda")
    torch.cuda.synchronize()
    ix.search_mmr_device(dq.data_ptr(), 37, k, 0.5, od.data_ptr(), oi.data_ptr(), og.data_ptr(), pool=pool)
    clip.synchronize()
    assert same3(whole, (od.cpu().numpy(), oi.cpu().numpy(), og.cpu().numpy()))
    # stored rows as queries: search_mmr of the vectors that were added, with the row itself excluded
    some = np.array([5, 0, 299, 5], dtype=np.int64)
    for t, r in enumerate(some):
        allow = np.ones(rows, dtype=np.bool_)
        allow[r] = False
        assert same3([a[t:t + 1] for a in ix.search_ids_mmr(some, k, 0.5, pool=pool)], ix.search_mmr(x[r], k, 0.5, pool=pool, allow=allow)), t
    # fewer eligible rows than k (an allow bitmap plus removed rows): the tail values
    allow = np.zeros(rows, dtype=np.bool_)
    allow[[3, 4, 5, 100, 200, 250]] = True
    assert ix.remove([4, 200]) == 2
    dt, it, gt = ix.search_mmr(q[:3], k, 0.5, pool=pool, allow=allow)
    assert (np.sort(it[:, :4], axis=1) == [3, 5, 100, 250]).all() and (it[:, 4:] == -1).all()
    assert np.isinf(dt[:, 4:]).all() and np.isinf(gt[:, 4:]).all() and np.isfinite(dt[:, :4]).all() and np.isfinite(gt[:, 1:4]).all()
    # refused arguments: false, a message that names the value, the outputs untouched
    capfd.readouterr()
    for kk, lam, pl, nq, word in ((k, float("nan"), pool, 1, "NaN"), (k, 1.5, pool, 1, "1.5"), (k, -0.25, pool, 1, "-0.25"), (k, 0.5, 1025, 1, "1025"),
                                  (k, 0.5, -1, 1, "-1"), (k, 0.5, k - 1, 1, "exceeds"), (k, 0.5, pool, 0, "n_queries 0"), (0, 0.5, pool, 1, "k")):
        ok, clean = raw_mmr(clip_lib, ix, q[:nq], kk, lam, pl)
        assert ok is False and clean and word in capfd.readouterr().err, (kk, lam, pl, nq)
    empty = clip_lib.Index(clip, dim, dtype)
    ok, clean = raw_mmr(clip_lib, empty, q[:1], k, 0.5, pool)
    assert ok is False and clean and "empty" in capfd.readouterr().err
    empty.close()
    ix.close()


def test_bench_hook(clip_lib):
    assert clip_lib.bench_search_mmr("f16", 3000, 64, 4, 5, 64, 0.5, copies=4, iters=2) > 0
    assert clip_lib.bench_search_mmr("f16", 3000, 64, 4, 65, 64, 0.5, copies=4, iters=1) == -3.0      # k > pool
    assert clip_lib.bench_search_mmr("f16", 3000, 64, 4, 5, 64, 1.5, copies=4, iters=1) == -3.0       # lambda outside [0, 1]
