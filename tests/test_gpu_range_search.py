"""GPU tier of range search and near-duplicate pairs (k_join.hip, clip_amd_index_range_search / clip_amd_index_pairs): results against a
float64 numpy reference over the values the index stores (read back from a saved index file), bit-identity with `search`, determinism
across calls, query splits, add splits and save / load, the edge cases of the contract (empty index, size 1, no queries, radius below /
above every distance, zero and non-finite rows, exact duplicates, capacity below the total, count-only calls, bad arguments) and a
1 M-row gallery with planted near-duplicates."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NP_DT = {"f16": np.float16, "f32": np.float32}
I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def quantize(x):
    """the i8 mapping of include/clip_amd.h in numpy (as tests/test_gpu_search_i8.py)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        amax = np.abs(x).max(1, keepdims=True)
        bad = ~np.isfinite(x).all(1, keepdims=True) | ~(amax > 0)
        amax = np.where(bad, np.float32(1), amax).astype(np.float32)
        q = np.rint((x / amax).astype(np.float32) * np.float32(127))
    return np.where(bad, 0, q).astype(np.int8)


def unit64(v):
    v = np.asarray(v, dtype=np.float64)
    nrm = np.sqrt((v * v).sum(1))[:, None]
    return np.where(nrm > 0, v / np.where(nrm > 0, nrm, 1), 0)


def stored64(index, tmp_path, name="rows.index"):
    """float64 operand of the reference distance from the index's own file: the stored values (i8: the stored integers, normalised)"""
    p = str(tmp_path / name)
    index.save(p)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    rows = np.memmap(p, dtype={0: np.float32, 1: np.float16, 3: np.int8}[dt], mode="r", offset=28, shape=(n, dim))
    return unit64(rows) if dt == 3 else np.asarray(rows, dtype=np.float64)


def query64(q, dtype):
    if dtype == "i8":
        return unit64(quantize(q))
    q = np.asarray(q, dtype=np.float32)
    nrm = np.sqrt((q * q).sum(1, dtype=np.float32)).astype(np.float32)[:, None]
    qn = np.where(nrm > 0, q / np.where(nrm > 0, nrm, 1), 0).astype(np.float32)
    return qn.astype(NP_DT[dtype]).astype(np.float64)


def tol_of(dim):
    return dim * 2.0 ** -24 + 1e-6          # test_gpu_search.check


def check_segments(lims, dist, ids, refd, radius, dim, pairs_from=None):
    """every segment against its float64 reference row: all within r - tol reported, none beyond r + tol, distances within tol, the
    contract's order; pairs_from: segment s is row pairs_from[s] of the pairs (only ids > it count)"""
    tol = tol_of(dim)
    r32 = np.float32(radius)
    assert lims[0] == 0 and np.all(np.diff(lims) >= 0) and lims[-1] == len(dist) == len(ids)
    assert np.all(dist <= r32)
    for s in range(refd.shape[0]):
        d, g = dist[lims[s]:lims[s + 1]].astype(np.float64), ids[lims[s]:lims[s + 1]]
        ref = refd[s]
        cand = np.arange(ref.shape[0])
        if pairs_from is not None:
            assert np.all(g > pairs_from[s])
            cand = cand[cand > pairs_from[s]]
        assert len(np.unique(g)) == len(g)
        assert np.all(np.abs(d - ref[g]) <= tol), np.abs(d - ref[g]).max()
        assert np.all(np.diff(d) >= 0) and np.all(np.diff(g)[np.diff(d) == 0] > 0), "distance order, equal distances lower id first"
        want = cand[ref[cand] < radius - tol]
        assert np.all(np.isin(want, g)), "a row well inside the radius is missing"
        assert np.all(ref[g] <= radius + tol)


def planted(rng, n, dim, every=7, noise=0.05):
    """gaussian rows where every `every`-th row is a small perturbation of an earlier one (near-duplicates next to random pairs)"""
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    for r in range(every, n, every):
        rows[r] = rows[r - every // 2 - 1] + noise * rng.standard_normal(dim, dtype=np.float32)
    return rows


CASES = [  # dtype, dim, N, nq
    ("f16", 32, 1, 3), ("f32", 32, 7, 5), ("i8", 64, 7, 5), ("f16", 512, 1000, 64), ("f32", 768, 1000, 20), ("i8", 512, 1000, 300),
    ("f16", 1280, 3000, 17), ("i8", 100, 3000, 1), ("f32", 96, 3000, 16), ("f16", 768, 10000, 130), ("i8", 1280, 10000, 16),
    ("f32", 1024, 10000, 40),
]


@pytest.mark.parametrize("dtype, dim, n, nq", CASES)
def test_exact_against_numpy(clip, clip_lib, tmp_path, dtype, dim, n, nq):
    rng = np.random.default_rng(dim * 11 + n + nq)
    rows = planted(rng, n, dim)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    q[: min(nq, n)] = rows[: min(nq, n)] + 0.1 * rng.standard_normal((min(nq, n), dim), dtype=np.float32)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    radius = 1.0 - 2.5 / np.sqrt(dim)            # a few per cent of the random pairs, every planted one
    r64 = stored64(ix, tmp_path)
    lims, dist, ids = ix.range_search(q, radius)
    assert lims.shape == (nq + 1,)
    check_segments(lims, dist, ids, 1.0 - query64(q, dtype) @ r64.T, radius, dim)
    i, j, d = ix.pairs(radius)
    plims = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    assert np.all(np.diff(i) >= 0)
    sample = np.arange(n) if n <= 3000 else np.sort(rng.choice(n, 400, replace=False))
    refp = 1.0 - r64[sample] @ r64.T
    for k, s in enumerate(sample):
        seg = slice(plims[s], plims[s + 1])
        check_segments(np.array([0, plims[s + 1] - plims[s]]), d[seg], j[seg], refp[k:k + 1], radius, dim, pairs_from=[s])
    if n <= 3000:                                 # the total over every row against the reference count (up to pairs within tol)
        ref = 1.0 - r64 @ r64.T
        iu = np.triu_indices(n, 1)
        tol = tol_of(dim)
        assert (ref[iu] < radius - tol).sum() <= len(d) <= (ref[iu] <= radius + tol).sum()
    ix.close()


@pytest.mark.parametrize("dtype, dim, n", [("f16", 512, 65537), ("i8", 768, 65537), ("f32", 512, 65537), ("f16", 512, 300000), ("i8", 512, 300000)])
def test_sampled_large(clip, clip_lib, tmp_path, dtype, dim, n):
    rng = np.random.default_rng(n + dim)
    rows = planted(rng, n, dim, every=64, noise=0.02)
    q = rows[rng.choice(n, 8, replace=False)] + 0.05 * rng.standard_normal((8, dim), dtype=np.float32)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    radius = 0.05
    r64 = stored64(ix, tmp_path)
    lims, dist, ids = ix.range_search(q, radius)
    check_segments(lims, dist, ids, 1.0 - query64(q, dtype) @ r64.T, radius, dim)
    i, j, d = ix.pairs(radius)
    plims = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    for r in range(64, n, 64):                   # every planted pair is found
        assert r in j[plims[r - 33]:plims[r - 32]], r
    sample = np.sort(rng.choice(n, 48, replace=False))
    refp = 1.0 - r64[sample] @ r64.T
    for k, s in enumerate(sample):
        seg = slice(plims[s], plims[s + 1])
        check_segments(np.array([0, plims[s + 1] - plims[s]]), d[seg], j[seg], refp[k:k + 1], radius, dim, pairs_from=[s])
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_far_pairs_over_many_super_tiles(clip, clip_lib, tmp_path, dtype):
    """random rows and a radius that gives a few pairs per row at any distance in id: pairs in tiles far off the diagonal, across the
    super-tiles of every L2 group and the partial last tiles (N = 300 000: 2344 row tiles, 293 super-tile rows)"""
    rng = np.random.default_rng(77)
    dim, n = 128, 300000
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    radius = 1.0 - 4.2 / np.sqrt(dim)             # cos >= 4.2 sigma: about 4 partners per row among 300 000
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    r64 = stored64(ix, tmp_path)
    i, j, d = ix.pairs(radius)
    assert n < len(i) < 10 * n
    assert (j - i).max() > n // 2 and np.all(j > i)
    plims = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    sample = np.unique(np.concatenate([[0, 1, 127, 128, n - 130, n - 129, n - 2, n - 1], rng.choice(n, 56, replace=False)]))
    refp = 1.0 - r64[sample] @ r64.T
    for k, s in enumerate(sample):
        seg = slice(plims[s], plims[s + 1])
        check_segments(np.array([0, plims[s + 1] - plims[s]]), d[seg], j[seg], refp[k:k + 1], radius, dim, pairs_from=[s])
    ref = 1.0 - r64[-300:] @ r64[-300:].T             # the last rows among themselves (j > i >= n - 300): the partial last tiles
    tol = tol_of(dim)
    iu = np.triu_indices(300, 1)
    tail = (i >= n - 300).sum()
    assert (ref[iu] < radius - tol).sum() <= tail <= (ref[iu] <= radius + tol).sum()
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "f32", "i8"])
def test_bit_identity_with_search(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    dim, n = 256, 5000
    rows = planted(rng, n, dim, every=5, noise=0.3)
    rows[100:110] = rows[99]                      # exact duplicates: ties
    q = rows[rng.choice(n, 40, replace=False)] + 0.2 * rng.standard_normal((40, dim), dtype=np.float32)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    radius = 0.3
    lims, dist, ids = ix.range_search(q, radius)
    sd, si = ix.search(q, 1024)
    seen = 0
    for s in range(len(q)):
        c = lims[s + 1] - lims[s]
        if c <= 1024:
            seen += c > 0
            assert np.array_equal(sd[s, :c].view(np.uint32), dist[lims[s]:lims[s + 1]].view(np.uint32))
            assert np.array_equal(si[s, :c], ids[lims[s]:lims[s + 1]])
            if c < 1024:
                assert not sd[s, c] <= np.float32(radius)
    assert seen >= 10
    i, j, d = ix.pairs(radius)
    plims = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    for r in [0, 4, 99, 100, 101, 2500, 4998, 4999] + rng.choice(n, 40, replace=False).tolist():
        rl, rd, rid = ix.range_search(rows[r:r + 1], radius)
        keep = rid > r
        assert np.array_equal(rd[keep].view(np.uint32), d[plims[r]:plims[r + 1]].view(np.uint32)), r
        assert np.array_equal(rid[keep], j[plims[r]:plims[r + 1]]), r
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_determinism_across_calls_splits_and_save_load(clip, clip_lib, tmp_path, dtype):
    rng = np.random.default_rng(41)
    dim, n = 384, 20000
    rows = planted(rng, n, dim, every=3, noise=0.4)
    q = rows[:300] + 0.3 * rng.standard_normal((300, dim), dtype=np.float32)
    radius = 0.25
    a = clip_lib.Index(clip, dim, dtype)
    a.add(rows)
    r1 = a.range_search(q, radius)
    p1 = a.pairs(radius)
    assert r1[0][-1] > 300 and len(p1[0]) > 1000
    same = lambda x, y: all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(x, y))
    assert same(r1, a.range_search(q, radius)) and same(p1, a.pairs(radius))
    parts = [a.range_search(q[s], radius) for s in (slice(0, 1), slice(1, 17), slice(17, 300))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.uint32), r1[1].view(np.uint32))
    assert np.array_equal(np.concatenate([p[2] for p in parts]), r1[2])
    assert np.array_equal(np.concatenate([np.diff(p[0]) for p in parts]), np.diff(r1[0]))
    b = clip_lib.Index(clip, dim, dtype)
    for lo, hi in zip([0, 1, 1023, 1030, 4097, 13000], [1, 1023, 1030, 4097, 13000, n]):
        b.add(rows[lo:hi])
        b.pairs(radius)                           # interleaved calls do not disturb later results
    assert same(r1, b.range_search(q, radius)) and same(p1, b.pairs(radius))
    path = str(tmp_path / "a.index")
    a.save(path)
    c = clip_lib.Index.load(clip, path)
    assert same(r1, c.range_search(q, radius)) and same(p1, c.pairs(radius))
    for x in (a, b, c):
        x.close()


def raw(ix, radius, cap, lims_n, q=None, out=True):
    """the C call with sentinel-filled lims and output buffers (capacity cap, 8 spare entries); (total, lims, distances, ids)"""
    L = ix.clip_lib
    lims = np.full(lims_n, -5, dtype=np.int64)
    d = np.full(max(cap, 1) + 8, -9.0, dtype=np.float32)
    g = np.full(max(cap, 1) + 8, -11, dtype=np.int64)
    dp = d.ctypes.data_as(F32P) if out else None
    gp = g.ctypes.data_as(I64P) if out else None
    if q is None:
        tot = L.clip_amd_index_pairs(ix.handle, radius, lims.ctypes.data_as(I64P), dp, gp, cap)
    else:
        tot = L.clip_amd_index_range_search(ix.handle, q.ctypes.data_as(F32P), q.shape[0], radius, lims.ctypes.data_as(I64P), dp, gp, cap)
    return tot, lims, d, g


@pytest.mark.parametrize("dtype", ["f16", "f32", "i8"])
def test_edge_cases(clip, clip_lib, dtype):
    rng = np.random.default_rng(51)
    dim = 64
    empty = clip_lib.Index(clip, dim, dtype)
    lims, d, g = empty.range_search(rng.standard_normal((3, dim), dtype=np.float32), 2.5)
    assert lims.tolist() == [0, 0, 0, 0] and len(d) == len(g) == 0
    i, j, d = empty.pairs(2.5)
    assert len(i) == len(j) == len(d) == 0
    one = clip_lib.Index(clip, dim, dtype)
    x = rng.standard_normal((1, dim), dtype=np.float32)
    one.add(x)
    assert len(one.pairs(3.0)[0]) == 0
    lims, d, g = one.range_search(x, 0.01)
    assert lims.tolist() == [0, 1] and g.tolist() == [0]
    lims, d, g = one.range_search(np.zeros((0, dim), np.float32), 1.0)
    assert lims.tolist() == [0] and len(d) == 0

    n = 3000
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    dup_ids = [10, 11, 700, 1999, 2000, 2950]
    for r in dup_ids:
        rows[r] = rows[10]
    rows[500] = 0.0
    if dtype == "i8":
        rows[501, 7] = np.nan
        rows[502, 0] = np.inf
    zero_ids = [500, 501, 502] if dtype == "i8" else [500]
    ix = clip_lib.Index(clip, dim, dtype)
    ix.clip_lib = clip_lib.lib()
    ix.add(rows[:1234])
    ix.add(rows[1234:])
    lims, d, g = ix.range_search(rows[:50], -1.0)         # below every distance
    assert np.all(lims == 0) and len(d) == 0
    i, j, d = ix.pairs(2.0)                               # every pair
    assert len(i) == n * (n - 1) // 2
    assert np.array_equal(np.bincount(i, minlength=n), n - 1 - np.arange(n))
    lims, d, g = ix.range_search(rows[10:11], 1e-3)       # exact duplicates: equal distances, ascending ids
    assert g[: len(dup_ids)].tolist() == dup_ids and np.all(d[: len(dup_ids)] == d[0])
    i, j, d = ix.pairs(0.999)                             # zero (and non-finite) rows: distance exactly 1, never below 1
    assert not np.isin(zero_ids, i).any() and not np.isin(zero_ids, j).any()
    i, j, d = ix.pairs(1.0)
    for z in zero_ids:
        partners = np.concatenate([j[i == z], i[j == z]])
        assert sorted(partners.tolist()) == [x for x in range(n) if x != z]
        assert np.all(d[(i == z) | (j == z)] == 1.0)
    lims, d, g = ix.range_search(np.zeros((2, dim), np.float32), 1.0)    # a zero query: every row at exactly 1, in id order
    assert lims.tolist() == [0, n, 2 * n] and np.all(d == 1.0) and g.tolist() == list(range(n)) * 2

    # capacity below the total: the total and lims, the outputs untouched; count-only calls
    full = ix.pairs(0.8)
    total = len(full[0])
    assert total > 10
    tot, lims, dd, gg = raw(ix, 0.8, total - 1, n + 1)
    assert tot == total and lims[-1] == total and np.array_equal(np.diff(lims), np.bincount(full[0], minlength=n))
    assert np.all(dd == -9.0) and np.all(gg == -11)
    tot, lims2, _, _ = raw(ix, 0.8, 0, n + 1, out=False)
    assert tot == total and np.array_equal(lims, lims2)
    tot, lims3, dd, gg = raw(ix, 0.8, total, n + 1)
    assert tot == total and np.array_equal(lims, lims3)
    assert np.array_equal(dd[:total].view(np.uint32), full[2].view(np.uint32)) and np.array_equal(gg[:total], full[1])
    assert np.all(dd[total:] == -9.0) and np.all(gg[total:] == -11)
    q = rows[:20].copy()
    rl, rd, rg = ix.range_search(q, 0.8)
    tot, lims, dd, gg = raw(ix, 0.8, 0, 21, q=q, out=False)
    assert tot == rl[-1] and np.array_equal(lims, rl)
    for x in (empty, one, ix):
        x.close()


def test_bad_arguments_return_minus_one(clip, clip_lib, capfd):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ix.add(np.ones((4, 32), np.float32))
    h = ix.handle
    q = np.ones((2, 32), np.float32)
    qp = q.ctypes.data_as(F32P)
    lims = np.full(5, -5, np.int64)
    lp = lims.ctypes.data_as(I64P)
    d = np.full(4, -9.0, np.float32)
    g = np.full(4, -11, np.int64)
    dp, gp = d.ctypes.data_as(F32P), g.ctypes.data_as(I64P)
    assert L.clip_amd_index_range_search(h, qp, 2, 0.5, None, dp, gp, 4) == -1
    assert L.clip_amd_index_range_search(h, qp, 2, float("nan"), lp, dp, gp, 4) == -1
    assert L.clip_amd_index_range_search(h, qp, -1, 0.5, lp, dp, gp, 4) == -1
    assert L.clip_amd_index_range_search(h, qp, 2, 0.5, lp, dp, gp, -1) == -1
    assert L.clip_amd_index_range_search(h, qp, 2, 0.5, lp, None, gp, 4) == -1
    assert L.clip_amd_index_range_search(h, qp, 2, 0.5, lp, dp, None, 4) == -1
    assert L.clip_amd_index_range_search(h, None, 2, 0.5, lp, dp, gp, 4) == -1
    assert L.clip_amd_index_pairs(h, 0.5, None, dp, gp, 4) == -1
    assert L.clip_amd_index_pairs(h, float("nan"), lp, dp, gp, 4) == -1
    assert L.clip_amd_index_pairs(h, 0.5, lp, dp, gp, -3) == -1
    assert L.clip_amd_index_pairs(h, 0.5, lp, None, None, 4) == -1
    assert np.all(lims == -5) and np.all(d == -9.0) and np.all(g == -11)
    err = capfd.readouterr().err
    for msg in ("lims is NULL", "radius is NaN", "n_queries -1 < 0", "capacity -1 < 0", "NULL result pointer", "NULL queries"):
        assert msg in err, msg
    assert L.clip_amd_index_range_search(h, None, 0, 0.5, lp, None, None, 0) == 0 and lims[0] == 0     # nothing to do is not an error
    assert ix.pairs(float("inf"))[0].tolist() == [0, 0, 0, 1, 1, 2]
    with pytest.raises(RuntimeError):
        ix.pairs(float("nan"))
    with pytest.raises(ValueError):
        ix.range_search(np.ones((2, 33), np.float32), 0.1)
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_one_million_rows_with_planted_duplicates(clip, clip_lib, tmp_path, dtype):
    torch = pytest.importorskip("torch")
    dim, n, radius = 512, 1 << 20, 0.05
    ix = clip_lib.Index(clip, dim, dtype)
    g = torch.Generator(device="cuda").manual_seed(7)
    piece = 1 << 18
    for r0 in range(0, n, piece):
        t = torch.randn((piece, dim), generator=g, device="cuda", dtype=torch.float32)
        t[63::64] = t[26::64] + 0.02 * torch.randn((piece // 64, dim), generator=g, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        ix.add_device(t.data_ptr(), piece)
        clip.synchronize()
        del t
    i, j, d = ix.pairs(radius)
    r64 = stored64(ix, tmp_path, "big.index")
    plims = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    src = np.arange(26, n, 64)
    for s in src:                                       # every planted pair, once, with the reference distance
        seg = slice(plims[s], plims[s + 1])
        k = np.nonzero(j[seg] == s + 37)[0]
        assert len(k) == 1, s
    sel = np.arange(0, len(src), 97)
    ref = 1.0 - (r64[src[sel]] * r64[src[sel] + 37]).sum(1)
    got = np.array([d[plims[s]:plims[s + 1]][j[plims[s]:plims[s + 1]] == s + 37][0] for s in src[sel]], dtype=np.float64)
    assert np.all(np.abs(got - ref) <= tol_of(dim))
    rng = np.random.default_rng(3)
    sample = np.sort(np.concatenate([rng.choice(n, 60, replace=False), src[:4]]))
    tol = tol_of(dim)
    for s in sample:                                    # totals against a float64 check of sampled rows against the whole gallery
        ref = 1.0 - r64[s + 1:] @ r64[s]
        c = plims[s + 1] - plims[s]
        assert (ref < radius - tol).sum() <= c <= (ref <= radius + tol).sum(), s
    lims, dist, ids = ix.range_search(np.asarray(r64[src[:16]], dtype=np.float32), radius)
    for k, s in enumerate(src[:16]):
        assert s in ids[lims[k]:lims[k + 1]] and s + 37 in ids[lims[k]:lims[k + 1]]
    ix.close()
    os.remove(str(tmp_path / "big.index"))
