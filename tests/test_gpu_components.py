"""GPU tier of connected components (k_components.hip, clip_amd_index_components).  The oracle is the library's own pair list: the edges
`Index.pairs` reports at the same radius come from the same score chain, so a host union over them must give exactly the labels, and the
minimum over a row's pairs exactly the bits of its nearest distance: every comparison here is for equality.  One case per dtype is also
checked against components computed in float64 from the stored values, at a radius inside a gap of the pair distances.
Data that makes the union work: path-shaped components with shuffled ids (random walks on the sphere), bursts of exact and near copies,
planted near-duplicates in a dense random graph; then the edges of the contract, masks (remove, allow, compact), determinism (calls,
save / load, add splits, device form) and one denser case of 20 000 rows."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)
U64P = C.POINTER(C.c_uint64)
DTYPES = ("f16", "f32", "i8")
STEP = 0.3                                            # tangent step of the walks: one step is at distance 1 - 1 / sqrt(1 + STEP^2)
D1 = 1.0 - 1.0 / np.sqrt(1.0 + STEP * STEP)           # 0.0422; two steps in independent directions: about twice that
CHAIN_RADIUS = 1.5 * D1


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def stored64(index, tmp_path, name="rows.index"):
    """float64 operand of the reference distance from the index's own file: the stored values (i8: the stored integers, normalised)"""
    p = str(tmp_path / name)
    index.save(p)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    rows = np.asarray(np.memmap(p, dtype={0: np.float32, 1: np.float16, 3: np.int8}[dt], mode="r", offset=28, shape=(n, dim)), dtype=np.float64)
    if dt == 3:
        nrm = np.sqrt((rows * rows).sum(1))[:, None]
        rows = np.where(nrm > 0, rows / np.where(nrm > 0, nrm, 1), 0)
    return rows


def tol_of(dim):
    return dim * 2.0 ** -24 + 1e-6          # the bound of the f32 score chain against float64 (tests/test_gpu_range_search.py)


def planted(rng, n, dim, every=7, noise=0.05):
    """gaussian rows where every `every`-th row is a small perturbation of an earlier one (near-duplicates next to random pairs)"""
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    for r in range(every, n, every):
        rows[r] = rows[r - every // 2 - 1] + noise * rng.standard_normal(dim, dtype=np.float32)
    return rows


def walks(rng, n, dim, length=100, shuffle=True):
    """chains of `length` rows, v[t + 1] = normalise(v[t] + STEP u) with u a random unit tangent at v[t]; ids randomly permuted"""
    rows = np.empty((n, dim), dtype=np.float64)
    for r0 in range(0, n, length):
        v = rng.standard_normal(dim)
        v /= np.linalg.norm(v)
        for t in range(r0, min(n, r0 + length)):
            rows[t] = v
            u = rng.standard_normal(dim)
            u -= (u @ v) * v
            v = v + STEP * u / np.linalg.norm(u)
            v /= np.linalg.norm(v)
    if shuffle:
        rows = rows[rng.permutation(n)]
    return (rows * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)       # (the index normalises)


def bursts(rng, n, dim):
    """groups of 1 ... 12 rows: an original, then exact copies and noisy copies in turn; ids randomly permuted"""
    rows = np.empty((n, dim), dtype=np.float32)
    r = 0
    while r < n:
        m = min(n - r, int(rng.integers(1, 13)))
        rows[r] = rng.standard_normal(dim, dtype=np.float32)
        for c in range(1, m):
            rows[r + c] = rows[r] if c % 2 else rows[r] + 0.05 * rng.standard_normal(dim, dtype=np.float32)
        r += m
    return rows[rng.permutation(n)]


def host_labels(n, i, j):
    """the lowest id of every row's component from an edge list (numpy label propagation to the fixed point)"""
    labels = np.arange(n, dtype=np.int64)
    while True:
        nxt = labels.copy()
        np.minimum.at(nxt, i, labels[j])
        np.minimum.at(nxt, j, labels[i])
        nxt = nxt[nxt]
        if np.array_equal(nxt, labels):
            return labels
        labels = nxt


def from_pairs(n, i, j, d, eligible=None):
    """(labels, nearest distance, nearest id, groups) of the contract from a pair list"""
    labels = host_labels(n, i, j)
    if eligible is not None:
        labels[~eligible] = -1
    near = np.full(n, np.inf, dtype=np.float32)
    nid = np.full(n, -1, dtype=np.int64)
    rows, other, dd = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([d, d])
    order = np.lexsort((other, dd, rows))            # per row: distance ascending, then the other id
    first = order[np.concatenate([[True], np.diff(rows[order]) != 0])] if rows.size else order
    near[rows[first]] = dd[first]
    nid[rows[first]] = other[first]
    groups = int(np.count_nonzero((labels == np.arange(n)) & (nid >= 0)))
    return labels, near, nid, groups


def call(clip_lib, ix, radius, allow=None, want_dist=True, want_id=True):
    """clip_amd_index_components itself: (return value, labels, nearest distance or None, nearest id or None)"""
    n = len(ix)
    words = None if allow is None else clip_lib.allow_words(allow, n)
    labels = np.full(n, -7, dtype=np.int64)
    dist = np.full(n, -7, dtype=np.float32) if want_dist else None
    nid = np.full(n, -7, dtype=np.int64) if want_id else None
    ret = clip_lib.lib().clip_amd_index_components(ix.handle, float(radius), None if words is None else words.ctypes.data_as(U64P),
                                                   labels.ctypes.data_as(I64P), None if dist is None else dist.ctypes.data_as(F32P),
                                                   None if nid is None else nid.ctypes.data_as(I64P))
    return ret, labels, dist, nid


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_pairs(clip_lib, ix, radius, eligible=None):
    """the call against the union of the index's own pairs; returns (pairs, result)"""
    n = len(ix)
    i, j, d = ix.pairs(radius)
    want = from_pairs(n, i, j, d, eligible)
    ret, labels, dist, nid = call(clip_lib, ix, radius)
    assert np.array_equal(labels, want[0])
    assert same_bits(dist, want[1]), "nearest distances differ from the minimum over pairs as bits"
    assert np.array_equal(nid, want[2])
    assert ret == want[3]
    return (i, j, d), (labels, dist, nid)


def make_index(clip, clip_lib, rows, dtype):
    ix = clip_lib.Index(clip, rows.shape[1], dtype)
    if len(rows):
        ix.add(rows)
    return ix


def has_fork(i, j):
    """a row with two lower-id near rows that are not near each other: what "remember my lowest neighbour" gets wrong"""
    edges = set(zip(i.tolist(), j.tolist()))
    lower = {}
    for a, b in edges:
        lower.setdefault(b, []).append(a)
    for b, below in lower.items():
        below.sort()
        for x in range(len(below)):
            for y in range(x + 1, len(below)):
                if (below[x], below[y]) not in edges:
                    return True
    return False


@pytest.mark.parametrize("dim", (32, 100, 512))
@pytest.mark.parametrize("n", (1, 7, 128, 129, 300, 1000))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("chains", "bursts", "planted"))
def test_equals_union_of_pairs(clip, clip_lib, kind, dtype, n, dim):
    rng = np.random.default_rng(1000 * dim + n + len(kind))
    if kind == "chains":
        rows, radius = walks(rng, n, dim), CHAIN_RADIUS
    elif kind == "bursts":
        rows, radius = bursts(rng, n, dim), 0.01
    else:
        rows, radius = planted(rng, n, dim), 1.0 - 2.5 / np.sqrt(dim)        # a few per cent of the random pairs: a dense random graph
    ix = make_index(clip, clip_lib, rows, dtype)
    (i, j, d), (labels, _, _) = check_against_pairs(clip_lib, ix, radius)
    if kind == "chains" and n >= 128:                # not trivial: long paths that cross tiles, and forks below a row
        assert np.bincount(labels).max() >= 50
        assert has_fork(i, j)
    if kind != "chains" and n >= 128:
        assert len(i) > 0 and np.bincount(labels).max() >= 3
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_labels_against_float64_components(clip, clip_lib, tmp_path, dtype):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n, dim = 300, 100
    rows = walks(np.random.default_rng(77), n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    r64 = stored64(ix, tmp_path)
    dist = 1.0 - r64 @ r64.T
    v = np.unique(dist[np.triu_indices(n, 1)])
    tol = tol_of(dim)
    gaps = [(hi - lo, lo, hi) for lo, hi in zip(v[:-1], v[1:]) if hi - lo >= 8 * tol and D1 < hi < 2.5 * D1]
    assert gaps, "no gap of 8 tol between the one-step and the two-step distances"
    _, lo, hi = max(gaps)
    radius = float((lo + hi) / 2)
    adj = np.triu(dist <= radius, 1)
    assert adj.sum() >= 200                          # the steps of the walks are edges
    _, comp = connected_components(csr_matrix(adj), directed=False)
    lowest = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(lowest, comp, np.arange(n))
    labels, near, nid = ix.components(radius)
    assert np.array_equal(labels, lowest[comp])
    assert np.bincount(labels).max() >= 50
    has = adj.any(0) | adj.any(1)
    assert np.array_equal(np.isfinite(near), has) and np.array_equal(nid >= 0, has)
    full = np.where(adj | adj.T, dist, np.inf)
    assert np.all(np.abs(near[has].astype(np.float64) - full.min(1)[has]) <= tol)
    ix.close()


def test_contract_edges(clip, clip_lib):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ret, labels, dist, nid = call(clip_lib, ix, 0.5)                         # empty index
    assert ret == 0 and labels.size == 0
    lab, nd, ni = ix.components(0.5)
    assert lab.shape == nd.shape == ni.shape == (0,)
    rng = np.random.default_rng(3)
    ix.add(rng.standard_normal((1, 32), dtype=np.float32))
    for radius in (-1.0, 0.5, 4.0):                                          # one row: no pair at any radius
        ret, labels, dist, nid = call(clip_lib, ix, radius)
        assert ret == 0 and labels.tolist() == [0] and dist.tolist() == [np.inf] and nid.tolist() == [-1]
    ix.add(rng.standard_normal((199, 32), dtype=np.float32))
    ix.remove([0, 5])
    live = ix.live_mask()
    ret, labels, dist, nid = call(clip_lib, ix, -1.0)                        # below every distance: every live row its own label
    assert ret == 0 and np.array_equal(labels, np.where(live, np.arange(200), -1))
    assert np.all(np.isinf(dist)) and np.all(nid == -1)
    ret, labels, dist, nid = call(clip_lib, ix, 4.0)                         # above every distance: one component, the lowest live id
    assert ret == 1 and np.array_equal(labels, np.where(live, 1, -1))
    assert np.all(np.isfinite(dist[live])) and np.all(np.isinf(dist[~live])) and np.all(nid[~live] == -1)
    check_against_pairs(clip_lib, ix, 4.0, live)
    want = call(clip_lib, ix, 0.7)
    for wd, wi in ((False, True), (True, False), (False, False)):           # NULL nearest pointers
        ret, labels, dist, nid = call(clip_lib, ix, 0.7, want_dist=wd, want_id=wi)
        assert ret == want[0] and np.array_equal(labels, want[1])
        assert dist is None or same_bits(dist, want[2])
        assert nid is None or np.array_equal(nid, want[3])
    # refused before any launch: outputs untouched
    ret, labels, dist, nid = call(clip_lib, ix, float("nan"))
    assert ret == -1 and np.all(labels == -7) and np.all(dist == -7) and np.all(nid == -7)
    assert L.clip_amd_index_components(ix.handle, 0.5, None, None, dist.ctypes.data_as(F32P), nid.ctypes.data_as(I64P)) == -1
    assert L.clip_amd_index_components(None, 0.5, None, labels.ctypes.data_as(I64P), None, None) == -1
    assert np.all(dist == -7) and np.all(nid == -7)
    with pytest.raises(RuntimeError):
        ix.components(float("nan"))
    with pytest.raises(RuntimeError):
        ix.components_device(float("nan"), 1)
    with pytest.raises(RuntimeError):
        ix.components_device(0.5, None)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_duplicates_and_zero_rows(clip, clip_lib, dtype):
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((140, 64), dtype=np.float32)
    rows[[3, 50, 130]] = rows[1]                     # exact duplicates, across the tile edge
    rows[[7, 90, 135]] = 0                           # zero rows: at distance exactly 1 from everything
    ix = make_index(clip, clip_lib, rows, dtype)
    for radius in (0.0, 1e-3, 0.999, 1.0):
        check_against_pairs(clip_lib, ix, radius)
    labels, _, _ = ix.components(1e-3)
    assert labels[[1, 3, 50, 130]].tolist() == [1, 1, 1, 1] and labels[7] == 7
    labels, _, _ = ix.components(1.0)
    assert np.all(labels == 0)                       # through a zero row everything hangs together at radius 1
    ix.close()


def test_removed_middle_link_splits_the_chain(clip, clip_lib):
    rows = walks(np.random.default_rng(21), 60, 64, length=60, shuffle=False)
    ix = make_index(clip, clip_lib, rows, "f16")
    labels, near, nid = ix.components(CHAIN_RADIUS)
    assert np.all(labels == 0) and np.all(np.isfinite(near))
    assert ix.remove([30]) == 1
    live = ix.live_mask()
    _, (labels, near, nid) = check_against_pairs(clip_lib, ix, CHAIN_RADIUS, live)
    assert np.all(labels[:30] == 0) and labels[30] == -1 and np.all(labels[31:] == 31)
    assert np.isinf(near[30]) and nid[30] == -1 and not np.any(nid == 30)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_allow_and_compact_equal_a_fresh_index(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    n, dim = 300, 100
    rows = walks(rng, n, dim, length=75)
    ix = make_index(clip, clip_lib, rows, dtype)
    keep = rng.random(n) < 0.8
    keep[:3] = [False, True, False]
    sel = np.flatnonzero(keep)
    fresh = make_index(clip, clip_lib, rows[sel], dtype)
    _, (fl, fd, fi) = check_against_pairs(clip_lib, fresh, CHAIN_RADIUS)
    assert np.bincount(fl).max() >= 10 and len(np.unique(fl)) > n // 75

    def mapped(labels, dist, nid):
        """a result over all ids against the fresh index's"""
        assert np.all(labels[~keep] == -1) and np.all(np.isinf(dist[~keep])) and np.all(nid[~keep] == -1)
        assert np.array_equal(labels[sel], sel[fl])
        assert same_bits(dist[sel], fd)
        assert np.array_equal(nid[sel], np.where(fi >= 0, sel[np.maximum(fi, 0)], -1))

    mapped(*ix.components(CHAIN_RADIUS, allow=keep))
    mapped(*ix.components(CHAIN_RADIUS, allow=sel[::-1]))
    gone = np.flatnonzero(~keep)
    ix.remove(gone[: len(gone) // 2])                # half removed, the other half not allowed
    mapped(*ix.components(CHAIN_RADIUS, allow=keep))
    ix.remove(gone)
    mapped(*ix.components(CHAIN_RADIUS))
    new_ids = ix.compact()
    assert np.array_equal(new_ids[sel], np.arange(len(sel)))
    labels, dist, nid = ix.components(CHAIN_RADIUS)
    assert np.array_equal(labels, fl) and same_bits(dist, fd) and np.array_equal(nid, fi)
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism(clip, clip_lib, tmp_path, dtype):
    import torch
    rng = np.random.default_rng(41)
    n, dim = 1000, 100
    rows = np.concatenate([walks(rng, 600, dim), bursts(rng, 400, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    first = ix.components(CHAIN_RADIUS)
    assert np.bincount(first[0]).max() >= 50
    for _ in range(2):
        again = ix.components(CHAIN_RADIUS)
        assert all(same_bits(a, b) for a, b in zip(first, again))
    p = str(tmp_path / "c.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert all(same_bits(a, b) for a, b in zip(first, loaded.components(CHAIN_RADIUS)))
    loaded.close()
    split = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 130), (130, 131), (131, 777), (777, n)):
        split.add(rows[lo:hi])
    assert all(same_bits(a, b) for a, b in zip(first, split.components(CHAIN_RADIUS)))
    split.close()
    tl = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    td = torch.full((n,), -7, dtype=torch.float32, device="cuda")
    ti = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.components_device(CHAIN_RADIUS, tl.data_ptr(), td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert all(same_bits(a, b.cpu().numpy()) for a, b in zip(first, (tl, td, ti)))
    allow = np.arange(n) % 5 != 2
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    tl.fill_(-7)
    torch.cuda.synchronize()
    ix.components_device(CHAIN_RADIUS, tl.data_ptr(), d_allow=tw.data_ptr())      # labels only, over a subset
    clip.synchronize()
    assert np.array_equal(tl.cpu().numpy(), ix.components(CHAIN_RADIUS, allow=allow)[0])
    assert np.all(td.cpu().numpy() == first[1])      # (the NULL outputs were not written)
    ix.close()


def test_denser_case_20000_rows(clip, clip_lib):
    """100 bursts of 200 copies in 20 000 rows: about 2 million pairs, 100 labels"""
    rng = np.random.default_rng(51)
    n, dim = 20000, 64
    base = rng.standard_normal((100, dim), dtype=np.float32)
    rows = (np.repeat(base, 200, axis=0) + 0.03 * rng.standard_normal((n, dim), dtype=np.float32))[rng.permutation(n)]
    ix = make_index(clip, clip_lib, rows, "f16")
    (i, j, d), (labels, _, _) = check_against_pairs(clip_lib, ix, 0.01)
    assert 1_500_000 <= len(i) <= 2_000_000 and len(np.unique(labels)) <= 200
    ix.close()
