"""GPU tier of density modes (k_modes.hip, clip_amd_index_modes).  The oracle is the library's own pair list: `Index.pairs(max(radius,
link))` of the same index holds every distance the contract speaks of, from the same score chain, so the contract in numpy over those pairs
(tests/modes_common.py: from_pairs) must give exactly the labels, parents, densities, mode count and the bits of every parent distance:
every comparison here is for equality.  For masked cases the pairs come from an index that holds only the eligible rows, ids mapped back.
One case per dtype is also checked against float64 distances of the stored values, at a radius and a link inside gaps of those distances.
Data: bursts of exact and noisy copies (ties in density and in distance, both decided by id), planted near-duplicates in a dense random
graph, random walks on the sphere, shuffled and, 600 rows long, unshuffled (a forest about 600 deep: every doubling pass is needed)."""
import ctypes as C
import struct

import numpy as np
import pytest

from modes_common import CHAIN_RADIUS, D1, bursts, from_pairs, planted, same_bits, walks

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
I32P = C.POINTER(C.c_int32)
F32P = C.POINTER(C.c_float)
U64P = C.POINTER(C.c_uint64)
DTYPES = ("f16", "f32", "i8")
INF = float("inf")


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


def make_index(clip, clip_lib, rows, dtype):
    ix = clip_lib.Index(clip, rows.shape[1], dtype)
    if len(rows):
        ix.add(rows)
    return ix


def call(clip_lib, ix, radius, link, allow=None, want=(True, True, True)):
    """clip_amd_index_modes itself: (return value, labels, parent or None, parent distance or None, density or None)"""
    n = len(ix)
    words = None if allow is None else clip_lib.allow_words(allow, n)
    labels = np.full(n, -7, dtype=np.int64)
    parent = np.full(n, -7, dtype=np.int64) if want[0] else None
    dist = np.full(n, -7, dtype=np.float32) if want[1] else None
    density = np.full(n, -7, dtype=np.int32) if want[2] else None
    ret = clip_lib.lib().clip_amd_index_modes(ix.handle, float(radius), float(link), None if words is None else words.ctypes.data_as(U64P),
                                              labels.ctypes.data_as(I64P), None if parent is None else parent.ctypes.data_as(I64P),
                                              None if dist is None else dist.ctypes.data_as(F32P),
                                              None if density is None else density.ctypes.data_as(I32P))
    return ret, labels, parent, dist, density


def same_result(got, want):
    """(labels, parent, parent distance, density) twice: equal, the distances as bits"""
    return len(got) == len(want) == 4 and all(same_bits(a, b) for a, b in zip(got, want))


def check_against_pairs(clip_lib, ix, radius, link, pairs=None):
    """the call against the contract over the index's own pairs (every live row eligible); returns (pairs, result)"""
    n = len(ix)
    i, j, d = ix.pairs(max(radius, link)) if pairs is None else pairs
    live = ix.live_mask() if ix.live < n else None
    want = from_pairs(n, i, j, d, radius, link, live)
    ret, labels, parent, dist, density = call(clip_lib, ix, radius, link)
    assert np.array_equal(density, want[3]), "densities differ from the counts over pairs"
    assert np.array_equal(parent, want[1])
    assert same_bits(dist, want[2]), "parent distances differ from the pairs' as bits"
    assert np.array_equal(labels, want[0])
    assert ret == want[4]
    assert ret == np.count_nonzero(labels == np.arange(n))
    return (i, j, d), (labels, parent, dist, density)


def data_of(kind, rng, n, dim):
    """(rows, radius, a link below it, a link above it)"""
    if kind == "walks":
        return walks(rng, n, dim), CHAIN_RADIUS, 0.9 * D1, 2.5 * D1
    if kind == "bursts":                             # exact copies: 0; noisy copy to original: about 0.00125; two noisy copies: about 0.0025
        return bursts(rng, n, dim), 0.01, 0.001, 0.02
    radius = 1.0 - 2.5 / np.sqrt(dim)                # a few per cent of the random pairs: a dense random graph
    return planted(rng, n, dim), radius, 0.8 * radius, 1.0 - 2.2 / np.sqrt(dim)


@pytest.mark.parametrize("dim", (40, 512))
@pytest.mark.parametrize("n", (1, 2, 127, 128, 129, 1025, 2100))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("bursts", "planted", "walks"))
def test_equals_contract_over_pairs(clip, clip_lib, kind, dtype, n, dim):
    rng = np.random.default_rng(1000 * dim + n + len(kind))
    rows, radius, below, above = data_of(kind, rng, n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    pairs = ix.pairs(above)
    results = {}
    for link in (below, radius, above):              # one pair list serves the three: from_pairs compares with radius and link itself
        _, results[link] = check_against_pairs(clip_lib, ix, radius, link, pairs)
    if n >= 127:                                     # not trivial: trees of several rows, and the link changes the forest
        labels, parent, dist, density = results[radius]
        assert density.max() >= 2 and np.bincount(labels).max() >= 3
        assert np.count_nonzero(results[below][1] >= 0) < np.count_nonzero(parent >= 0) <= np.count_nonzero(results[above][1] >= 0)
        assert same_bits(results[below][3], density) and same_bits(results[above][3], density)      # density does not depend on link
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bursts_with_exact_copies_lowest_id_first(clip, clip_lib, dtype):
    """ties everywhere: the copies of one row have equal densities and are at equal distances from each other, so ids decide both"""
    rng = np.random.default_rng(17)
    n, dim = 700, 40
    rows = bursts(rng, n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    _, (labels, parent, dist, density) = check_against_pairs(clip_lib, ix, 0.01, 0.01)
    _, inverse, counts = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    checked = 0
    for g in np.flatnonzero(counts >= 2):
        ids = np.flatnonzero(inverse == g)          # ascending
        assert len(set(density[ids].tolist())) == 1 and len(set(labels[ids].tolist())) == 1
        assert np.all(parent[ids[1:]] == ids[0])     # every later copy hangs under the lowest id, at the copies' own distance
        assert len(set(dist[ids[1:]].tobytes()[4 * t:4 * t + 4] for t in range(len(ids) - 1))) == 1
        checked += len(ids) - 1
    assert checked >= 100
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unshuffled_walks_make_a_forest_600_deep(clip, clip_lib, dtype):
    """a walk in id order is a path: the interior densities tie at 2, so every interior row's parent is its lower-id neighbour, and the
    root is the walk's second row (its first row has one neighbour only and hangs under it): 598 steps deep, all ten (here eleven:
    n = 1200) doubling passes are needed"""
    n, dim, length = 1200, 512, 600
    rows = walks(np.random.default_rng(5), n, dim, length=length, shuffle=False)
    ix = make_index(clip, clip_lib, rows, dtype)
    _, (labels, parent, dist, density) = check_against_pairs(clip_lib, ix, CHAIN_RADIUS, CHAIN_RADIUS)
    for r0 in (0, length):
        assert density[r0] == 1 and density[r0 + length - 1] == 1 and np.all(density[r0 + 1:r0 + length - 1] == 2)
        assert parent[r0] == r0 + 1 and parent[r0 + 1] == -1
        assert np.array_equal(parent[r0 + 2:r0 + length], np.arange(r0 + 1, r0 + length - 1))
        assert np.all(labels[r0:r0 + length] == r0 + 1)          # one label per walk
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_float64_distances(clip, clip_lib, tmp_path, dtype):
    n, dim = 300, 100
    rows = walks(np.random.default_rng(77), n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    r64 = stored64(ix, tmp_path)
    d64 = 1.0 - r64 @ r64.T
    np.fill_diagonal(d64, np.inf)
    v = np.unique(d64[np.triu_indices(n, 1)])
    tol = tol_of(dim)

    def in_gap(lo_bound, hi_bound):
        gaps = [(hi - lo, lo, hi) for lo, hi in zip(v[:-1], v[1:]) if hi - lo > 2 * tol and lo_bound < hi < hi_bound]
        assert gaps, "no gap wider than 2 tol between %g and %g" % (lo_bound, hi_bound)
        _, lo, hi = max(gaps)
        return float(np.float32((lo + hi) / 2))

    radius = in_gap(2.0 * D1, 2.4 * D1)              # the steps of the walks and about half of the two-step pairs: densities 2 ... 4
    link = in_gap(3.0 * D1, 4.5 * D1)
    for value in (radius, link):                     # (the f32 rounding of the midpoint stays inside its gap)
        k = np.searchsorted(v, value)
        assert v[k] - value > tol and value - v[k - 1] > tol
    labels, parent, dist, density = ix.modes(radius, link)
    want_density = (d64 <= radius).sum(1)
    assert np.array_equal(density, want_density) and density.max() >= 3
    ids = np.arange(n)
    outranks = (want_density[None, :] > want_density[:, None]) | ((want_density[None, :] == want_density[:, None]) & (ids[None, :] < ids[:, None]))
    cand = np.where(outranks & (d64 <= link), d64, np.inf)            # [x, y]: y outranks x and is within link of it
    has = parent >= 0
    assert np.array_equal(has, np.isfinite(cand.min(1))) and has.sum() >= 200
    x = np.flatnonzero(has)
    assert np.all(outranks[x, parent[x]])                             # every parent outranks its child
    assert np.all(np.abs(d64[x, parent[x]] - dist[x].astype(np.float64)) <= tol)
    assert np.all(cand.min(1)[x] >= dist[x].astype(np.float64) - 2 * tol)          # no outranking row within link is closer
    assert np.all(np.isinf(dist[~has]))
    root = np.where(has, parent, ids)
    for _ in range(10):
        root = root[root]
    assert np.array_equal(labels, root)
    ix.close()


def test_contract_edges(clip, clip_lib):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ret, labels, parent, dist, density = call(clip_lib, ix, 0.5, 0.5)        # empty index
    assert ret == 0 and labels.size == 0
    assert all(a.shape == (0,) for a in ix.modes(0.5))
    rng = np.random.default_rng(3)
    ix.add(rng.standard_normal((1, 32), dtype=np.float32))
    for radius, link in ((-1.0, -1.0), (0.5, 0.5), (4.0, INF)):             # one row: a mode of density 0 at any scale
        ret, labels, parent, dist, density = call(clip_lib, ix, radius, link)
        assert ret == 1 and labels.tolist() == [0] and parent.tolist() == [-1] and dist.tolist() == [np.inf] and density.tolist() == [0]
    ix.add(rng.standard_normal((199, 32), dtype=np.float32))
    ix.remove([0, 5])
    live = ix.live_mask()
    n = 200
    ret, labels, parent, dist, density = call(clip_lib, ix, -1.0, -1.0)     # below every distance: every live row a mode of density 0
    assert ret == 198 and np.array_equal(labels, np.where(live, np.arange(n), -1))
    assert np.all(parent == -1) and np.all(np.isinf(dist)) and np.array_equal(density, np.where(live, 0, -1))
    ret, labels, parent, dist, density = call(clip_lib, ix, -1.0, INF)      # densities all 0: rank is the id, the lowest live id the only root
    assert ret == 1 and np.array_equal(labels, np.where(live, 1, -1)) and np.all(parent[live][1:] >= 1) and np.all(parent[live][1:] < np.flatnonzero(live)[1:])
    all_pairs = ix.pairs(4.0)
    assert len(all_pairs[0]) == 198 * 197 // 2
    check_against_pairs(clip_lib, ix, -1.0, INF, all_pairs)
    for radius in (0.6, 0.8, 4.0):                                           # link = +inf: only the top-ranked row is a root
        _, (labels, parent, dist, density) = check_against_pairs(clip_lib, ix, radius, INF, all_pairs)
        top = np.flatnonzero(density == density.max())[0]
        assert np.array_equal(labels, np.where(live, top, -1)) and parent[top] == -1 and np.count_nonzero(parent[live] < 0) == 1
    check_against_pairs(clip_lib, ix, 0.7, 0.5, all_pairs)
    check_against_pairs(clip_lib, ix, 0.5, 0.7, all_pairs)
    want = call(clip_lib, ix, 0.7, 0.8)
    assert 1 < want[0] < 198
    for mask in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):      # NULL optional outputs
        got = call(clip_lib, ix, 0.7, 0.8, want=mask)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        assert all(g is None or same_bits(g, w) for g, w in zip(got[2:], want[2:]))
        assert [g is None for g in got[2:]] == [not m for m in mask]
    # refused before any launch: outputs untouched
    for radius, link in ((float("nan"), 0.5), (0.5, float("nan"))):
        ret, labels, parent, dist, density = call(clip_lib, ix, radius, link)
        assert ret == -1 and np.all(labels == -7) and np.all(parent == -7) and np.all(dist == -7) and np.all(density == -7)
    assert L.clip_amd_index_modes(ix.handle, 0.5, 0.5, None, None, parent.ctypes.data_as(I64P), dist.ctypes.data_as(F32P), density.ctypes.data_as(I32P)) == -1
    assert np.all(parent == -7) and np.all(dist == -7) and np.all(density == -7)
    with pytest.raises(ValueError):
        ix.modes(float("nan"))
    with pytest.raises(ValueError):
        ix.modes_device(0.5, 1, link=float("nan"))
    with pytest.raises(RuntimeError):
        ix.modes_device(0.5, None)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_allow_and_compact_equal_a_fresh_index(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    n, dim = 400, 40
    rows = np.concatenate([walks(rng, 250, dim, length=50), bursts(rng, 150, dim)])[rng.permutation(n)]
    radius, link = CHAIN_RADIUS, 2.0 * D1
    ix = make_index(clip, clip_lib, rows, dtype)
    keep = rng.random(n) < 0.8
    keep[:3] = [False, True, False]
    sel = np.flatnonzero(keep)
    fresh = make_index(clip, clip_lib, rows[sel], dtype)
    _, (fl, fp, fd, fn) = check_against_pairs(clip_lib, fresh, radius, link)
    assert np.bincount(fl).max() >= 5 and fn.max() >= 3
    whole = ix.modes(radius, link)
    assert not np.array_equal(whole[3][sel], fn)     # (the rows left out were somebody's neighbours: the mask matters)

    def mapped(labels, parent, dist, density):
        """a result over all ids against the fresh index's, ids mapped back"""
        assert np.all(labels[~keep] == -1) and np.all(parent[~keep] == -1) and np.all(np.isinf(dist[~keep])) and np.all(density[~keep] == -1)
        assert np.array_equal(labels[sel], sel[fl])
        assert np.array_equal(parent[sel], np.where(fp >= 0, sel[np.maximum(fp, 0)], -1))
        assert same_bits(dist[sel], fd)
        assert np.array_equal(density[sel], fn)

    mapped(*ix.modes(radius, link, allow=keep))                  # allow as a mask
    mapped(*ix.modes(radius, link, allow=sel[::-1]))             # allow as ids
    ret = call(clip_lib, ix, radius, link, allow=keep)[0]
    assert ret == np.count_nonzero(fp < 0)
    gone = np.flatnonzero(~keep)
    ix.remove(gone[: len(gone) // 2])                            # half removed, the other half not allowed
    mapped(*ix.modes(radius, link, allow=keep))
    ix.remove(gone)
    mapped(*ix.modes(radius, link))                              # remove alone
    check_against_pairs(clip_lib, ix, radius, link)
    new_ids = ix.compact()
    assert np.array_equal(new_ids[sel], np.arange(len(sel)))
    assert same_result(ix.modes(radius, link), (fl, fp, fd, fn))
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism(clip, clip_lib, tmp_path, dtype):
    import torch
    rng = np.random.default_rng(41)
    n, dim = 1000, 100
    rows = np.concatenate([walks(rng, 600, dim), bursts(rng, 400, dim)])
    radius, link = CHAIN_RADIUS, 2.0 * D1
    ix = make_index(clip, clip_lib, rows, dtype)
    first = ix.modes(radius, link)
    assert np.bincount(first[0]).max() >= 5 and first[3].max() >= 3
    for _ in range(2):
        assert same_result(ix.modes(radius, link), first)
    p = str(tmp_path / "m.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_result(loaded.modes(radius, link), first)
    loaded.close()
    split = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 130), (130, 131), (131, 777), (777, n)):
        split.add(rows[lo:hi])
    assert same_result(split.modes(radius, link), first)
    split.close()
    tl = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    tp = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    td = torch.full((n,), -7, dtype=torch.float32, device="cuda")
    tn = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.modes_device(radius, tl.data_ptr(), link, tp.data_ptr(), td.data_ptr(), tn.data_ptr())
    clip.synchronize()
    assert same_result(tuple(t.cpu().numpy() for t in (tl, tp, td, tn)), first)
    allow = np.arange(n) % 5 != 2
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    tl.fill_(-7)
    torch.cuda.synchronize()
    ix.modes_device(radius, tl.data_ptr(), link, d_allow=tw.data_ptr())          # labels only, over a subset
    clip.synchronize()
    assert np.array_equal(tl.cpu().numpy(), ix.modes(radius, link, allow=allow)[0])
    assert same_bits(td.cpu().numpy(), first[2]) and same_bits(tn.cpu().numpy(), first[3])      # (the NULL outputs were not written)
    ix.close()


def test_20000_planted_rows(clip, clip_lib):
    """a dense random graph over 20 000 rows at dim 64: more than a million pairs, densities in the hundreds"""
    rng = np.random.default_rng(51)
    n, dim = 20000, 64
    ix = make_index(clip, clip_lib, planted(rng, n, dim), "f16")
    radius = 1.0 - 2.5 / np.sqrt(dim)
    (i, j, d), (labels, parent, dist, density) = check_against_pairs(clip_lib, ix, radius, 1.0 - 2.4 / np.sqrt(dim))
    assert 500_000 <= len(i) <= 4_000_000 and density.max() >= 100
    ix.close()
