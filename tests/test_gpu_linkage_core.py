"""GPU tier of the mutual-reachability tree (k_linkage.hip's CORE instantiation, clip_amd_index_linkage_core).  The oracle is Kruskal's
algorithm (tests/linkage_core_common.py) over the library's own numbers: `Index.pairs(radius=4)` reports every pair with the bits of the
score chain and `Index.search_ids(..., k)[:, k - 1]` is the contract's definition of a core distance, so the tree must come out byte for
byte: every comparison here is for equality.  Both routes of the neighbour search; k = 0 against `linkage`; DBSCAN* consistency with
`components`; a finite link; masks; determinism; the device form; argument errors; one row and an empty index."""
import ctypes as C

import numpy as np
import pytest

from linkage_core_common import CHAIN_RADIUS, bursts, core_kruskal, planted, same_bits, walks

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)
U64P = C.POINTER(C.c_uint64)
DTYPES = ("f16", "f32", "i8")
KINDS = {"walks": walks, "bursts": bursts, "planted": planted}
KS = (1, 5, 33)
SHAPES = [(n, 100) for n in (1, 2, 3, 127, 128, 129, 300, 1100)] + [(300, 32), (300, 512)]


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


def same_edges(got, want):
    return all(same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b)) for a, b in zip(got, want))


def eligible_pairs(ix, eligible=None):
    """every pair of eligible rows with the distance `pairs` reports (no distance of unit vectors exceeds 2)"""
    i, j, d = ix.pairs(4.0)
    live = ix.live_mask() if eligible is None else eligible & ix.live_mask()
    use = live[i] & live[j]
    m = int(live.sum())
    assert int(use.sum()) == m * (m - 1) // 2
    return i[use], j[use], d[use], live


def core_by_search(ix, k, eligible):
    """the contract's core column: entry k - 1 of search_ids over the eligible rows, +inf outside them, -inf over them for k = 0"""
    core = np.full(len(ix), np.inf, dtype=np.float32)
    ids = np.flatnonzero(eligible)
    if k == 0:
        core[ids] = -np.inf
    elif len(ids):
        core[ids] = ix.search_ids(ids, k, exclude_self=True, allow=eligible)[0][:, k - 1]
    return core


def oracle(ix, k, link=np.inf, eligible=None):
    i, j, d, live = eligible_pairs(ix, eligible)
    core = core_by_search(ix, k, live)
    return core_kruskal(len(ix), i, j, d, core, link) + (core,)


def call(clip_lib, ix, k, link, allow=None, want_core=True):
    """clip_amd_index_linkage_core itself over poisoned outputs: (return value, lo, hi, weights, core)"""
    n = len(ix)
    words = None if allow is None else clip_lib.allow_words(allow, n)
    lo = np.full(max(n - 1, 1), -7, dtype=np.int64)
    hi = np.full(max(n - 1, 1), -7, dtype=np.int64)
    w = np.full(max(n - 1, 1), -7, dtype=np.float32)
    core = np.full(n + 3, -7, dtype=np.float32)
    ret = clip_lib.lib().clip_amd_index_linkage_core(ix.handle, int(k), float(link), None if words is None else words.ctypes.data_as(U64P),
                                                     lo.ctypes.data_as(I64P), hi.ctypes.data_as(I64P), w.ctypes.data_as(F32P),
                                                     core.ctypes.data_as(F32P) if want_core else None)
    return ret, lo, hi, w, core


def set_route(clip_lib, ix, route):
    assert clip_lib.lib().clip_amd_test_index_knn_route(ix.handle, route) >= 0


@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_equals_kruskal_over_the_index_s_own_pairs_and_neighbours(clip, clip_lib, kind, dtype, n, dim):
    rng = np.random.default_rng(1000 * dim + n + len(kind))
    rows = KINDS[kind](rng, n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    i, j, d, live = eligible_pairs(ix)
    for k in KS:
        core = core_by_search(ix, k, live)
        assert np.all(np.isinf(core)) == (k >= n)                            # fewer than k other rows: +inf
        want = core_kruskal(n, i, j, d, core)
        assert len(want[0]) == n - 1
        routes = (0, 1, 2) if n >= 300 and dim == 100 else (0,)              # automatic, the scan, the tiled kernel
        for route in routes:
            set_route(clip_lib, ix, route)
            ret, lo, hi, w, got_core = call(clip_lib, ix, k, np.inf)
            assert ret == n - 1 and same_edges((lo[:ret], hi[:ret], w[:ret]), want), "the tree differs from Kruskal (route %d)" % route
            assert same_bits(got_core[:n], core), "core is not the k-th distance of search_ids (route %d)" % route
            assert np.all(lo[ret:] == -7) and np.all(hi[ret:] == -7) and np.all(w[ret:] == -7) and np.all(got_core[n:] == -7)
        set_route(clip_lib, ix, 0)
    got = ix.linkage_core(5)
    assert same_edges(got, core_kruskal(n, i, j, d, core_by_search(ix, 5, live)) + (core_by_search(ix, 5, live),))
    ret, lo, hi, w, untouched = call(clip_lib, ix, 5, np.inf, want_core=False)               # core may be NULL
    assert ret == n - 1 and same_edges((lo[:ret], hi[:ret], w[:ret]), got[:3]) and np.all(untouched == -7)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_0_is_linkage_byte_for_byte(clip, clip_lib, dtype):
    rng = np.random.default_rng(17)
    n, dim = 600, 100
    rows = np.concatenate([walks(rng, 400, dim), bursts(rng, 200, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    allow = rng.random(n) < 0.7
    for link, mask in ((None, None), (CHAIN_RADIUS, None), (None, allow), (0.0, allow)):
        lo, hi, w, core = ix.linkage_core(0, link, allow=mask)
        assert same_edges((lo, hi, w), ix.linkage(link, allow=mask))
        want = np.where(np.ones(n, dtype=bool) if mask is None else mask, -np.inf, np.inf).astype(np.float32)
        assert same_bits(core, want)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cut_is_dbscan_star_and_a_finite_link_is_a_prefix(clip, clip_lib, dtype):
    rng = np.random.default_rng(61)
    n, dim, k = 600, 100, 5
    rows = np.concatenate([walks(rng, 400, dim), bursts(rng, 200, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    lo, hi, w, core = ix.linkage_core(k)
    assert len(lo) == n - 1 and np.all(np.isfinite(core))
    # under w every row nearer to x than core[x] is at one weight from x: the tie-break of the edge order decided many edges
    assert np.count_nonzero(np.diff(w) == 0) > 0.1 * (len(w) - 1)
    merges = np.unique(w)
    picks = merges[np.linspace(0, len(merges) - 1, 6).astype(int)]
    radii = []
    for m in picks:
        radii += [m, np.nextafter(m, np.float32(-1))]
    for radius in radii:
        dense = core <= radius
        labels = clip_lib.cut_linkage(n, lo, hi, w, radius=float(radius))
        assert np.array_equal(labels[~dense], np.flatnonzero(~dense)), radius                 # every other row is a group of its own
        assert not np.isin(labels[dense], np.flatnonzero(~dense)).any()
        if dense.any():
            want, _, _ = ix.components(float(radius), allow=dense)
            assert np.array_equal(labels[dense], want[dense]), radius
    for link in (float(picks[2]), float(np.nextafter(picks[2], np.float32(-1))), float(picks[4]), 0.0, -1.0):
        flo, fhi, fw, fcore = ix.linkage_core(k, link)
        e = int(np.count_nonzero(w <= np.float32(link)))
        assert len(flo) == e and same_edges((flo, fhi, fw), (lo[:e], hi[:e], w[:e])), "a finite link is a prefix of the whole tree"
        assert same_bits(fcore, core)
    assert 0 < int(np.count_nonzero(w <= picks[2])) < n - 1
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_equal_a_fresh_index(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    n, dim, k = 300, 100, 4
    rows = np.concatenate([walks(rng, 200, dim, length=50), bursts(rng, 100, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    keep = rng.random(n) < 0.8
    keep[:3] = [False, True, False]
    sel = np.flatnonzero(keep)
    fresh = make_index(clip, clip_lib, rows[sel], dtype)
    flo, fhi, fw, fcore = fresh.linkage_core(k)
    assert same_edges((flo, fhi, fw, fcore), oracle(fresh, k)) and len(flo) == len(sel) - 1
    core = np.full(n, np.inf, dtype=np.float32)
    core[sel] = fcore
    want = (sel[flo], sel[fhi], fw, core)
    for route in (1, 2):
        set_route(clip_lib, ix, route)
        assert same_edges(ix.linkage_core(k, allow=keep), want), route
        assert same_edges(ix.linkage_core(k, allow=sel[::-1]), want), route
    set_route(clip_lib, ix, 0)
    assert same_edges(ix.linkage_core(k, allow=keep), oracle(ix, k, eligible=keep))
    link = float(fw[len(fw) // 2])
    part = fresh.linkage_core(k, link)
    assert 0 < len(part[0]) < len(flo)
    assert same_edges(ix.linkage_core(k, link, allow=keep), (sel[part[0]], sel[part[1]], part[2], core))
    gone = np.flatnonzero(~keep)
    ix.remove(gone[: len(gone) // 2])                # half removed, the other half not allowed
    for route in (1, 2):
        set_route(clip_lib, ix, route)
        assert same_edges(ix.linkage_core(k, allow=keep), want), route
    ix.remove(gone)
    for route in (1, 2, 0):
        set_route(clip_lib, ix, route)
        assert same_edges(ix.linkage_core(k), want), route
    assert same_edges(ix.linkage_core(k), oracle(ix, k))
    new_ids = ix.compact()
    assert np.array_equal(new_ids[sel], np.arange(len(sel)))
    assert same_edges(ix.linkage_core(k), (flo, fhi, fw, fcore))
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism(clip, clip_lib, tmp_path, dtype):
    rng = np.random.default_rng(41)
    n, dim, k = 1000, 100, 7
    rows = np.concatenate([walks(rng, 600, dim), bursts(rng, 400, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    first = ix.linkage_core(k)
    assert len(first[0]) == n - 1
    assert 1 <= ix.linkage_rounds() <= 10            # the round counter covers this call: ceil(log2 1000) rounds are queued
    for _ in range(2):
        assert same_edges(ix.linkage_core(k), first)
    p = str(tmp_path / "l.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_edges(loaded.linkage_core(k), first)
    loaded.close()
    split = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 130), (130, 131), (131, 777), (777, n)):
        split.add(rows[lo:hi])
    for route in (1, 2):
        set_route(clip_lib, split, route)
        assert same_edges(split.linkage_core(k), first), route
    split.close()
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form(clip, clip_lib, dtype):
    import torch
    rng = np.random.default_rng(43)
    n, dim, k = 700, 64, 6
    rows = np.concatenate([walks(rng, 400, dim), bursts(rng, 300, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    allow = np.arange(n) % 5 != 2
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    pad = 64                                         # canaries behind every output

    def run(link, d_allow=None, want_core=True):
        tlo = torch.full((n - 1 + pad,), -7, dtype=torch.int64, device="cuda")
        thi = torch.full((n - 1 + pad,), -7, dtype=torch.int64, device="cuda")
        td = torch.full((n - 1 + pad,), -7, dtype=torch.float32, device="cuda")
        tcore = torch.full((n + pad,), -7, dtype=torch.float32, device="cuda")
        tc = torch.full((1 + pad,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.linkage_core_device(k, tlo.data_ptr(), thi.data_ptr(), td.data_ptr(), tc.data_ptr(), d_core=tcore.data_ptr() if want_core else None,
                               link=link, d_allow=d_allow)
        clip.synchronize()
        return tuple(t.cpu().numpy() for t in (tlo, thi, td, tcore, tc))

    for link, d_allow, host in ((None, None, ix.linkage_core(k)), (CHAIN_RADIUS, None, ix.linkage_core(k, CHAIN_RADIUS)),
                                (None, tw.data_ptr(), ix.linkage_core(k, allow=allow))):
        lo, hi, d, core, count = run(link, d_allow)
        m = int(count[0])
        assert m == len(host[0]) and np.all(count[1:] == -7)
        assert np.all(lo[m:] == -7) and np.all(hi[m:] == -7) and np.all(d[m:] == -7) and np.all(core[n:] == -7)
        order = np.lexsort((hi[:m], lo[:m], d[:m]))
        assert same_edges((lo[:m][order], hi[:m][order], d[:m][order], core[:n]), host)
        again = run(link, d_allow)
        assert all(same_bits(a, b) for a, b in zip((lo, hi, d, core, count), again)), "two runs differ"
        without = run(link, d_allow, want_core=False)                            # d_core may be NULL
        assert all(same_bits(a, b) for a, b in zip((lo, hi, d, count), without[:3] + without[4:])) and np.all(without[3] == -7)
    ix.close()


def test_contract_edges_and_argument_errors(clip, clip_lib, capfd):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ret, lo, hi, w, core = call(clip_lib, ix, 3, np.inf)                     # empty index
    assert ret == 0 and lo[0] == -7 and np.all(core == -7)
    assert all(a.shape == (0,) for a in ix.linkage_core(3))
    rng = np.random.default_rng(3)
    ix.add(rng.standard_normal((1, 32), dtype=np.float32))
    for k, link, c in ((3, -1.0, np.inf), (1, 0.5, np.inf), (3, np.inf, np.inf), (0, np.inf, -np.inf)):     # one row: no edge, its core
        ret, lo, hi, w, core = call(clip_lib, ix, k, link)
        assert ret == 0 and lo[0] == -7 and hi[0] == -7 and w[0] == -7 and core[0] == c and np.all(core[1:] == -7)
    assert call(clip_lib, ix, 3, np.inf, allow=np.zeros(1, dtype=bool))[4][0] == np.inf
    ix.add(rng.standard_normal((199, 32), dtype=np.float32))
    ix.remove([0, 5])
    live = ix.live_mask()
    ret, lo, hi, w, core = call(clip_lib, ix, 3, -1.0)                       # below every weight: no edge, the cores all the same
    assert ret == 0 and np.all(lo == -7) and same_bits(core[:200], oracle(ix, 3)[3])
    ret, lo, hi, w, core = call(clip_lib, ix, 3, np.inf)
    assert ret == 197 and same_edges((lo[:ret], hi[:ret], w[:ret], core[:200]), oracle(ix, 3, eligible=live))
    assert not np.isin([0, 5], np.concatenate([lo[:ret], hi[:ret]])).any() and np.all(lo[ret:] == -7)
    assert core[0] == np.inf and core[5] == np.inf
    only = np.zeros(200, dtype=bool)
    only[[0, 7]] = True                                                      # one eligible row (0 is removed): m <= 1
    ret, lo, hi, w, core = call(clip_lib, ix, 3, np.inf, allow=only)
    assert ret == 0 and np.all(core[:200] == np.inf)
    few = np.zeros(200, dtype=bool)
    few[[3, 9, 11]] = True                                                   # three eligible rows, k = 3: +inf weights, ordered by (lo, hi)
    ret, lo, hi, w, core = call(clip_lib, ix, 3, np.inf, allow=few)
    assert ret == 2 and lo[:2].tolist() == [3, 3] and hi[:2].tolist() == [9, 11] and np.all(w[:2] == np.inf)
    assert call(clip_lib, ix, 3, 3.0e38, allow=few)[0] == 0                  # in the graph only at link = inf
    # refused before any launch: outputs untouched
    capfd.readouterr()
    for k, link in ((3, float("nan")), (-1, 0.5), (1025, 0.5)):
        ret, lo, hi, w, core = call(clip_lib, ix, k, link)
        assert ret == -1 and np.all(lo == -7) and np.all(hi == -7) and np.all(w == -7) and np.all(core == -7)
    lp, hp, wp, cp = lo.ctypes.data_as(I64P), hi.ctypes.data_as(I64P), w.ctypes.data_as(F32P), core.ctypes.data_as(F32P)
    assert L.clip_amd_index_linkage_core(ix.handle, 3, 0.5, None, None, hp, wp, cp) == -1
    assert L.clip_amd_index_linkage_core(ix.handle, 3, 0.5, None, lp, None, wp, cp) == -1
    assert L.clip_amd_index_linkage_core(ix.handle, 3, 0.5, None, lp, hp, None, cp) == -1
    assert L.clip_amd_index_linkage_core(None, 3, 0.5, None, lp, hp, wp, cp) == -1
    err = capfd.readouterr().err
    assert "link is NaN" in err and err.count("NULL result pointer") == 3 and "index is NULL" in err
    assert "k = -1 outside 0 ... 1024" in err and "k = 1025 outside 0 ... 1024" in err
    assert np.all(lo == -7) and np.all(hi == -7) and np.all(w == -7) and np.all(core == -7)
    import torch
    t = torch.full((5, 256), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = [t[r].data_ptr() for r in range(5)]
    for bad in ((0, ptr[1], ptr[2], ptr[3]), (ptr[0], 0, ptr[2], ptr[3]), (ptr[0], ptr[1], 0, ptr[3]), (ptr[0], ptr[1], ptr[2], 0)):
        with pytest.raises(RuntimeError):
            ix.linkage_core_device(3, *bad, d_core=ptr[4])
    for k, link in ((3, float("nan")), (-1, 0.5), (1025, 0.5)):
        assert L.clip_amd_index_linkage_core_device(ix.handle, k, link, None, ptr[0], ptr[1], ptr[2], ptr[4], ptr[3]) is False
    assert L.clip_amd_index_linkage_core_device(None, 3, 0.5, None, ptr[0], ptr[1], ptr[2], ptr[4], ptr[3]) is False
    clip.synchronize()
    assert bool((t == -7).all())
    with pytest.raises(ValueError):
        ix.linkage_core(3, float("nan"))
    with pytest.raises(ValueError):
        ix.linkage_core(1025)
    ix.close()
