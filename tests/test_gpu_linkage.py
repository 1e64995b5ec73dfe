"""GPU tier of the single-linkage tree (k_linkage.hip, clip_amd_index_linkage).  The oracle is Kruskal's algorithm (tests/linkage_common.py)
over the library's own pair list: `Index.pairs(radius=4)` reports every pair with the bits of the same score chain, so the tree must come
out byte for byte: every comparison here is for equality.  Data: walks (deep trees, many rounds), bursts with exact copies (zero and equal
distances), planted near-duplicates; all ties (one-hot rows); consistency with `components`; masks (remove, allow, compact);
determinism (calls, add splits, save / load); the device form; argument errors."""
import ctypes as C

import numpy as np
import pytest

from linkage_common import CHAIN_RADIUS, bursts, kruskal, labels_of, planted, same_bits, walks

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)
U64P = C.POINTER(C.c_uint64)
DTYPES = ("f16", "f32", "i8")
KINDS = {"walks": walks, "bursts": bursts, "planted": planted}


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


def all_pairs(ix):
    """every pair of the index with its distance: the oracle's input (no distance of unit vectors exceeds 2)"""
    i, j, d = ix.pairs(4.0)
    assert len(i) == len(ix) * (len(ix) - 1) // 2 - removed_pairs(ix)
    return i, j, d


def removed_pairs(ix):
    live = int(ix.live_mask().sum())
    n = len(ix)
    return n * (n - 1) // 2 - live * (live - 1) // 2


def oracle(ix, link=np.inf, eligible=None):
    i, j, d = all_pairs(ix)
    if eligible is not None:
        use = eligible[i] & eligible[j]
        i, j, d = i[use], j[use], d[use]
    return kruskal(len(ix), i, j, d, link)


def same_edges(got, want):
    return all(same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b)) for a, b in zip(got, want))


def call(clip_lib, ix, link, allow=None):
    """clip_amd_index_linkage itself over poisoned outputs: (return value, lo, hi, distances)"""
    n = len(ix)
    words = None if allow is None else clip_lib.allow_words(allow, n)
    lo = np.full(max(n - 1, 1), -7, dtype=np.int64)
    hi = np.full(max(n - 1, 1), -7, dtype=np.int64)
    dist = np.full(max(n - 1, 1), -7, dtype=np.float32)
    ret = clip_lib.lib().clip_amd_index_linkage(ix.handle, float(link), None if words is None else words.ctypes.data_as(U64P),
                                                lo.ctypes.data_as(I64P), hi.ctypes.data_as(I64P), dist.ctypes.data_as(F32P))
    return ret, lo, hi, dist


@pytest.mark.parametrize("dim", (32, 100, 512))
@pytest.mark.parametrize("n", (1, 2, 3, 127, 128, 129, 300, 1100))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_equals_kruskal_over_the_index_s_own_pairs(clip, clip_lib, kind, dtype, n, dim):
    rng = np.random.default_rng(1000 * dim + n + len(kind))
    rows = KINDS[kind](rng, n, dim)
    ix = make_index(clip, clip_lib, rows, dtype)
    want = oracle(ix)
    assert len(want[0]) == n - 1
    got = ix.linkage()
    assert same_edges(got, want), "the tree differs from Kruskal over the index's pairs"
    ret, lo, hi, dist = call(clip_lib, ix, np.inf)
    assert ret == n - 1 and same_edges((lo[:ret], hi[:ret], dist[:ret]), want)
    assert np.all(lo[ret:] == -7) and np.all(hi[ret:] == -7) and np.all(dist[ret:] == -7)
    if kind == "bursts" and n >= 127:
        assert np.count_nonzero(np.diff(want[2]) == 0) >= 10         # equal distances: the tie-break decided edges
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("doubled", (False, True))
def test_all_ties(clip, clip_lib, dtype, doubled):
    """200 one-hot rows: every distance is exactly 1, the tree is the star of row 0; doubled: every row twice, distance 0 inside a pair"""
    rows = np.eye(200, 256, dtype=np.float32)
    if doubled:
        rows = np.repeat(rows, 2, axis=0)
    n = len(rows)
    ix = make_index(clip, clip_lib, rows, dtype)
    lo, hi, d = ix.linkage()
    assert same_edges((lo, hi, d), oracle(ix))
    if not doubled:
        assert np.all(lo == 0) and np.array_equal(hi, np.arange(1, n)) and np.all(d == 1.0)
    else:
        assert np.array_equal(lo[:200], np.arange(0, n, 2)) and np.array_equal(hi[:200], np.arange(1, n, 2))
        assert np.all(d[:200] == d[0]) and abs(float(d[0])) <= 2.0 ** -22       # (i8: 1 - 127 * 127 / 127 / 127 in f32 need not be 0)
        assert np.all(lo[200:] == 0) and np.array_equal(hi[200:], np.arange(2, n, 2)) and np.all(d[200:] == 1.0)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_consistent_with_components(clip, clip_lib, dtype):
    rng = np.random.default_rng(61)
    n, dim = 600, 100
    rows = np.concatenate([walks(rng, 400, dim), bursts(rng, 200, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    lo, hi, d = ix.linkage()
    assert len(lo) == n - 1
    merges = np.unique(d)
    picks = merges[np.linspace(0, len(merges) - 1, 12).astype(int)]
    radii = []
    for m in picks:
        radii += [m, np.nextafter(m, np.float32(-1))]
    radii += [(a + b) / np.float32(2) for a, b in zip(picks[:-1], picks[1:])] + [np.float32(-1), np.float32(4)]
    for radius in radii:
        labels, _, _ = ix.components(float(radius))
        assert np.array_equal(clip_lib.cut_linkage(n, lo, hi, d, radius=float(radius)), labels), radius
    for link in (CHAIN_RADIUS, float(picks[3]), float(np.nextafter(picks[3], np.float32(-1))), 0.0, -1.0):
        labels, _, _ = ix.components(link)
        c = len(np.unique(labels))
        flo, fhi, fd = ix.linkage(link)
        assert len(flo) == n - c
        assert same_edges((flo, fhi, fd), (lo[:n - c], hi[:n - c], d[:n - c])), "a finite link is a prefix of the whole tree"
        assert np.array_equal(clip_lib.cut_linkage(n, flo, fhi, fd), labels)
    for groups in (1, 2, 17, n - 1, n):
        labels = clip_lib.cut_linkage(n, lo, hi, d, n_groups=groups)
        assert len(np.unique(labels)) == groups
        assert np.array_equal(labels, labels_of(n, lo[:n - groups], hi[:n - groups]))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_equal_a_fresh_index(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    n, dim = 300, 100
    rows = np.concatenate([walks(rng, 200, dim, length=50), bursts(rng, 100, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    keep = rng.random(n) < 0.8
    keep[:3] = [False, True, False]
    sel = np.flatnonzero(keep)
    fresh = make_index(clip, clip_lib, rows[sel], dtype)
    flo, fhi, fd = fresh.linkage()
    assert same_edges((flo, fhi, fd), oracle(fresh)) and len(flo) == len(sel) - 1
    want = (sel[flo], sel[fhi], fd)
    assert same_edges(ix.linkage(allow=keep), want)
    assert same_edges(ix.linkage(allow=sel[::-1]), want)
    assert same_edges(ix.linkage(allow=keep), oracle(ix, eligible=keep))
    link = float(fd[len(fd) // 2])
    part = fresh.linkage(link)
    assert 0 < len(part[0]) < len(flo)
    assert same_edges(ix.linkage(link, allow=keep), (sel[part[0]], sel[part[1]], part[2]))
    gone = np.flatnonzero(~keep)
    ix.remove(gone[: len(gone) // 2])                # half removed, the other half not allowed
    assert same_edges(ix.linkage(allow=keep), want)
    ix.remove(gone)
    assert same_edges(ix.linkage(), want)
    assert same_edges(ix.linkage(), oracle(ix))
    labels = clip_lib.cut_linkage(n, *ix.linkage(), radius=CHAIN_RADIUS, eligible=ix.live_mask())
    assert np.array_equal(labels, ix.components(CHAIN_RADIUS)[0])
    new_ids = ix.compact()
    assert np.array_equal(new_ids[sel], np.arange(len(sel)))
    assert same_edges(ix.linkage(), (flo, fhi, fd))
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism(clip, clip_lib, tmp_path, dtype):
    rng = np.random.default_rng(41)
    n, dim = 1000, 100
    rows = np.concatenate([walks(rng, 600, dim), bursts(rng, 400, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    first = ix.linkage()
    assert len(first[0]) == n - 1
    for _ in range(2):
        assert same_edges(ix.linkage(), first)
    p = str(tmp_path / "l.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_edges(loaded.linkage(), first)
    loaded.close()
    split = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 130), (130, 131), (131, 777), (777, n)):
        split.add(rows[lo:hi])
    assert same_edges(split.linkage(), first)
    split.close()
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form(clip, clip_lib, dtype):
    import torch
    rng = np.random.default_rng(43)
    n, dim = 700, 64
    rows = np.concatenate([walks(rng, 400, dim), bursts(rng, 300, dim)])
    ix = make_index(clip, clip_lib, rows, dtype)
    allow = np.arange(n) % 5 != 2
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    pad = 64                                         # canaries behind every output

    def run(link, d_allow=None):
        tlo = torch.full((n - 1 + pad,), -7, dtype=torch.int64, device="cuda")
        thi = torch.full((n - 1 + pad,), -7, dtype=torch.int64, device="cuda")
        td = torch.full((n - 1 + pad,), -7, dtype=torch.float32, device="cuda")
        tc = torch.full((1 + pad,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.linkage_device(tlo.data_ptr(), thi.data_ptr(), td.data_ptr(), tc.data_ptr(), link=link, d_allow=d_allow)
        clip.synchronize()
        return tuple(t.cpu().numpy() for t in (tlo, thi, td, tc))

    for link, d_allow, host in ((None, None, ix.linkage()), (CHAIN_RADIUS, None, ix.linkage(CHAIN_RADIUS)),
                                (None, tw.data_ptr(), ix.linkage(allow=allow))):
        lo, hi, d, count = run(link, d_allow)
        m = int(count[0])
        assert m == len(host[0]) and np.all(count[1:] == -7)
        assert np.all(lo[m:] == -7) and np.all(hi[m:] == -7) and np.all(d[m:] == -7)
        order = np.lexsort((hi[:m], lo[:m], d[:m]))
        assert same_edges((lo[:m][order], hi[:m][order], d[:m][order]), host)
        again = run(link, d_allow)
        assert all(same_bits(a, b) for a, b in zip((lo, hi, d, count), again)), "two runs differ"
    ix.close()


def test_contract_edges_and_argument_errors(clip, clip_lib, capfd):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ret, lo, hi, dist = call(clip_lib, ix, np.inf)                           # empty index
    assert ret == 0 and lo[0] == -7
    assert all(a.shape == (0,) for a in ix.linkage())
    rng = np.random.default_rng(3)
    ix.add(rng.standard_normal((1, 32), dtype=np.float32))
    for link in (-1.0, 0.5, np.inf):                                         # one row: no edge
        ret, lo, hi, dist = call(clip_lib, ix, link)
        assert ret == 0 and lo[0] == -7 and hi[0] == -7 and dist[0] == -7
    ix.add(rng.standard_normal((199, 32), dtype=np.float32))
    ix.remove([0, 5])
    live = ix.live_mask()
    ret, lo, hi, dist = call(clip_lib, ix, -1.0)                             # below every distance: no edge
    assert ret == 0 and np.all(lo == -7)
    ret, lo, hi, dist = call(clip_lib, ix, np.inf)
    assert ret == 197 and same_edges((lo[:ret], hi[:ret], dist[:ret]), oracle(ix, eligible=live))
    assert not np.isin([0, 5], np.concatenate([lo[:ret], hi[:ret]])).any() and np.all(lo[ret:] == -7)
    only = np.zeros(200, dtype=bool)
    only[[0, 7]] = True                                                      # one eligible row (0 is removed): m <= 1
    assert call(clip_lib, ix, np.inf, allow=only)[0] == 0
    # refused before any launch: outputs untouched
    capfd.readouterr()
    ret, lo, hi, dist = call(clip_lib, ix, float("nan"))
    assert ret == -1 and np.all(lo == -7) and np.all(hi == -7) and np.all(dist == -7)
    lp, hp, dp = lo.ctypes.data_as(I64P), hi.ctypes.data_as(I64P), dist.ctypes.data_as(F32P)
    assert L.clip_amd_index_linkage(ix.handle, 0.5, None, None, hp, dp) == -1
    assert L.clip_amd_index_linkage(ix.handle, 0.5, None, lp, None, dp) == -1
    assert L.clip_amd_index_linkage(ix.handle, 0.5, None, lp, hp, None) == -1
    assert L.clip_amd_index_linkage(None, 0.5, None, lp, hp, dp) == -1
    err = capfd.readouterr().err
    assert "link is NaN" in err and err.count("NULL result pointer") == 3 and "index is NULL" in err
    assert np.all(lo == -7) and np.all(hi == -7) and np.all(dist == -7)
    import torch
    t = torch.full((4, 256), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = [t[r].data_ptr() for r in range(4)]
    for bad in ((0, ptr[1], ptr[2], ptr[3]), (ptr[0], 0, ptr[2], ptr[3]), (ptr[0], ptr[1], 0, ptr[3]), (ptr[0], ptr[1], ptr[2], 0)):
        with pytest.raises(RuntimeError):
            ix.linkage_device(*bad)
    assert L.clip_amd_index_linkage_device(ix.handle, float("nan"), None, ptr[0], ptr[1], ptr[2], ptr[3]) is False
    assert L.clip_amd_index_linkage_device(None, 0.5, None, ptr[0], ptr[1], ptr[2], ptr[3]) is False
    clip.synchronize()
    assert bool((t == -7).all())
    with pytest.raises(ValueError):
        ix.linkage(float("nan"))
    ix.close()
