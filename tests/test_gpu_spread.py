"""GPU tier of farthest-first selection (k_spread.hip, clip_amd_index_spread).  The oracle is the library's own pair list: `Index.pairs(4.0)`
of the same index holds the distance of every pair of live rows, from the same score chain, so the contract in numpy over the dense matrix
of those pairs (tests/spread_common.py: spread_contract) must give exactly the centres, their order, the owners and the bits of every
reach and owner distance: every comparison here is for equality.  The traversal is chaotic (one differing bit changes every later pick),
so the main grid runs it to the end: n_max = n pins every step.  For masked cases the oracle is an index that holds only the eligible
rows, ids mapped back.  One case per dtype is also checked against float64 distances of the stored values, and one larger case by those
properties alone.  Data: bursts of exact and noisy copies (ties in the gap, decided by id, and in the owner, decided by position),
planted near-duplicates among random rows, random walks on the sphere."""
import ctypes as C
import itertools
import struct

import numpy as np
import pytest

from spread_common import bursts, matrix_from_pairs, planted, same_bits, spread_contract, walks

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)
U64P = C.POINTER(C.c_uint64)
DTYPES = ("f16", "f32", "i8")
INF = float("inf")
GENERATORS = {"bursts": bursts, "planted": planted, "walks": walks}


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


def call(clip_lib, ix, n_max, stop=-INF, seeds=None, allow=None, want=(True, True, True, True), centres=True):
    """clip_amd_index_spread itself on sentinel-filled outputs: (return value, centres [n_max], reach or None, owner or None, owner distance
    or None, cover radius or None)"""
    n = len(ix)
    words = None if allow is None else clip_lib.allow_words(allow, n)
    s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int64)
    size = max(int(n_max), 0)
    c = np.full(size, -7, dtype=np.int64)
    reach = np.full(size, -7, dtype=np.float32) if want[0] else None
    owner = np.full(n, -7, dtype=np.int64) if want[1] else None
    dist = np.full(n, -7, dtype=np.float32) if want[2] else None
    cover = np.full(1, -7, dtype=np.float32) if want[3] else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    ret = clip_lib.lib().clip_amd_index_spread(ix.handle, int(n_max), float(stop), ptr(s, I64P), 0 if s is None else len(s), ptr(words, U64P),
                                               ptr(c, I64P) if centres else None, ptr(reach, F32P), ptr(owner, I64P), ptr(dist, F32P), ptr(cover, F32P))
    return ret, c, reach, owner, dist, cover


def untouched(res):
    return all(a is None or np.all(a == -7) for a in res[1:])


def same_result(got, want):
    """(centres, reach, owner, owner distance, cover radius) twice: equal, the distances as bits"""
    return len(got) == len(want) == 5 and all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(got[:4], want[:4])) and \
        same_bits(np.float32(got[4]), np.float32(want[4]))


def matrix_of(ix):
    """the oracle's matrix: every pair of live rows of the index, as the library's own pairs report them"""
    n = len(ix)
    i, j, d = ix.pairs(4.0)
    assert len(i) == ix.live * (ix.live - 1) // 2
    return matrix_from_pairs(n, i, j, d)


def check(clip_lib, ix, D, n_max, stop=-INF, seeds=(), eligible=None, allow=None, picks_by_id=None):
    """the call against the contract over D; returns the contract's five outputs"""
    want = spread_contract(D, n_max, stop, seeds, eligible, picks_by_id)
    ret, c, reach, owner, dist, cover = call(clip_lib, ix, n_max, stop, list(seeds) if len(seeds) else None, allow)
    m = len(want[0])
    assert ret == m
    assert np.array_equal(c[:m], want[0]), "centres differ from the contract over pairs"
    assert np.all(c[m:] == -1) and np.all(np.isinf(reach[m:])) and np.all(reach[m:] > 0)
    assert same_bits(reach[:m], want[1]), "reaches differ from the pairs' as bits"
    assert np.array_equal(owner, want[2])
    assert same_bits(dist, want[3]), "owner distances differ from the pairs' as bits"
    assert same_bits(cover[0], want[4])
    return want


@pytest.mark.parametrize("dim", (40, 512))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 127, 128, 129, 1025, 2100))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("bursts", "planted", "walks"))
def test_equals_contract_over_pairs(clip, clip_lib, kind, dtype, n, dim):
    rng = np.random.default_rng(1000 * dim + n + len(kind))
    ix = make_index(clip, clip_lib, GENERATORS[kind](rng, n, dim), dtype)
    D = matrix_of(ix)
    by_id = []
    c, reach, owner, dist, cover = check(clip_lib, ix, D, n, picks_by_id=by_id)                 # the whole permutation
    assert sorted(c.tolist()) == list(range(n)) and cover == 0 and np.array_equal(owner, np.arange(n)) and np.all(dist == 0)
    assert np.isinf(reach[0]) and np.all(np.diff(reach[1:]) <= 0)                                # non-increasing from the first finite entry
    pc, preach, powner, pdist, pcover = check(clip_lib, ix, D, 7)                                # a prefix
    m = min(7, n)
    assert np.array_equal(pc, c[:m]) and same_bits(preach, reach[:m])
    if n > 7:
        assert same_bits(pcover, reach[7])           # the coverage radius of a prefix is the reach of the next pick
        assert np.all(np.isin(powner, pc)) and np.bincount(powner).max() >= 2
    if kind == "bursts" and n >= 127:                # not trivial: picks decided by id among equal gaps
        assert sum(by_id) >= 20
    ix.close()


@pytest.mark.parametrize("n_seeds", (1, 16, 17, 40))
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeds(clip, clip_lib, dtype, n_seeds):
    """one sweep, exactly one full sweep, several sweeps of the 16-column seed pass; exact copies among the seeds, so that the order of
    the seeds decides who owns the rows near them"""
    rng = np.random.default_rng(300 + n_seeds)
    n, dim = 300, 40
    rows = bursts(rng, n, dim)
    _, inverse, counts = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    group = int(np.flatnonzero(counts >= 3)[0])
    copies = np.flatnonzero(inverse == group)[:3]                                               # three exact copies, ids ascending
    ix = make_index(clip, clip_lib, rows, dtype)
    D = matrix_of(ix)
    others = rng.permutation(np.setdiff1d(np.arange(n), copies))
    if n_seeds == 1:
        seeds = [int(copies[1])]
    else:                                            # the HIGHEST copy first, the lowest one 15 or more positions later: another sweep
        seeds = [int(copies[2])] + others[:n_seeds - 2].tolist() + [int(copies[0])]
    for n_max in (n_seeds, n_seeds + 30):
        c, reach, owner, dist, cover = check(clip_lib, ix, D, n_max, seeds=seeds)
        assert c[:n_seeds].tolist() == seeds and np.all(np.isinf(reach[:n_seeds])) and np.all(np.isfinite(reach[n_seeds:]))
        free = [int(x) for x in copies if x not in seeds]
        assert free and all(owner[x] == seeds[0] for x in free)                                 # the copy given first owns the free copies
        if n_max == n_seeds:                         # pure nearest-seed assignment
            rest = np.setdiff1d(np.arange(n), seeds)
            assert np.array_equal(dist[rest], D[seeds][:, rest].min(0))
    if n_seeds > 1:                                  # the same seeds in another order: the other copy owns them
        back = seeds[::-1]
        c, reach, owner, dist, cover = check(clip_lib, ix, D, n_seeds, seeds=back)
        assert all(owner[x] == back[0] for x in free)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_stop_radius(clip, clip_lib, dtype):
    rng = np.random.default_rng(19)
    n, dim = 400, 40
    ix = make_index(clip, clip_lib, walks(rng, n, dim), dtype)
    D = matrix_of(ix)
    full = spread_contract(D, n)
    reach = full[1].astype(np.float64)
    steps = np.flatnonzero((reach[1:-1] - reach[2:]) > 1e-4) + 1                                # t: a clear gap between reach[t] and reach[t + 1]
    assert len(steps) >= 10
    for t in (steps[0], steps[len(steps) // 2], steps[-1]):
        stop = float(np.float32((reach[t] + reach[t + 1]) / 2))
        assert reach[t + 1] < stop < reach[t]
        got = check(clip_lib, ix, D, n, stop=stop)
        assert len(got[0]) == t + 1 and np.array_equal(got[0], full[0][:t + 1]) and got[4] <= np.float32(stop)
        assert len(check(clip_lib, ix, D, t, stop=stop)[0]) == t                                # n_max ends it first
    seeds = [7, 3, 200]
    for s, want in (((), [0]), (seeds, seeds)):      # above every distance: the seeds, or the one first row
        got = check(clip_lib, ix, D, n, stop=4.0, seeds=s)
        assert got[0].tolist() == want
        assert check(clip_lib, ix, D, n, stop=INF, seeds=s)[0].tolist() == want
    a = ix.spread(50, None)
    b = ix.spread(50, -INF)
    assert same_result(a, b) and same_result(a, check(clip_lib, ix, D, 50))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_allow_and_compact_equal_a_fresh_index(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    n, dim = 400, 40
    rows = np.concatenate([walks(rng, 250, dim, length=50), bursts(rng, 150, dim)])[rng.permutation(n)]
    ix = make_index(clip, clip_lib, rows, dtype)
    keep = rng.random(n) < 0.8
    keep[:3] = [False, True, False]
    keep[32:64] = False                              # a whole mask word, and with it two whole 16-row tiles
    sel = np.flatnonzero(keep)
    fresh = make_index(clip, clip_lib, rows[sel], dtype)
    Df = matrix_of(fresh)
    seeds_f = [5, 0, 77]
    cases = [(len(sel), -INF, ()), (9, -INF, ()), (40, -INF, seeds_f), (len(sel), 0.03, ()), (len(sel) + 50, -INF, ())]
    want = {t: check(clip_lib, fresh, Df, *case) for t, case in enumerate(cases)}
    whole = ix.spread(9)
    assert not np.array_equal(whole[0], sel[want[1][0]])                                        # (the rows left out were picked: the mask matters)

    def mapped(t, got):
        """a result over all ids against the fresh index's, ids mapped back"""
        fc, fr, fo, fd, fcover = want[t]
        centres, reach, owner, dist, cover = got
        assert np.array_equal(centres, sel[fc]) and same_bits(reach, fr)
        assert np.all(owner[~keep] == -1) and np.all(np.isinf(dist[~keep]))
        assert np.array_equal(owner[sel], sel[fo]) and same_bits(dist[sel], fd) and same_bits(np.float32(cover), np.float32(fcover))

    def run(allow):
        for t, (n_max, stop, seeds) in enumerate(cases):
            mapped(t, ix.spread(n_max, None if stop == -INF else stop, sel[list(seeds)] if len(seeds) else None, allow=allow))

    run(keep)                                        # allow as a mask
    run(sel[::-1])                                   # allow as ids
    gone = np.flatnonzero(~keep)
    ix.remove(gone[: len(gone) // 2])                # half removed, the other half not allowed
    run(keep)
    ix.remove(gone)
    run(None)                                        # remove alone
    D = matrix_of(ix)                                # (pairs lists the live rows only)
    check(clip_lib, ix, D, 40, seeds=sel[seeds_f].tolist(), eligible=keep)
    new_ids = ix.compact()
    assert np.array_equal(new_ids[sel], np.arange(len(sel)))
    for t, (n_max, stop, seeds) in enumerate(cases):
        assert same_result(ix.spread(n_max, None if stop == -INF else stop, list(seeds) or None), want[t])
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism(clip, clip_lib, tmp_path, dtype):
    import torch
    rng = np.random.default_rng(41)
    n, dim = 1000, 100
    rows = np.concatenate([walks(rng, 600, dim), bursts(rng, 400, dim)])
    n_max, seeds = 300, [999, 0, 500]
    ix = make_index(clip, clip_lib, rows, dtype)
    first = ix.spread(n_max, seeds=seeds)
    assert len(first[0]) == n_max and first[4] > 0 and np.bincount(first[2]).max() >= 5
    for _ in range(2):
        assert same_result(ix.spread(n_max, seeds=seeds), first)
    p = str(tmp_path / "s.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_result(loaded.spread(n_max, seeds=seeds), first)
    loaded.close()
    split = clip_lib.Index(clip, dim, dtype)
    for lo, hi in ((0, 1), (1, 130), (130, 131), (131, 777), (777, n)):
        split.add(rows[lo:hi])
    assert same_result(split.spread(n_max, seeds=seeds), first)
    split.close()
    tc = torch.full((n_max,), -7, dtype=torch.int64, device="cuda")
    tr = torch.full((n_max,), -7, dtype=torch.float32, device="cuda")
    to = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    td = torch.full((n,), -7, dtype=torch.float32, device="cuda")
    tv = torch.full((1,), -7, dtype=torch.float32, device="cuda")
    tm = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.spread_device(n_max, tc.data_ptr(), None, seeds, tr.data_ptr(), to.data_ptr(), td.data_ptr(), tv.data_ptr(), tm.data_ptr())
    clip.synchronize()
    assert int(tm.item()) == n_max
    assert same_result((tc.cpu().numpy(), tr.cpu().numpy(), to.cpu().numpy(), td.cpu().numpy(), tv.cpu().numpy()[0]), first)
    # a stop radius met mid-way: every step is queued and the ones after the end write nothing
    t = 100 + int(np.flatnonzero(first[1][100:-1] - first[1][101:] > 1e-5)[0])                 # a clear step of the reach sequence
    stop = float(np.float32((float(first[1][t]) + float(first[1][t + 1])) / 2))
    assert first[1][t + 1] < stop < first[1][t]
    want = ix.spread(n_max, stop, seeds)
    m = t + 1
    assert len(want[0]) == m
    ix.spread_device(n_max, tc.data_ptr(), stop, seeds, tr.data_ptr(), to.data_ptr(), td.data_ptr(), tv.data_ptr(), tm.data_ptr())
    clip.synchronize()
    assert int(tm.item()) == m and np.all(tc.cpu().numpy()[m:] == -1) and np.all(np.isinf(tr.cpu().numpy()[m:]))
    assert same_result((tc.cpu().numpy()[:m], tr.cpu().numpy()[:m], to.cpu().numpy(), td.cpu().numpy(), tv.cpu().numpy()[0]), want)
    # centres only, over a subset: the NULL outputs are not written
    allow = np.arange(n) % 5 != 2
    tw = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64).copy()).cuda()
    tc.fill_(-7)
    torch.cuda.synchronize()
    ix.spread_device(n_max, tc.data_ptr(), seeds=[999, 0], d_allow=tw.data_ptr())
    clip.synchronize()
    assert np.array_equal(tc.cpu().numpy(), ix.spread(n_max, seeds=[999, 0], allow=allow)[0])
    assert same_bits(tr.cpu().numpy()[:m], want[1]) and same_bits(to.cpu().numpy(), want[2]) and same_bits(td.cpu().numpy(), want[3])
    assert int(tm.item()) == m
    with pytest.raises(RuntimeError):                # a seed that is not allowed: refused, nothing written
        ix.spread_device(n_max, tc.data_ptr(), seeds=[2], d_allow=tw.data_ptr())
    clip.synchronize()
    assert np.array_equal(tc.cpu().numpy(), ix.spread(n_max, seeds=[999, 0], allow=allow)[0])
    ix.close()


def float64_properties(ix, d64, tol, n_max, result):
    """what the traversal must satisfy whatever the f32 bits: every pick is, within 2 tol, the farthest row of its step, and every owner
    distance is, within tol, the float64 minimum over the centres"""
    centres, reach, owner, dist, cover = result
    n = len(d64)
    assert len(centres) == n_max and len(set(centres.tolist())) == n_max
    gap = d64[centres[0]].copy()
    chosen = np.zeros(n, dtype=bool)
    chosen[centres[0]] = True
    for t in range(1, n_max):
        x = centres[t]
        assert not chosen[x]
        assert gap[x] >= np.where(chosen, -np.inf, gap).max() - 2 * tol, "step %d picked a row that is not the farthest" % t
        assert abs(gap[x] - float(reach[t])) <= tol
        chosen[x] = True
        gap = np.minimum(gap, d64[x])
    rest = ~chosen
    assert np.all(np.abs(gap[rest] - dist[rest].astype(np.float64)) <= tol) and np.all(dist[chosen] == 0)
    assert np.all(np.abs(d64[owner[rest], np.flatnonzero(rest)] - gap[rest]) <= 2 * tol) and np.array_equal(owner[chosen], np.flatnonzero(chosen))
    assert abs(float(cover) - (gap[rest].max() if rest.any() else 0.0)) <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_float64_distances(clip, clip_lib, tmp_path, dtype):
    n, dim = 300, 100
    ix = make_index(clip, clip_lib, walks(np.random.default_rng(77), n, dim), dtype)
    r64 = stored64(ix, tmp_path)
    d64 = 1.0 - r64 @ r64.T
    for n_max in (n, 60):
        float64_properties(ix, d64, tol_of(dim), n_max, ix.spread(n_max))
    ix.close()


def test_contract_edges(clip, clip_lib):
    L = clip_lib.lib()
    ix = clip_lib.Index(clip, 32, "f16")
    ret, c, reach, owner, dist, cover = call(clip_lib, ix, 3)                                   # empty index
    assert ret == 0 and c.tolist() == [-1] * 3 and np.all(np.isinf(reach)) and owner.size == 0 and cover[0] == 0
    got = ix.spread(3)
    assert all(a.shape == (0,) for a in got[:4]) and got[4] == 0
    assert untouched(call(clip_lib, ix, 3, seeds=[0])) and call(clip_lib, ix, 3, seeds=[0])[0] == -1
    rng = np.random.default_rng(3)
    ix.add(rng.standard_normal((1, 32), dtype=np.float32))
    for n_max, stop in ((1, -INF), (5, -INF), (5, 0.5), (5, INF)):                              # one row
        ret, c, reach, owner, dist, cover = call(clip_lib, ix, n_max, stop)
        assert ret == 1 and c.tolist() == [0] + [-1] * (n_max - 1) and np.all(np.isinf(reach)) and owner.tolist() == [0] and dist.tolist() == [0.0] and cover[0] == 0
    ix.add(rng.standard_normal((199, 32), dtype=np.float32))
    ix.remove([0, 5])
    n = 200
    D = matrix_of(ix)
    live = ix.live_mask()
    check(clip_lib, ix, D, 1000, eligible=live)                                                 # n_max beyond the eligible count
    allow = np.arange(n) % 3 != 1
    want = call(clip_lib, ix, 20, seeds=[9, 3], allow=allow)
    assert want[0] == 20
    check(clip_lib, ix, D, 20, seeds=[9, 3], eligible=live & allow, allow=allow)
    for mask in itertools.product((False, True), repeat=4):                                     # NULL optional outputs in every combination
        got = call(clip_lib, ix, 20, seeds=[9, 3], allow=allow, want=mask)
        assert got[0] == 20 and np.array_equal(got[1], want[1])
        assert all(g is None or same_bits(g, w) for g, w in zip(got[2:], want[2:]))
        assert [g is None for g in got[2:]] == [not m for m in mask]
    none = np.zeros(n, dtype=bool)
    ret, c, reach, owner, dist, cover = call(clip_lib, ix, 4, allow=none)                       # no eligible row
    assert ret == 0 and np.all(c == -1) and np.all(np.isinf(reach)) and np.all(owner == -1) and np.all(np.isinf(dist)) and cover[0] == 0
    # refused before any launch: outputs untouched
    refusals = [dict(n_max=5, stop=float("nan")), dict(n_max=0), dict(n_max=-3), dict(n_max=1, seeds=[1, 2]),
                dict(n_max=5, seeds=[0]), dict(n_max=5, seeds=[2, 5]),                          # removed
                dict(n_max=5, seeds=[2, 4], allow=allow),                                       # not allowed
                dict(n_max=5, seeds=[200]), dict(n_max=5, seeds=[-1]), dict(n_max=5, seeds=[2, 3, 2])]
    for kw in refusals:
        res = call(clip_lib, ix, **kw)
        assert res[0] == -1 and untouched(res), kw
    res = call(clip_lib, ix, 5, centres=False)
    assert res[0] == -1 and untouched(res)
    assert call(clip_lib, ix, 5, seeds=[2, 3], allow=allow)[0] == 5                             # (the well-formed neighbour of the refusals goes through)
    for kw in (dict(n=3, radius=float("nan")), dict(n=0), dict(n=1, seeds=[1, 2]), dict(n=5, seeds=[0]), dict(n=5, seeds=[2, 4], allow=allow),
               dict(n=5, seeds=[200]), dict(n=5, seeds=[2, 2])):
        with pytest.raises(ValueError):
            ix.spread(**kw)
    with pytest.raises(RuntimeError):
        ix.spread_device(3, None)
    with pytest.raises(RuntimeError):
        ix.spread_device(5, 1, seeds=[0])                                                       # removed: the library's to find
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_copies_and_zero_vectors(clip, clip_lib, dtype):
    rng = np.random.default_rng(5)
    n, dim = 70, 40
    rows = np.repeat(rng.standard_normal((1, dim), dtype=np.float32), n, axis=0)
    ix = make_index(clip, clip_lib, rows, dtype)
    c, reach, owner, dist, cover = check(clip_lib, ix, matrix_of(ix), n)
    assert c.tolist() == list(range(n))              # all equal: picked in id order
    assert len(set(reach[1:].tobytes()[4 * t:4 * t + 4] for t in range(n - 1))) == 1 and abs(float(reach[1])) < 1e-3
    c, reach, owner, dist, cover = ix.spread(1)
    assert np.all(owner == 0) and dist[0] == 0 and len(set(dist[1:].tolist())) == 1 and cover == max(dist[1], 0)      # (the centre's own 0 counts)
    ix.close()
    if dtype == "i8":                                # zero vectors: distance exactly 1 to everything, each other included
        rows = rng.standard_normal((40, dim), dtype=np.float32)
        rows[[3, 17, 30]] = 0
        ix = make_index(clip, clip_lib, rows, dtype)
        D = matrix_of(ix)
        assert np.all(D[3, np.arange(40) != 3] == 1) and D[17, 30] == 1
        check(clip_lib, ix, D, 40)
        c, reach, owner, dist, cover = check(clip_lib, ix, D, 2, seeds=[17, 3])
        assert owner[30] == 17 and dist[30] == 1 and np.all(dist[np.setdiff1d(np.arange(40), [3, 17])] == 1)
        ix.close()


def test_20000_planted_rows(clip, clip_lib, tmp_path):
    """256 picks over 20 000 rows at dim 64, several tiles per wave: checked against float64 distances of the stored values"""
    rng = np.random.default_rng(51)
    n, dim, n_max = 20000, 64, 256
    ix = make_index(clip, clip_lib, planted(rng, n, dim), "f16")
    result = ix.spread(n_max)
    r64 = stored64(ix, tmp_path)
    centres = result[0]
    assert len(centres) == n_max and centres[0] == 0
    d64 = 1.0 - r64 @ r64[centres].T                 # only the centres' columns: [x, t] = d(x, centres[t])
    tol = tol_of(dim)
    gap = d64[:, 0].copy()
    chosen = np.zeros(n, dtype=bool)
    chosen[0] = True
    for t in range(1, n_max):
        x = centres[t]
        assert not chosen[x] and gap[x] >= np.where(chosen, -np.inf, gap).max() - 2 * tol and abs(gap[x] - float(result[1][t])) <= tol
        chosen[x] = True
        gap = np.minimum(gap, d64[:, t])
    rest = ~chosen
    assert np.all(np.abs(gap[rest] - result[3][rest].astype(np.float64)) <= tol) and np.all(result[3][chosen] == 0)
    pos = np.full(n, -1)
    pos[centres] = np.arange(n_max)
    assert np.all(np.abs(d64[np.flatnonzero(rest), pos[result[2][rest]]] - gap[rest]) <= 2 * tol)
    assert abs(float(result[4]) - gap[rest].max()) <= tol and same_bits(np.float32(result[4]), result[3].max())
    assert np.all(np.diff(result[1][1:]) <= 0)
    ix.close()
