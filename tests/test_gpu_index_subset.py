"""GPU tier of row removal and subset search on the exact index (clip_amd_index_remove / _live / _live_mask / _search_subset[_device];
the masked instantiation of search_scan_kernel): X restricted to the eligible rows E — by removal, by an allowed set, or by both —
returns exactly what a fresh index Y of R[E] returns, ids mapped in order.  All comparisons are exact (bits of the distances, ids)."""
import numpy as np
import pytest

from index_subset_common import DTYPES, WAYS, eligible_sets, ip, make_x, make_y, open_clip, raw_search_subset, same_bits, stray_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    m = open_clip(clip_lib, fixture_cache)
    yield m
    m.close()


# dim, n, nq, k: every dim, n (1, around one 64-row iteration, several chunks at >= 257, 5000), query tiling (1, 2, 4) and k (1024 at n = 5000:
# one chunk with the buffer-shrink path busy) appears several times; a pruned cross product
SHAPES = [
    (32, 1, 1, 1), (512, 1, 17, 5), (32, 63, 17, 5), (512, 63, 1, 100), (200, 64, 1, 1), (32, 64, 70, 1024), (32, 65, 70, 100),
    (200, 65, 17, 1024), (512, 257, 17, 5), (200, 257, 70, 1), (200, 1000, 70, 100), (512, 1000, 1, 1024), (32, 1000, 17, 1),
    (32, 5000, 17, 1024), (512, 5000, 70, 100), (200, 5000, 1, 5),
]
CASES = [(dt,) + s for dt in DTYPES for s in SHAPES if not (dt != "f16" and s in ((512, 1, 17, 5), (32, 64, 70, 1024)))]


@pytest.mark.parametrize("dtype, dim, n, nq, k", CASES)
def test_subset_equals_fresh_index(clip, clip_lib, dtype, dim, n, nq, k):
    rng = np.random.default_rng(dim * 13 + n * 3 + nq + k)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    q[0] = rows[n // 2] * 2.0
    for name, elig in eligible_sets(n).items():
        y, m = make_y(clip_lib, clip, rows, dtype, elig)
        yd, yi = y.search(q, k)
        want_ids = m[yi]
        n_e = int(elig.sum())
        assert np.all(yi[:, min(k, n_e):] == -1) and np.all(np.isinf(yd[:, min(k, n_e):]))       # what the tail must look like
        for way in WAYS:
            x, allow = make_x(clip_lib, clip, rows, dtype, elig, way)
            if way == "allow":          # through the raw entry point, every bit at a position >= size set: those bits are ignored
                d, i = raw_search_subset(clip_lib, x, q, k, stray_words(clip_lib, allow))
            else:
                d, i = x.search(q, k, allow=allow)
            assert same_bits(d, yd) and np.array_equal(i, want_ids), (name, way)
            x.close()
        y.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_zero_rows_with_exclusions(clip, clip_lib, dtype):
    rng = np.random.default_rng(5)
    dim = 64
    rows = rng.standard_normal((3000, dim), dtype=np.float32)
    dup = rows[10].copy()
    dup_ids = [10, 11, 700, 1999, 2000, 2950]
    for i in dup_ids:
        rows[i] = dup
    rows[500] = 0.0
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows[:1234])
    ix.add(rows[1234:])
    assert ix.remove([11, 2000]) == 2
    allow = np.ones(3000, dtype=bool)
    allow[700] = False
    d, g = ix.search(dup[None], 8, allow=allow)
    assert g[0, :3].tolist() == [10, 1999, 2950] and np.all(d[0, :3] == d[0, 0])         # the survivors, in id order at one distance
    assert not set(g[0].tolist()) & {11, 700, 2000} and d[0, 3] > d[0, 0]
    d, g = ix.search(dup[None], 8)                                                       # removal alone: 700 is back
    assert g[0, :4].tolist() == [10, 700, 1999, 2950] and np.all(d[0, :4] == d[0, 0])
    z = np.zeros((2, dim), dtype=np.float32)
    d, g = ix.search(z, 5, allow=np.arange(3000) >= 9)      # zero query: distance exactly 1 to everything, lowest eligible ids first
    assert np.all(d == 1.0) and g.tolist() == [[9, 10, 12, 13, 14]] * 2
    zr = clip_lib.Index(clip, dim, dtype)                   # a zero row stays at distance exactly 1, while it is eligible
    zr.add(rows[:600])
    zr.remove(np.arange(100, 300))
    qs = rng.standard_normal((4, dim), dtype=np.float32)
    d, g = zr.search(qs, 1024)
    assert np.all((g == 500).sum(1) == 1) and np.all(d[g == 500] == 1.0) and np.all(g[:, 400:] == -1) and np.all(g[:, :400] >= 0)
    assert not np.any((g >= 100) & (g < 300))
    d, g = zr.search(qs, 1024, allow=np.arange(600) != 500)
    assert not np.any(g == 500) and np.all(g[:, 399:] == -1) and np.all(np.isinf(d[:, 399:]))
    ix.close()
    zr.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_then_add_past_the_capacity(clip, clip_lib, dtype):
    rng = np.random.default_rng(31)
    dim, nq, k = 32, 17, 100
    rows = rng.standard_normal((3000, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    x = clip_lib.Index(clip, dim, dtype)
    x.add(rows[:1000])
    first = rng.permutation(1000)[:300]
    assert x.remove(first) == 300
    assert x.remove(np.concatenate([first[:50], first[:50]])) == 0                 # removed before, and twice in one call
    x.add(rows[1000:])                                                             # 3000 rows: past the first allocation of 1024
    assert len(x) == 3000 and x.live == 2700
    live = np.ones(3000, dtype=bool)
    live[first] = False
    assert np.array_equal(x.live_mask(), live)                                     # removal state survived the reallocation
    second = np.array([1000, 1000, 1500, 2999, 2999, 1001, int(first[0])])
    assert x.remove(second) == 4                                                   # duplicates count once, an old one not at all
    live[second] = False
    assert x.live == 2696 and len(x) == 3000 and np.array_equal(x.live_mask(), live)
    y, m = make_y(clip_lib, clip, rows, dtype, live)
    yd, yi = y.search(q, k)
    d, i = x.search(q, k)
    assert same_bits(d, yd) and np.array_equal(i, m[yi])
    sub = live & (rng.random(3000) < 0.3)
    y2, m2 = make_y(clip_lib, clip, rows, dtype, sub)
    yd, yi = y2.search(q, k)
    d, i = x.search(q, k, allow=np.flatnonzero(sub | ~live))                        # ids form; removed rows allowed: they stay away
    assert same_bits(d, yd) and np.array_equal(i, m2[yi])
    for a in (x, y, y2):
        a.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form_matches_host_form(clip, clip_lib, dtype):
    import torch
    assert torch.cuda.is_available()
    rng = np.random.default_rng(9)
    dim, n, nq, k = 200, 3000, 37, 50
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    x = clip_lib.Index(clip, dim, dtype)
    x.add(rows)
    x.remove(np.arange(0, n, 7))
    allow = rng.random(n) < 0.4
    hd, hi = x.search(q, k, allow=allow)
    words = stray_words(clip_lib, allow)
    tw = torch.from_numpy(words.view(np.int64).copy()).cuda()
    tq = torch.from_numpy(q).cuda()
    td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    x.search_subset_device(tq.data_ptr(), nq, k, tw.data_ptr(), td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert same_bits(td.cpu().numpy(), hd) and np.array_equal(ti.cpu().numpy(), hi)
    x.search_subset_device(tq.data_ptr(), nq, k, None, td.data_ptr(), ti.data_ptr())      # NULL: every live row
    clip.synchronize()
    hd, hi = x.search(q, k)
    assert same_bits(td.cpu().numpy(), hd) and np.array_equal(ti.cpu().numpy(), hi)
    x.close()


def test_bad_arguments_change_nothing(clip, clip_lib, tmp_path, capfd):
    L = clip_lib.lib()
    rng = np.random.default_rng(3)
    dim = 32
    ix = clip_lib.Index(clip, dim, "f16")
    ix.add(rng.standard_normal((10, dim), dtype=np.float32))
    q = rng.standard_normal((3, dim), dtype=np.float32)
    d0, i0 = ix.search(q, 5)
    capfd.readouterr()

    def unchanged():
        d, i = ix.search(q, 5)
        return same_bits(d, d0) and np.array_equal(i, i0) and ix.live == 10 and len(ix) == 10

    for bad in ([3, 10], [-1], [0, 1, 2, 1 << 40]):
        a = np.asarray(bad, dtype=np.int64)
        assert L.clip_amd_index_remove(ix.handle, ip(a), len(a)) == -1                 # one id out of range: nothing is removed
        assert "outside" in capfd.readouterr().err and unchanged()
    a = np.asarray([1], dtype=np.int64)
    assert L.clip_amd_index_remove(ix.handle, None, 1) == -1 and "NULL ids" in capfd.readouterr().err and unchanged()
    assert L.clip_amd_index_remove(ix.handle, ip(a), -1) == -1 and capfd.readouterr().err and unchanged()
    assert L.clip_amd_index_remove(None, ip(a), 1) == -1 and capfd.readouterr().err
    assert L.clip_amd_index_remove(ix.handle, None, 0) == 0 and unchanged()           # nothing to do is not an error
    assert L.clip_amd_index_compact(None, None) == -1 and capfd.readouterr().err
    assert not L.clip_amd_index_live_mask(None, None) and capfd.readouterr().err
    assert L.clip_amd_index_live(None) == 0
    with pytest.raises(RuntimeError):
        ix.remove([10])
    capfd.readouterr()
    with pytest.raises(ValueError):
        ix.search(q, 5, allow=np.ones(9, dtype=bool))
    with pytest.raises(ValueError):
        ix.search(q, 5, allow=[10])
    with pytest.raises(ValueError):
        ix.range_search(q, 0.5, allow=[-1])
    assert capfd.readouterr().err == "" and unchanged()                                 # raised before any call into the library
    good = str(tmp_path / "good.index")
    ix.save(good)
    assert ix.remove([4]) == 1
    path = str(tmp_path / "removed.index")
    assert not L.clip_amd_index_save(ix.handle, path.encode())
    assert "compact" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        ix.save(path)
    d, i = ix.search(q, 5)                                                              # the refused save left the index as it was
    ok =clip_lib.Index.load(clip, good)
    ok.remove([4])
    d1, i1 = ok.search(q, 5)
    assert same_bits(d, d1) and np.array_equal(i, i1) and 4 not in i and ix.live == 9
    ok.close()
    ix.close()
