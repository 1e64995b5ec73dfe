"""GPU tier of clip_amd_index_compact (compact_ids_kernel / compact_gather_kernel): after remove + compact the index is, byte for byte in
its saved file and bit for bit in its results, the index Y to which only the survivors were ever added; new_ids maps every old id."""
import numpy as np
import pytest

from index_subset_common import DTYPES, make_y, open_clip, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    m = open_clip(clip_lib, fixture_cache)
    yield m
    m.close()


def removal_sets(n):
    rng = np.random.default_rng(77 + n)
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "random40": rng.random(n) < 0.4}


# n = 70000 rows: the prefix count spans two workgroups of 65536 rows each; 4097: many bitmap words, one workgroup
CASES = [(dt, 32, n) for dt in DTYPES for n in (1, 64, 65, 4097, 70000)] + [(dt, 200, 4097) for dt in DTYPES]


@pytest.mark.parametrize("dtype, dim, n", CASES)
def test_compact_equals_fresh_index(clip, clip_lib, tmp_path, dtype, dim, n):
    L = clip_lib.lib()
    rng = np.random.default_rng(dim + n)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    extra = rng.standard_normal((70, dim), dtype=np.float32)
    q = rng.standard_normal((17, dim), dtype=np.float32)
    q[0] = rows[n - 1]
    k = 100
    px, py = str(tmp_path / "x.index"), str(tmp_path / "y.index")
    for name, gone in removal_sets(n).items():
        keep = ~gone
        n_e = int(keep.sum())
        y, _ = make_y(clip_lib, clip, rows, dtype, keep)
        x = clip_lib.Index(clip, dim, dtype)
        x.add(rows[:n // 2])
        x.add(rows[n // 2:])
        if gone.any():
            assert x.remove(np.flatnonzero(gone)) == n - n_e
        new_ids = x.compact()
        assert np.array_equal(new_ids, np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)), name
        if name == "random40" and dtype == "f16":                # NULL new_ids: a second index ends up with the same bytes (below)
            x.close()
            x = clip_lib.Index(clip, dim, dtype)
            x.add(rows)
            assert x.remove(np.flatnonzero(gone)) == n - n_e
            assert L.clip_amd_index_compact(x.handle, None) == n_e
        assert len(x) == n_e and x.live == n_e and np.array_equal(x.live_mask(), np.ones(n_e, dtype=bool))
        x.save(px)
        y.save(py)
        raw = open(px, "rb").read()
        assert raw == open(py, "rb").read(), name                # the stored values moved bit for bit
        if n_e == 0:
            assert len(raw) == 28                                # a header-only file
        yd, yi = y.search(q, k)
        d, i = x.search(q, k)
        assert same_bits(d, yd) and np.array_equal(i, yi), name
        if n_e == 0:
            assert np.all(i == -1) and np.all(np.isinf(d))
        for r in (0.05, 1.0):
            for a, b in zip(x.range_search(q, r), y.range_search(q, r)):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), name
        z = clip_lib.Index.load(clip, px)                        # unchanged across a save / load round trip
        d, i = z.search(q, k)
        assert len(z) == n_e and same_bits(d, yd) and np.array_equal(i, yi), name
        z.close()
        for a in (x, y):                                         # a later add continues from id |E|
            a.add(extra)
        assert len(x) == n_e + 70 and x.live == n_e + 70
        yd, yi = y.search(q, k)
        d, i = x.search(q, k)
        assert same_bits(d, yd) and np.array_equal(i, yi), name
        d, i = x.search(extra[:3] * 2.0, 1)
        assert i[:, 0].tolist() == [n_e, n_e + 1, n_e + 2]
        x.save(px)
        y.save(py)
        assert open(px, "rb").read() == open(py, "rb").read(), name
        x.close()
        y.close()


def test_compact_twice_and_after_more_removals(clip, clip_lib):
    rng = np.random.default_rng(8)
    dim = 32
    rows = rng.standard_normal((500, dim), dtype=np.float32)
    q = rng.standard_normal((5, dim), dtype=np.float32)
    x = clip_lib.Index(clip, dim, "i8")
    x.add(rows)
    x.remove(np.arange(0, 500, 2))
    first = x.compact()
    assert np.array_equal(x.compact(), np.arange(250))           # nothing removed since: a no-op, every id stays
    x.remove([0, 249])
    second = x.compact()
    assert second[0] == -1 and second[249] == -1 and np.array_equal(second[1:249], np.arange(248))
    keep = np.zeros(500, dtype=bool)
    keep[np.flatnonzero(first >= 0)[1:249]] = True
    y, _ = make_y(clip_lib, clip, rows, "i8", keep)
    yd, yi = y.search(q, 10)
    d, i = x.search(q, 10)
    assert len(x) == 248 and same_bits(d, yd) and np.array_equal(i, yi)
    x.close()
    y.close()
