"""GPU tier of removal and subset search on the join side of the exact index (the masked instantiation of join_kernel): range search over
the eligible rows E — by removal, by an allowed set, or by both — and pairs after removal equal, bit for bit, those of a fresh index Y of
R[E] with the ids mapped in order; lims keeps its shape, removed rows own empty segments, count-only calls return the same totals."""
import numpy as np
import pytest

from index_subset_common import (DTYPES, WAYS, eligible_sets, fp, ip, make_x, make_y, open_clip, raw_range_subset, same_bits, stray_words)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    m = open_clip(clip_lib, fixture_cache)
    yield m
    m.close()


# dim, n, nq: n around the 128-row tile edge, nq on both query-tile widths (16 queries up to 16, 128 above)
SHAPES = [(32, 1, 1), (512, 1, 17), (32, 127, 17), (512, 127, 130), (32, 128, 1), (512, 128, 17), (32, 129, 130), (512, 129, 1),
          (32, 1000, 130), (512, 1000, 17), (512, 1000, 1)]


def planted(rng, n, nq, dim):
    """rows with perturbed copies of earlier rows and one zero row; queries that are perturbed rows, one exact row, one zero query"""
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    for i in range(3, n, 5):
        rows[i] = rows[i - 3] + 0.02 * rng.standard_normal(dim, dtype=np.float32)
    if n > 2:
        rows[n // 2] = 0.0
    q = rows[rng.integers(0, n, size=nq)] + 0.02 * rng.standard_normal((nq, dim), dtype=np.float32)
    q[0] = rows[0]
    if nq > 2:
        q[nq - 1] = 0.0
    return rows, q


def radii(dim):
    """0.05: the planted copies only; a cut through the bulk of the random rows (cosine of random vectors: sigma = 1 / sqrt(dim));
    1.0: about half of the rows, and the zero row at exactly 1"""
    return [0.05, 1.0 - 1.0 / np.sqrt(dim), 1.0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim, n, nq", SHAPES)
def test_range_search_subset_equals_fresh_index(clip, clip_lib, dtype, dim, n, nq):
    rng = np.random.default_rng(dim + 7 * n + nq)
    rows, q = planted(rng, n, nq, dim)
    sizes = set()
    for name, elig in eligible_sets(n).items():
        y, m = make_y(clip_lib, clip, rows, dtype, elig)
        want = [y.range_search(q, r) for r in radii(dim)]
        for way in WAYS:
            x, allow = make_x(clip_lib, clip, rows, dtype, elig, way)
            for r, (yl, yd, yi) in zip(radii(dim), want):
                if way == "allow":      # raw entry point, stray bits past size set; count-only first, then with the exact capacity
                    words = stray_words(clip_lib, allow)
                    total, lims, _, _ = raw_range_subset(clip_lib, x, q, r, words, 0)
                    assert total == len(yi) and np.array_equal(lims, yl), (name, way, r)
                    total, l, d, i = raw_range_subset(clip_lib, x, q, r, words, total)
                    assert total == len(yi)
                else:
                    l, d, i = x.range_search(q, r, allow=allow)
                assert np.array_equal(l, yl) and same_bits(d, yd) and np.array_equal(i, m[yi]), (name, way, r)
                if name == "all":
                    sizes.add(len(yi))
            x.close()
        y.close()
    if n >= 127:
        assert min(sizes) > 0 and max(sizes) < n * nq          # the radii are neither empty nor everything


def raw_pairs(clip_lib, ix, radius, capacity):
    lims = np.full(len(ix) + 1, -7, dtype=np.int64)
    dist = np.empty(max(capacity, 1), dtype=np.float32)
    ids = np.empty(max(capacity, 1), dtype=np.int64)
    total = clip_lib.lib().clip_amd_index_pairs(ix.handle, float(radius), ip(lims), fp(dist) if capacity else None, ip(ids) if capacity else None,
                                                capacity)
    return int(total), lims


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim, n", sorted(set(s[:2] for s in SHAPES)))
def test_pairs_after_removal_equal_fresh_index(clip, clip_lib, dtype, dim, n):
    rng = np.random.default_rng(dim + 11 * n)
    rows, _ = planted(rng, n, 1, dim)
    for name, elig in eligible_sets(n).items():
        y, m = make_y(clip_lib, clip, rows, dtype, elig)
        x, _ = make_x(clip_lib, clip, rows, dtype, elig, "remove")
        for r in radii(dim):
            yi, yj, yd = y.pairs(r)
            xi, xj, xd = x.pairs(r)
            assert np.array_equal(xi, m[yi]) and np.array_equal(xj, m[yj]) and same_bits(xd, yd), (name, r)
            total, lims = raw_pairs(clip_lib, x, r, 0)                       # count only: size + 1 entries, removed rows own nothing
            assert total == len(yd) and len(lims) == n + 1 and lims[0] == 0 and lims[-1] == total
            per_row = np.zeros(n, dtype=np.int64)
            per_row[elig] = np.bincount(yi, minlength=int(elig.sum()))
            assert np.array_equal(np.diff(lims), per_row), (name, r)
        x.close()
        y.close()
