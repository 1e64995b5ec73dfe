"""Shared pieces of the density-modes tests of the exact index (not a test module): the contract of clip_amd_index_modes in numpy from a
pair list, and the data generators of tests/test_gpu_components.py (copied: that file stays as it is)."""
import numpy as np

STEP = 0.3                                            # tangent step of the walks: one step is at distance 1 - 1 / sqrt(1 + STEP^2)
D1 = 1.0 - 1.0 / np.sqrt(1.0 + STEP * STEP)           # 0.0422; two steps in independent directions: about twice that
CHAIN_RADIUS = 1.5 * D1


def from_pairs(n, i, j, d, radius, link, eligible=None):
    """The contract from a pair list (i[t] < j[t] at distance d[t], every pair of eligible rows with d <= max(radius, link) listed once):
    (labels int64, parent int64, parent_distance f32, density int32, modes).
    density: the pairs with d <= radius a row is in, compared in f32.  y outranks x: density[y] > density[x], or equal and y < x.
    parent: per row the first of its outranking other endpoints with d <= link in the order (d, other id); -1 / +inf without one.
    labels: parents followed to the fixed point.  A row that is not eligible: -1, -1, +inf, -1."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    d = np.asarray(d, dtype=np.float32)
    radius, link = np.float32(radius), np.float32(link)
    ok = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool)
    assert np.all(ok[i]) and np.all(ok[j]), "a pair with a row that is not eligible"
    near = d <= radius
    density = (np.bincount(i[near], minlength=n) + np.bincount(j[near], minlength=n)).astype(np.int32)
    rows, other, dd = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([d, d])
    up = (dd <= link) & ((density[other] > density[rows]) | ((density[other] == density[rows]) & (other < rows)))
    rows, other, dd = rows[up], other[up], dd[up]
    order = np.lexsort((other, dd, rows))             # per row: distance ascending, then the other id
    first = order[np.concatenate([[True], np.diff(rows[order]) != 0])] if rows.size else order
    parent = np.full(n, -1, dtype=np.int64)
    pdist = np.full(n, np.inf, dtype=np.float32)
    parent[rows[first]] = other[first]
    pdist[rows[first]] = dd[first]
    labels = np.where(parent >= 0, parent, np.arange(n, dtype=np.int64))
    while True:
        nxt = labels[labels]
        if np.array_equal(nxt, labels):
            break
        labels = nxt
    modes = int(np.count_nonzero(ok & (parent < 0)))
    labels[~ok] = -1
    density[~ok] = -1
    return labels, parent, pdist, density, modes


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


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
