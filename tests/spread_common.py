"""Shared pieces of the farthest-first selection tests of the exact index (not a test module): the contract of clip_amd_index_spread in
numpy over a dense distance matrix, and the data generators of tests/modes_common.py (copied: that file stays as it is)."""
import numpy as np

STEP = 0.3                                            # tangent step of the walks: one step is at distance 1 - 1 / sqrt(1 + STEP^2)
D1 = 1.0 - 1.0 / np.sqrt(1.0 + STEP * STEP)           # 0.0422; two steps in independent directions: about twice that


def matrix_from_pairs(n, i, j, d):
    """dense f32 [n, n] from a full pair list: D[i, j] = D[j, i] = d, everything else (the diagonal, rows without pairs) +inf"""
    D = np.full((n, n), np.inf, dtype=np.float32)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    d = np.asarray(d, dtype=np.float32)
    D[i, j] = d
    D[j, i] = d
    return D


def spread_contract(D, n_max, stop=-np.inf, seeds=(), eligible=None, picks_by_id=None):
    """The contract over a symmetric f32 matrix D of the distances between eligible rows (the diagonal is not read):
    (centres int64 [m], reach f32 [m], owner int64 [n], owner_distance f32 [n], cover_radius f32).
    Seeds first, in order (none: the lowest eligible id), reach +inf.  Then, while fewer than n_max centres are chosen and an eligible row
    is not one: x = the row of largest gap (the minimum of D[c, x] over the centres), the lowest id among equals; gap <= stop ends the
    traversal, else x is a centre with reach gap.  owner: the centre of smallest (D[c, x], position of c); a centre owns itself at 0; a
    row that is not eligible: -1 / +inf.  cover_radius: the largest owner distance of an eligible row (0 without one).
    picks_by_id (a list, optional): receives True / False per greedy pick: another candidate had the same gap."""
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[0]
    ok = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool).copy()
    stop = np.float32(stop)
    owner = np.full(n, -1, dtype=np.int64)
    odist = np.full(n, np.inf, dtype=np.float32)
    centres, reach = [], []
    if not ok.any():
        return np.zeros(0, np.int64), np.zeros(0, np.float32), owner, odist, np.float32(0)
    first = [int(s) for s in seeds] if len(seeds) else [int(np.flatnonzero(ok)[0])]
    assert len(set(first)) == len(first) and all(ok[s] for s in first) and len(first) <= n_max
    gap = np.full(n, np.inf, dtype=np.float32)        # of the eligible rows that are not centres
    pos = np.full(n, -1, dtype=np.int64)
    cand = ok.copy()

    def take(x, r):
        t = len(centres)
        centres.append(x)
        reach.append(r)
        cand[x] = False
        closer = cand & (D[x] < gap)                  # strictly: the earlier centre keeps a tie
        gap[closer] = D[x][closer]
        pos[closer] = t
        pos[x] = t

    for s in first:
        take(s, np.float32(np.inf))
    while len(centres) < n_max and cand.any():
        g = np.where(cand, gap, -np.inf)
        x = int(np.argmax(g))                         # the first maximum: the lowest id
        if g[x] <= stop:
            break
        if picks_by_id is not None:
            picks_by_id.append(int(np.count_nonzero(g == g[x])) > 1)
        take(x, g[x])
    c = np.asarray(centres, dtype=np.int64)
    owner[ok] = c[pos[ok]]
    odist[ok] = np.where(cand[ok], gap[ok], np.float32(0))
    cover = odist[ok].max()
    return c, np.asarray(reach, dtype=np.float32), owner, odist, np.float32(cover)


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
