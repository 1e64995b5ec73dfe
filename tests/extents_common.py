"""What the two tiers of the extents tests share: the numpy reference of Index.extents over a pair list, and the data.

The reference takes the pairs (i < j, d) exactly as `Index.pairs(4.0)` lists them (cosine distances never exceed 2, so that is every pair
whose distance is not NaN, with the bits the contract names) and derives every output by the contract's own definitions: there is no
arithmetic, only comparisons of those f32 values, so the library is compared with it for equality."""
import numpy as np


def reference(size, labels, pi, pj, pd, eligible=None):
    """(centre, radius, diameter, reach, far, groups) of the contract: `labels` int64 [size], the pairs pi < pj at distance pd (f32),
    `eligible` bool [size] or None for every row.  A pair counts when both rows are members and carry one label."""
    labels = np.asarray(labels, dtype=np.int64)
    member = labels >= 0
    if eligible is not None:
        member &= np.asarray(eligible, dtype=np.bool_)
    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    pd = np.asarray(pd, dtype=np.float32)
    reach = np.where(member, np.float32(0), np.float32(np.inf)).astype(np.float32)
    far = np.full(size, -1, dtype=np.int64)
    have = np.zeros(size, dtype=np.bool_)
    keep = member[pi] & member[pj] & (labels[pi] == labels[pj]) & ~np.isnan(pd)
    for a, b, d in zip(pi[keep].tolist(), pj[keep].tolist(), pd[keep]):
        for x, y in ((a, b), (b, a)):
            if not have[x] or d > reach[x] or (d == reach[x] and y < far[x]):
                reach[x], far[x], have[x] = d, y, True
    centre = np.full(size, -1, dtype=np.int64)
    radius = np.full(size, np.inf, dtype=np.float32)
    diameter = np.full(size, np.inf, dtype=np.float32)
    groups = 0
    for lab in np.unique(labels[member]).tolist():
        g = np.flatnonzero(member & (labels == lab))
        c = min(g.tolist(), key=lambda x: (reach[x], x))
        centre[g], radius[g], diameter[g] = c, reach[c], reach[g].max()
        groups += 1
    return centre, radius, diameter, reach, far, groups


def same_bits(got, want):
    """every array of `got` equals its partner in `want`, floats by their bits"""
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != w.dtype or g.shape != w.shape:
            return False
        if not np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w):
            return False
    return True


def clustered(rng, n, dim, clusters=12, noise=0.25):
    """rows around `clusters` directions with exact copies sprinkled in: near rows, far rows and ties of distance in one index"""
    heads = rng.standard_normal((clusters, dim)).astype(np.float32)
    rows = heads[rng.integers(0, clusters, n)] + noise * rng.standard_normal((n, dim)).astype(np.float32)
    for r in range(5, n, 9):
        rows[r] = rows[r - 3]                  # an exact copy of an earlier row
    return rows.astype(np.float32)
