"""The numpy reference of Index.closest_pairs over a pair list: the contract's own sentence.  The pairs (i < j, d) come exactly as
`Index.pairs(4.0)` lists them (every pair whose distance is not NaN, with the bits the contract names); the reference filters them by
eligibility, labels and `after`, sorts by (d, i, j) and cuts.  There is no arithmetic, so the library is compared with it for equality."""
import numpy as np


def reference(n, pi, pj, pd, eligible=None, labels=None, after=None):
    """(lo, hi, d): the first n candidates among the pairs pi < pj at distance pd (f32); `eligible` bool [size], `labels` int64 [size]
    (negative: not eligible; only pairs of different labels count), `after` = (d, lo, hi): only pairs strictly after it"""
    pi, pj, pd = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64), np.asarray(pd, dtype=np.float32)
    keep = ~np.isnan(pd)
    if eligible is not None:
        keep &= eligible[pi] & eligible[pj]
    if labels is not None:
        keep &= (labels[pi] >= 0) & (labels[pj] >= 0) & (labels[pi] != labels[pj])
    if after is not None:
        d, lo, hi = np.float32(after[0]), int(after[1]), int(after[2])
        keep &= (pd > d) | ((pd == d) & ((pi > lo) | ((pi == lo) & (pj > hi))))
    pi, pj, pd = pi[keep], pj[keep], pd[keep]
    order = np.lexsort((pj, pi, pd))[:n]
    return pi[order], pj[order], pd[order]
