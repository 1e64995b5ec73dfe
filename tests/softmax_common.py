"""The float64 reference of the softmax queries of the exact index (tests/test_gpu_softmax.py)."""
import numpy as np


def softmax_reference(lims, dist, ids, eligible, beta, n):
    """(probs float64 [nq, n], log_z float64 [nq]) from a complete list of distances: query i's rows are ids[lims[i] : lims[i + 1]] at
    dist[...], the f32 values search reports (what range_search at radius 4, or a search with k = every row, returns; -1 ids are
    skipped).  eligible: bool [n], or [nq, n] where it differs per query.  probs[i, r] = exp(-beta (d_ir - m_i)) / S_i over the eligible
    rows, 0 elsewhere; log_z = -beta m + log S, -inf without an eligible row."""
    nq = len(lims) - 1
    el = np.broadcast_to(np.asarray(eligible, dtype=bool), (nq, n))
    probs, log_z = np.zeros((nq, n)), np.full(nq, -np.inf)
    for i in range(nq):
        r, d = np.asarray(ids[lims[i]:lims[i + 1]]), np.asarray(dist[lims[i]:lims[i + 1]], dtype=np.float64)
        keep = r >= 0
        keep[keep] = el[i, r[keep]]
        r, d = r[keep], d[keep]
        if r.size:
            w = np.exp(-float(beta) * (d - d.min()))
            probs[i, r] = w / w.sum()
            log_z[i] = -float(beta) * d.min() + np.log(w.sum())
    return probs, log_z
