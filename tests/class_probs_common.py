"""The float64 reference of the class probabilities of the exact index (tests/test_gpu_class_probs.py)."""
import numpy as np


def class_probs_reference(lims, dist, ids, labels, eligible, beta, n_classes):
    """(probs float64 [nq, n_classes], log_z float64 [nq]) from a complete list of distances: query i's rows are ids[lims[i] : lims[i + 1]]
    at dist[...], the f32 values search reports (what range_search at radius 4, or a search with k = every row, returns; -1 ids are
    skipped).  eligible: bool [n], or [nq, n] where it differs per query; an unlabelled row (-1) is never eligible.  probs[i, c] = the sum
    of exp(-beta (d - m_i)) over the eligible rows of class c / the same sum S_i over every eligible row; log_z = -beta m + log S, -inf
    (and zeros) without an eligible row."""
    nq, labels = len(lims) - 1, np.asarray(labels)
    el = np.broadcast_to(np.asarray(eligible, dtype=bool), (nq, len(labels))) & (labels >= 0)
    probs, log_z = np.zeros((nq, n_classes)), np.full(nq, -np.inf)
    for i in range(nq):
        r, d = np.asarray(ids[lims[i]:lims[i + 1]]), np.asarray(dist[lims[i]:lims[i + 1]], dtype=np.float64)
        keep = r >= 0
        keep[keep] = el[i, r[keep]]
        r, d = r[keep], d[keep]
        if r.size:
            w = np.exp(-float(beta) * (d - d.min()))
            probs[i] = np.bincount(labels[r], weights=w, minlength=n_classes) / w.sum()
            log_z[i] = -float(beta) * d.min() + np.log(w.sum())
    return probs, log_z
