"""Shared pieces of the k-NN voting tests (not a test module): the definition of a vote applied in numpy to a ranking that an existing
entry point produced (Index.search / Index.search_ids with the voters as the allowed set), never to anything the voting code returned."""
import numpy as np


def vote_of(dist, ids, labels, k, m):
    """The definition on rankings: dist / ids [nq, >= k'] are each query's voters in search's order (-1 padded; only the first k columns
    are read), labels the int label of every row.  Per query: the classes of the first k voters by votes descending, then by the rank of
    the class's nearest entry; per class its number, votes, and the distance and id of that entry; the tail -1 / 0 / +inf / -1.
    Returns (classes int32, votes int32, distances f32, ids int64), [nq, m] each."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    nq = dist.shape[0]
    out_c = np.full((nq, m), -1, dtype=np.int32)
    out_v = np.zeros((nq, m), dtype=np.int32)
    out_d = np.full((nq, m), np.inf, dtype=np.float32)
    out_i = np.full((nq, m), -1, dtype=np.int64)
    for q in range(nq):
        row = ids[q, :k]
        row = row[row >= 0]
        if not len(row):
            continue
        cls, first, votes = np.unique(labels[row], return_index=True, return_counts=True)
        order = np.lexsort((first, -votes))[:m]              # votes descending, then the first rank ascending
        n = len(order)
        out_c[q, :n] = cls[order]
        out_v[q, :n] = votes[order]
        out_d[q, :n] = dist[q, first[order]]
        out_i[q, :n] = row[first[order]]
    return out_c, out_v, out_d, out_i


def same_votes(a, b):
    """two (classes, votes, distances, ids) results are the same bits"""
    return (all(np.asarray(x).shape == np.asarray(y).shape for x, y in zip(a, b)) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.ascontiguousarray(a[2], dtype=np.float32).view(np.uint32), np.ascontiguousarray(b[2], dtype=np.float32).view(np.uint32))
            and np.array_equal(a[3], b[3]))


def voters_of(labels, allow=None, live=None):
    """bool [n]: labelled, allowed (None: every row) and live (None: every row)"""
    v = np.asarray(labels) >= 0
    if allow is not None:
        v = v & np.asarray(allow, dtype=bool)
    if live is not None:
        v = v & np.asarray(live, dtype=bool)
    return v
