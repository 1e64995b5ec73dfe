"""References of the biased-search tests: all distances of an index through range_search (search's bits), and a float64 restatement of
the stored rows and stored queries (f16 as tests/test_gpu_search.py, i8 as tests/test_gpu_search_i8.py does it)."""
import struct

import numpy as np


def all_distances(ix, q):
    """float32 [nq, len]: range_search's distance of every (query, row) pair, +inf where a row is not eligible"""
    lims, dist, ids = ix.range_search(q, 4.0)
    D = np.full((len(q), len(ix)), np.inf, dtype=np.float32)
    D[np.repeat(np.arange(len(q)), np.diff(lims)), ids] = dist
    return D


def top_k(scores, k):
    """(ids int64 [nq, k], order) by np.lexsort((ids, scores)) per query; -1 where the score is +inf or there is no row"""
    nq, n = scores.shape
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        o = np.lexsort((np.arange(n), scores[i]))[:k]
        o = o[np.isfinite(scores[i, o])]
        ids[i, :o.size] = o
    return ids


def unit64(v):
    v = np.asarray(v, dtype=np.float64)
    nrm = np.sqrt((v * v).sum(1))[:, None]
    return np.where(nrm > 0, v / np.where(nrm > 0, nrm, 1), 0)


def stored64(ix, q, dtype, path):
    """(rows, queries) float64 unit vectors of what the index stores (from its own file) and of the queries as it prepares them"""
    ix.save(path)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(path, "rb").read(28)[8:])
    q = np.asarray(q, dtype=np.float32)
    if dtype == "i8":
        rows = np.fromfile(path, dtype=np.int8, offset=28).reshape(n, dim)
        q8 = np.rint((q / np.abs(q).max(1, keepdims=True)).astype(np.float32) * np.float32(127))
        return unit64(rows), unit64(q8)
    rows = np.fromfile(path, dtype=np.float16, offset=28).reshape(n, dim).astype(np.float64)
    sq = np.zeros((len(q), (dim + 63) // 64 * 64), dtype=np.float32)      # the kernel's own summation order (stored_queries of test_gpu_search.py)
    sq[:, :dim] = q * q
    lanes = np.zeros((len(q), 64), dtype=np.float32)
    for c in range(0, sq.shape[1], 64):
        lanes = lanes + sq[:, c:c + 64]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ off]
    return rows, (q / np.sqrt(lanes[:, :1])).astype(np.float32).astype(np.float16).astype(np.float64)
