"""What the tests of the mutual-reachability tree share (tests/test_linkage_core_cpu.py, tests/test_gpu_linkage_core.py): the oracle of
clip_amd_index_linkage_core, which is the oracle of the single-linkage tree (tests/linkage_common.py: Kruskal's algorithm in the edge
order, the contract's definition word for word) over the weights w = max(d, core[lo], core[hi]), and the data generators, by import."""
import numpy as np

from linkage_common import (CHAIN_RADIUS, bursts, edge_order, forest_by_definition, kruskal, labels_of, planted, same_bits,  # noqa: F401
                            walks)


def mutual_reach(i, j, d, core):
    """w [pairs] f32 = max(d, core[i], core[j]), every operand an f32: the maximum of three numbers that are no NaNs is exact"""
    core = np.asarray(core, dtype=np.float32)
    return np.maximum(np.maximum(np.asarray(d, dtype=np.float32), core[np.asarray(i, dtype=np.int64)]), core[np.asarray(j, dtype=np.int64)])


def core_kruskal(n, i, j, d, core, link=np.inf):
    """(lo, hi, w) of the minimum spanning forest of "w <= link" under the edge order (w, lo, hi), sorted in that order"""
    return kruskal(n, i, j, mutual_reach(i, j, d, core), link)


def core_by_definition(n, i, j, d, core, link=np.inf):
    return forest_by_definition(n, i, j, mutual_reach(i, j, d, core), link)


def core_distances(n, i, j, d, k, eligible=None):
    """core [n] f32 from a pair list that holds every pair of eligible rows: the k-th smallest distance of a row to another eligible row,
    +inf with fewer than k of them and outside `eligible`, -inf over `eligible` for k = 0 (numpy; small n)"""
    eligible = np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool)
    full = np.full((n, n), np.inf, dtype=np.float32)
    use = eligible[i] & eligible[j]
    full[i[use], j[use]] = d[use]
    full[j[use], i[use]] = d[use]
    core = np.full(n, np.inf, dtype=np.float32)
    if k == 0:
        core[eligible] = -np.inf
    elif k <= n:
        core[eligible] = np.sort(full, axis=1)[eligible, k - 1]
    return core
