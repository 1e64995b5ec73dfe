"""What the linkage tests share (tests/test_linkage_cpu.py, tests/test_gpu_linkage.py): the oracle of clip_amd_index_linkage, Kruskal's
algorithm in numpy over a pair list in the edge order (d, lo, hi), the brute-force form of the contract's definition for tiny graphs, and
copies of the data generators of tests/test_gpu_components.py (walks, bursts, planted)."""
import numpy as np

STEP = 0.3                                            # tangent step of the walks: one step is at distance 1 - 1 / sqrt(1 + STEP^2)
D1 = 1.0 - 1.0 / np.sqrt(1.0 + STEP * STEP)           # 0.0422; two steps in independent directions: about twice that
CHAIN_RADIUS = 1.5 * D1
KRUSKAL_CHUNK = 4096


def edge_order(lo, hi, d):
    """the permutation that sorts edges by (d, lo, hi); d is compared as f32"""
    return np.lexsort((np.asarray(hi), np.asarray(lo), np.asarray(d, dtype=np.float32)))


def kruskal(n, i, j, d, link=np.inf):
    """(lo, hi, d) of the minimum spanning forest of the graph "d <= link" over the pairs (i[t] < j[t], d[t]) under the edge order
    (d, lo, hi), sorted in that order: the edges are walked in order and one is taken when its ends are not connected yet.  The walk
    goes through the sorted list in chunks; ahead of each chunk a vectorised pass drops the edges whose ends the forest so far already
    connects (they can never be taken), the rest is plain Kruskal."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    d = np.asarray(d, dtype=np.float32)
    assert np.all(i < j)
    use = d <= np.float32(link)
    i, j, d = i[use], j[use], d[use]
    order = edge_order(i, j, d)
    i, j, d = i[order], j[order], d[order]
    parent = np.arange(n, dtype=np.int64)
    taken = []
    for s in range(0, len(i), KRUSKAL_CHUNK):
        if len(taken) == n - 1:
            break
        while True:                                   # flat: parent[x] is x's root
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        open_edges = np.flatnonzero(parent[i[s:s + KRUSKAL_CHUNK]] != parent[j[s:s + KRUSKAL_CHUNK]]) + s
        for t in open_edges.tolist():
            a, b = int(i[t]), int(j[t])
            while parent[a] != a:
                a = int(parent[a])
            while parent[b] != b:
                b = int(parent[b])
            if a != b:
                parent[max(a, b)] = min(a, b)
                taken.append(t)
    taken = np.asarray(taken, dtype=np.int64)
    return i[taken], j[taken], d[taken]


def forest_by_definition(n, i, j, d, link=np.inf):
    """the contract word for word, for tiny graphs: an edge with d <= link belongs to the forest exactly when its ends are not connected
    by the edges that are strictly smaller in the order (d, lo, hi); sorted in that order"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    d = np.asarray(d, dtype=np.float32)
    keys = [(float(d[t]), int(i[t]), int(j[t])) for t in range(len(i)) if d[t] <= np.float32(link)]
    out = []
    for key in keys:
        label = list(range(n))
        changed = True
        while changed:                                # label propagation over the strictly smaller edges
            changed = False
            for other in keys:
                if other < key and label[other[1]] != label[other[2]]:
                    label[other[1]] = label[other[2]] = min(label[other[1]], label[other[2]])
                    changed = True
        if label[key[1]] != label[key[2]]:
            out.append(key)
    out.sort()
    return (np.array([k[1] for k in out], dtype=np.int64), np.array([k[2] for k in out], dtype=np.int64),
            np.array([k[0] for k in out], dtype=np.float32))


def labels_of(n, lo, hi, eligible=None):
    """the lowest id of every row's group under the given edges (numpy label propagation to the fixed point); -1 outside eligible"""
    labels = np.arange(n, dtype=np.int64)
    while True:
        nxt = labels.copy()
        np.minimum.at(nxt, lo, labels[hi])
        np.minimum.at(nxt, hi, labels[lo])
        nxt = nxt[nxt]
        if np.array_equal(nxt, labels):
            break
        labels = nxt
    if eligible is not None:
        labels[~eligible] = -1
    return labels


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


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
