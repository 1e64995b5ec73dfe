"""Shared pieces of the distinct-search tests of the exact index (not a test module): the definition of the walk in plain Python, the
planted data set and the oracle that applies the definition to the index's own search results."""
import numpy as np


def walk(ranked, near, k):
    """The definition.  ranked: the ids of one pool's members in search's order (a -1 ends the pool); near: a set of (lower id, higher id)
    pairs; returns (kept ids, counts), at most k of each: a member that an earlier kept member is near to is suppressed and suppresses
    nothing; counts[t] is the number of members kept member t suppressed, each counted for the first kept member near it, over the
    whole pool."""
    members = []
    for r in ranked:
        if int(r) < 0:
            break
        members.append(int(r))
    suppressed, kept, counts = set(), [], []
    for pos, a in enumerate(members):
        if len(kept) == k:
            break
        if a in suppressed:
            continue
        mine = [b for b in members[pos + 1:] if b not in suppressed and (min(a, b), max(a, b)) in near]
        suppressed.update(mine)
        kept.append(a)
        counts.append(len(mine))
    return kept, counts


def collapse(ranked, near, k):
    """What distinct search is NOT: the first member of every connected component of the near graph over the pool"""
    members = [int(r) for r in ranked if int(r) >= 0]
    parent = {a: a for a in members}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in near:
        if a in parent and b in parent:
            parent[find(a)] = find(b)
    seen, kept = set(), []
    for a in members:
        if find(a) not in seen:
            seen.add(find(a))
            kept.append(a)
    return kept[:k]


def planted(dim, seed=0):
    """(rows f32 [170, dim], kind int [170]): 40 unit base vectors in three kinds by b % 3: 0 a singleton; 1 a burst, the base and 5 copies
    base + 0.1 / sqrt(dim) N(0, I); 2 a chain of 6, cos(0.25 t) base + sin(0.25 t) dir with dir a unit vector orthogonal to base
    (consecutive members at distance ~0.031, members two apart at ~0.122); permuted."""
    rng = np.random.default_rng(977 * dim + seed)
    rows, kind = [], []
    for b in range(40):
        base = rng.standard_normal(dim)
        base /= np.linalg.norm(base)
        if b % 3 == 0:
            rows.append(base)
            kind.append(0)
        elif b % 3 == 1:
            rows.append(base)
            rows.extend(base + 0.1 / np.sqrt(dim) * rng.standard_normal(dim) for _ in range(5))
            kind.extend([1] * 6)
        else:
            d = rng.standard_normal(dim)
            d -= d.dot(base) * base
            d /= np.linalg.norm(d)
            rows.extend(np.cos(0.25 * t) * base + np.sin(0.25 * t) * d for t in range(6))
            kind.extend([2] * 6)
    rows, kind = np.asarray(rows, dtype=np.float32), np.asarray(kind)
    assert rows.shape == (170, dim)
    order = rng.permutation(170)
    return np.ascontiguousarray(rows[order]), kind[order]


def near_pairs(ix, members, radius):
    """The near relation over the ids `members` from the index's own results: search_ids of the members among the members; for the pair
    i < j the entry of query i and row j, compared with the radius in f32."""
    members = np.asarray(members, dtype=np.int64)
    if members.size < 2:
        return set()
    allow = np.zeros(len(ix), dtype=np.bool_)
    allow[members] = True
    dist, ids = ix.search_ids(members, min(members.size, 1024), exclude_self=True, allow=allow)
    r = np.float32(radius)
    hit = (ids > members[:, None]) & (dist <= r)
    return {(int(members[t]), int(ids[t, c])) for t, c in zip(*np.nonzero(hit))}


def pair_distances(ix, members):
    """{(i, j): f32 distance} for every pair i < j of `members`, the entry of query i and row j"""
    members = np.asarray(members, dtype=np.int64)
    allow = np.zeros(len(ix), dtype=np.bool_)
    allow[members] = True
    dist, ids = ix.search_ids(members, min(members.size, 1024), exclude_self=True, allow=allow)
    return {(int(members[t]), int(ids[t, c])): dist[t, c] for t in range(members.size) for c in range(ids.shape[1]) if ids[t, c] > members[t]}


def expected(ix, ranked, k, radius, cache=None):
    """(distances [nq, k], ids [nq, k], counts [nq, k]) of the definition applied to ranked = (distances [nq, P], ids [nq, P]), the
    pools as search leaves them.  cache: a dict that keeps the near relation of a pool's member set."""
    dist, ids = ranked
    nq = len(ids)
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_c = np.zeros((nq, k), dtype=np.int32)
    for q in range(nq):
        members = ids[q][ids[q] >= 0]
        key = (id(ix), float(radius), tuple(sorted(members.tolist())))
        near = cache.get(key) if cache is not None else None
        if near is None:
            near = near_pairs(ix, members, radius)
            if cache is not None:
                cache[key] = near
        kept, counts = walk(ids[q], near, k)
        pos = {int(r): t for t, r in enumerate(ids[q]) if r >= 0}
        for t, (a, c) in enumerate(zip(kept, counts)):
            out_d[q, t], out_i[q, t], out_c[q, t] = dist[q, pos[a]], a, c
    return out_d, out_i, out_c


def same(a, b):
    """two (distances, ids, counts) results are the same bits"""
    return (a[0].shape == b[0].shape and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint32), np.ascontiguousarray(b[0]).view(np.uint32))
            and np.array_equal(a[1], b[1]) and np.array_equal(np.asarray(a[2], dtype=np.int64), np.asarray(b[2], dtype=np.int64)))
