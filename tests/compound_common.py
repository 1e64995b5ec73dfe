"""Shared pieces of the compound-query tests of the exact index (not a test module): the definition in plain numpy over a matrix of
single-term distances, the planted data set and its queries, and the oracle that fills that matrix from the index's own single-term
results (range_search at radius 4 for vector terms, search_ids for stored-row terms) and applies the definition."""
import numpy as np

ALL, WITHIN, BEYOND, OVER = 0, 1, 2, 3
KINDS = {"all": ALL, "within": WITHIN, "beyond": BEYOND, "over": OVER}


def compound(D, kinds, bounds, k, excluded=()):
    """The definition for one query.  D f32 [terms, n]: D[t, r] = the distance search reports for (term t, row r), NaN in every term for a
    row that is not live or not allowed; kinds [terms] (0 all, 1 within, 2 beyond, 3 over); bounds [terms] f32; excluded: row ids that are
    not eligible.  score = the max over the all-terms; within: d <= bound; beyond: d > bound; over: d > score + bound, the sum in f32.
    Returns (distances f32 [k], ids int64 [k]): the k best eligible rows by (score, id), +inf / -1 where there are fewer."""
    D = np.asarray(D, dtype=np.float32)
    assert D.ndim == 2 and D.shape[0] == len(kinds) == len(bounds), "one row of D, one kind and one bound per term"
    kinds = np.asarray(kinds, dtype=np.int64)
    bounds = np.asarray(bounds, dtype=np.float32)
    assert (kinds == ALL).any(), "a compound query ranks by at least one all-term"
    ok = ~np.isnan(D).any(axis=0)
    with np.errstate(invalid="ignore"):
        score = D[kinds == ALL].max(axis=0).astype(np.float32)
        for t, kind in enumerate(kinds):
            if kind == WITHIN:
                ok &= D[t] <= bounds[t]
            elif kind == BEYOND:
                ok &= D[t] > bounds[t]
            elif kind == OVER:
                ok &= D[t] > (score + bounds[t]).astype(np.float32)
    for r in excluded:
        if 0 <= int(r) < ok.size:
            ok[int(r)] = False
    rows = np.flatnonzero(ok)
    rows = rows[np.lexsort((rows, score[rows]))][:k]
    dist = np.full(k, np.inf, dtype=np.float32)
    ids = np.full(k, -1, dtype=np.int64)
    dist[:rows.size] = score[rows]
    ids[:rows.size] = rows
    return dist, ids


def directions(dim, count=10, seed=0):
    """`count` random unit vectors, f32 [count, dim]"""
    rng = np.random.default_rng(4177 * dim + seed)
    u = rng.standard_normal((count, dim))
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


def planted(dim, n, seed=0):
    """(rows f32 [n, dim], dirs f32 [10, dim]): every row a noisy mixture w u_i + (1 - w) u_j of a random pair of the ten directions
    with w in [0.2, 0.8], plus noise of norm ~0.25.  A row that is near u_i and u_j is the best for "all of u_i, u_j" while a row that
    is nearly u_i alone leads the single-term list of u_i, and u_i + u_j ranks by the sum of the two distances, not by the worse."""
    dirs = directions(dim, 10, seed)
    rng = np.random.default_rng(911 * dim + 7 * n + seed)
    rows = np.empty((n, dim), dtype=np.float32)
    for r in range(n):
        i, j = rng.choice(10, size=2, replace=False)
        w = rng.uniform(0.2, 0.8)
        rows[r] = w * dirs[i] + (1 - w) * dirs[j] + 0.25 / np.sqrt(dim) * rng.standard_normal(dim)
    return rows, dirs


def term_vectors(dirs, picks, rng):
    """the directions `picks` with a little noise each: what a text or an image of that concept would give"""
    dim = dirs.shape[1]
    return [(dirs[p] + 0.1 / np.sqrt(dim) * rng.standard_normal(dim)).astype(np.float32) for p in picks]


def make_queries(dirs, nq, n_terms, seed=0, lengths=None):
    """nq compound queries of n_terms terms (lengths: a list of term counts to cycle through instead) over distinct directions.  Term 0 is
    always an all-term; by query number mod 4 the rest is: 0 every term all; 1 the last term over (bound 0, 0.45 or 0.7); 2 the last
    term beyond 0.8; 3 the last term within 0.75 and, from 4 terms on, the one before it over 0.  A query of one term is that all-term."""
    rng = np.random.default_rng(6007 * dirs.shape[1] + 101 * nq + 13 * n_terms + seed)
    out = []
    for c in range(nq):
        m = lengths[c % len(lengths)] if lengths else n_terms
        vecs = term_vectors(dirs, rng.choice(len(dirs), size=m, replace=False), rng)
        q = [(v, "all") for v in vecs]
        if m > 1 and c % 4 == 1:
            q[-1] = (vecs[-1], "over", (0.0, 0.45, 0.7)[(c // 4) % 3])
        elif m > 1 and c % 4 == 2:
            q[-1] = (vecs[-1], "beyond", 0.8)
        elif m > 1 and c % 4 == 3:
            q[-1] = (vecs[-1], "within", 0.75)
            if m >= 4:
                q[-2] = (vecs[-2], "over")
        out.append(q)
    return out


def term_distances(ix, what, allow=None):
    """D row(s) of terms from the index's own single-term results, NaN for a row that is not eligible: vectors [m, dim] through
    range_search at radius 4 (every eligible row is within 4), a stored-row id through search_ids(exclude_self=False) (n <= 1024)."""
    n = len(ix)
    if isinstance(what, (int, np.integer)):
        assert n <= 1024
        dist, ids = ix.search_ids([int(what)], max(n, 1), exclude_self=False, allow=allow)
        D = np.full((1, n), np.nan, dtype=np.float32)
        D[0, ids[0][ids[0] >= 0]] = dist[0][ids[0] >= 0]
        return D
    vecs = np.ascontiguousarray(what, dtype=np.float32).reshape(-1, ix.dim)
    lims, dist, ids = ix.range_search(vecs, 4.0, allow=allow)
    D = np.full((len(vecs), n), np.nan, dtype=np.float32)
    for t in range(len(vecs)):
        D[t, ids[lims[t]:lims[t + 1]]] = dist[lims[t]:lims[t + 1]]
    return D


def query_arrays(query):
    """(whats, kinds, bounds) of one compound query in the form of Index.search_compound"""
    whats = [term[0] for term in query]
    kinds = [KINDS[term[1]] for term in query]
    bounds = [np.float32(term[2]) if len(term) == 3 else np.float32(0) for term in query]
    return whats, kinds, bounds


def query_matrix(ix, query, allow=None):
    """D [terms, n] of one compound query: the vector terms in one range_search call, the id terms one search_ids call each"""
    whats, _, _ = query_arrays(query)
    D = np.empty((len(whats), len(ix)), dtype=np.float32)
    vec = [t for t, w in enumerate(whats) if not isinstance(w, (int, np.integer))]
    if vec:
        D[vec] = term_distances(ix, np.stack([whats[t] for t in vec]), allow)
    for t, w in enumerate(whats):
        if t not in vec:
            D[t] = term_distances(ix, w, allow)[0]
    return D


def flatten(queries, dim):
    """(terms f32 [total, dim], term_ids int64 [total], kinds int32 [total], bounds f32 [total], term_lims int64 [nq + 1]): the arrays of
    clip_amd_index_search_compound for a list of compound queries; an id term's vector is zeros"""
    terms, term_ids, kinds, bounds, lims = [], [], [], [], [0]
    for query in queries:
        whats, kk, bb = query_arrays(query)
        for w in whats:
            is_id = isinstance(w, (int, np.integer))
            term_ids.append(int(w) if is_id else -1)
            terms.append(np.zeros(dim, dtype=np.float32) if is_id else np.asarray(w, dtype=np.float32))
        kinds.extend(kk)
        bounds.extend(bb)
        lims.append(len(kinds))
    return (np.ascontiguousarray(np.stack(terms), dtype=np.float32).reshape(-1, dim), np.asarray(term_ids, dtype=np.int64),
            np.asarray(kinds, dtype=np.int32), np.asarray(bounds, dtype=np.float32), np.asarray(lims, dtype=np.int64))


def oracle(ix, queries, k, allow=None, exclude_terms=True):
    """(distances [nq, k], ids [nq, k]) of the definition over the index's own single-term distances: every vector term of the call in
    one range_search, every distinct id term in one search_ids"""
    terms, term_ids, kinds, bounds, lims = flatten(queries, ix.dim)
    D = np.empty((len(kinds), len(ix)), dtype=np.float32)
    vec = np.flatnonzero(term_ids < 0)
    if vec.size:
        D[vec] = term_distances(ix, terms[vec], allow)
    by_id = {}
    for t in np.flatnonzero(term_ids >= 0):
        if int(term_ids[t]) not in by_id:
            by_id[int(term_ids[t])] = term_distances(ix, int(term_ids[t]), allow)[0]
        D[t] = by_id[int(term_ids[t])]
    dist = np.empty((len(queries), k), dtype=np.float32)
    ids = np.empty((len(queries), k), dtype=np.int64)
    for c in range(len(queries)):
        t0, t1 = lims[c], lims[c + 1]
        excluded = term_ids[t0:t1][term_ids[t0:t1] >= 0] if exclude_terms else []
        dist[c], ids[c] = compound(D[t0:t1], kinds[t0:t1], bounds[t0:t1], k, excluded)
    return dist, ids


def same(a, b):
    """two (distances, ids) results are the same bits"""
    return (a[0].shape == b[0].shape and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint32), np.ascontiguousarray(b[0]).view(np.uint32))
            and np.array_equal(a[1], b[1]))
