"""Shared pieces of the removal / compaction / subset-search tests of the exact index (not a test module).

Notation of those tests: X = the index under test holding rows R; E = the eligible rows (live and allowed); Y = a fresh index of R[E]
added in order; m = the increasing map from Y's ids to X's.  Every (query, row) distance is bit-identical however rows are tiled, so X
restricted to E must return exactly what Y returns, ids mapped through m."""
import ctypes as C

import numpy as np

DTYPES = ["f16", "f32", "i8"]
WAYS = ["remove", "allow", "both"]


def open_clip(clip_lib, fixture_cache):
    from oracle import fixtures
    assert clip_lib.device_count() >= 1, "no HIP device"
    return clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)


def eligible_sets(n, seed=0):
    """name -> bool [n]: the eligible sets every test walks through"""
    rng = np.random.default_rng(1000 + seed + n)
    ids = np.arange(n)
    sets = {
        "all": np.ones(n, dtype=bool),
        "none": np.zeros(n, dtype=bool),
        "first": ids == 0,
        "last": ids == n - 1,
        "range37_411": (ids >= 37) & (ids < min(411, n)),          # not aligned to 16
        "alternate16": (ids // 16) % 2 == 0,                       # whole 16-row groups without an eligible row: the skip path
        "random50": rng.random(n) < 0.5,
        "random2": rng.random(n) < 0.02,
    }
    return sets


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def stray_words(clip_lib, mask):
    """the uint64 words of a bool mask with every bit at a position >= len(mask) set to 1"""
    n = len(mask)
    w = clip_lib.allow_words(mask, n).copy()
    if n % 64:
        w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return w


def make_x(clip_lib, clip, rows, dtype, elig, way):
    """(X, allow): X holds `rows` (two add calls); the rows outside `elig` are excluded by removal, by the returned allow mask, or half
    each way ("both": the allow mask then also allows the removed rows, which must not bring them back)."""
    n = len(rows)
    x = clip_lib.Index(clip, rows.shape[1], dtype)
    cut = n // 3
    x.add(rows[:cut])
    x.add(rows[cut:])
    out = np.flatnonzero(~elig)
    allow = None
    if way == "remove":
        rem = out
    elif way == "allow":
        rem = out[:0]
        allow = elig.copy()
    else:
        rem = out[::2]
        allow = elig.copy()
        allow[rem] = True
    if len(rem):
        assert x.remove(rem) == len(rem)
    assert len(x) == n and x.live == n - len(rem)
    return x, allow


def make_y(clip_lib, clip, rows, dtype, elig):
    """(Y, m with -1 appended so that m[-1] == -1 maps the empty id)"""
    y = clip_lib.Index(clip, rows.shape[1], dtype)
    if elig.any():
        y.add(rows[elig])
    return y, np.append(np.flatnonzero(elig), -1).astype(np.int64)


def raw_search_subset(clip_lib, ix, q, k, words):
    q = np.ascontiguousarray(q, dtype=np.float32)
    dist = np.empty((len(q), k), dtype=np.float32)
    ids = np.empty((len(q), k), dtype=np.int64)
    assert clip_lib.lib().clip_amd_index_search_subset(ix.handle, fp(q), len(q), k, up(words) if words is not None else None, fp(dist), ip(ids))
    return dist, ids


def raw_range_subset(clip_lib, ix, q, radius, words, capacity):
    """(total, lims, distances, ids) of one clip_amd_index_range_search_subset call with the given capacity (0: count only)"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    lims = np.full(len(q) + 1, -7, dtype=np.int64)
    dist = np.empty(max(capacity, 1), dtype=np.float32)
    ids = np.empty(max(capacity, 1), dtype=np.int64)
    total = clip_lib.lib().clip_amd_index_range_search_subset(ix.handle, fp(q), len(q), float(radius), up(words) if words is not None else None,
                                                              ip(lims), fp(dist) if capacity else None, ip(ids) if capacity else None, capacity)
    return int(total), lims, dist[:max(min(total, capacity), 0)], ids[:max(min(total, capacity), 0)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
