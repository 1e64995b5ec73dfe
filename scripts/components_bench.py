"""Connected components of the exact index (k_components.hip, clip_amd_index_components) against the routes there were, measured in one run.

    python scripts/components_bench.py [--quick] [--reps N] [--parent-lib PATH/libclip.so]

1. sparse   the data of scripts/pairs_bench.py (seeded random rows, every 64th a perturbation of an earlier one: N / 64 pairs), radius
            0.05, dim 512, f16 and i8, N = 65 536 and 262 144: clip_amd_bench_components against clip_amd_bench_range (pairs) of this
            build and, with --parent-lib, of the parent commit's library loaded next to it.  The same scoring pass; components drops the
            counts to the host, scatter and sort and adds the init, flatten and finish launches.
2. dense    N = 65 536 rows in bursts of 64 / 256 / 1024 noisy copies (radius 0.05: every pair of a burst is near), through a real Index:
            Index.components against Index.pairs + image_search.duplicate_groups (the route `dedup` had; both parts timed) and against
            Index.pairs + scipy connected_components (a vectorised host union), with the pair count, the bytes each route returns and
            whether pairs needed its second scoring pass (more than 2^21 pairs).
3. callers  pairs and range_search (nq 1024) at 65 536 x 512 f16 of this build against the parent's (--parent-lib): the shared tile body
            must have cost them nothing.

Every time is the wall time of the synchronous host call in microseconds.  A figure is the median of --reps repetitions (each the hook's
mean over its own iterations) with (min ... max) behind it, the repetitions of the things compared taken in turn.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import image_search, synth  # noqa: E402

RADIUS = 0.05
HIT_BUDGET = 1 << 21            # search.cpp JOIN_HIT_BUDGET: pairs scores a second time above it
DT = {"f32": 0, "f16": 1, "i8": 3}


def parent_range(path):
    """clip_amd_bench_range of another build of the library (the parent commit's), or None"""
    if not path:
        return None
    L = C.CDLL(path)
    L.clip_amd_bench_range.restype = C.c_float
    L.clip_amd_bench_range.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int]
    return lambda dt, n, dim, nq, r, iters: float(L.clip_amd_bench_range(DT[dt], n, dim, nq, r, iters))


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"]) if s else "         -"


def in_turn(calls, reps):
    """{name: stats} of the named calls, repetition by repetition in turn"""
    got = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            us = f()
            if us < 0:
                raise RuntimeError("%s failed: %s" % (k, us))
            got[k].append(us)
    return {k: stats(v) for k, v in got.items()}


def wall(f, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return out, stats(ts)


def burst_rows(rng, n, dim, burst):
    base = rng.standard_normal((n // burst, dim), dtype=np.float32)
    return np.repeat(base, burst, axis=0) + 0.05 * rng.standard_normal((n, dim), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    torch.cuda.init()
    parent = parent_range(a.parent_lib)
    rows = []

    print("# 1. sparse: N / 64 pairs, dim 512, radius %g; us per call, median (min ... max) of %d repetitions" % (RADIUS, a.reps))
    print("%-4s %8s %32s %32s %32s %8s" % ("dt", "N", "components", "pairs", "pairs (parent build)", "c / p"))
    for dt in ("f16", "i8"):
        for n in (1 << 16,) if a.quick else (1 << 16, 1 << 18):
            calls = {"components": lambda: clip_cpp_amd.bench_components(dt, n, 512, RADIUS, a.iters),
                     "pairs": lambda: clip_cpp_amd.bench_range(dt, n, 512, 0, RADIUS, a.iters)}
            if parent:
                calls["pairs_parent"] = lambda: parent(dt, n, 512, 0, RADIUS, a.iters)
            s = in_turn(calls, a.reps)
            yard = s.get("pairs_parent", s["pairs"])
            ratio = s["components"]["median"] / yard["median"]
            rows.append(dict(kind="sparse", dtype=dt, n=n, ratio=round(ratio, 4), **s))
            print("%-4s %8d %32s %32s %32s %8.4f" % (dt, n, fmt(s["components"]), fmt(s["pairs"]), fmt(s.get("pairs_parent")), ratio), flush=True)

    print("\n# 3. existing callers at 65 536 x 512 f16, this build against the parent's; us per call")
    print("%-14s %32s %32s %8s" % ("call", "this build", "parent build", "ratio"))
    for name, nq in (("pairs", 0), ("range nq=1024", 1024)):
        calls = {"now": lambda: clip_cpp_amd.bench_range("f16", 1 << 16, 512, nq, RADIUS, max(a.iters, 5))}
        if parent:
            calls["parent"] = lambda: parent("f16", 1 << 16, 512, nq, RADIUS, max(a.iters, 5))
        s = in_turn(calls, a.reps)
        ratio = s["now"]["median"] / s["parent"]["median"] if parent else float("nan")
        rows.append(dict(kind="callers", call=name, ratio=round(ratio, 4) if parent else None, **s))
        print("%-14s %32s %32s %8.4f" % (name, fmt(s["now"]), fmt(s.get("parent")), ratio), flush=True)
    print("\n# 2. dense: N = 65 536, dim 512, bursts of noisy copies, radius %g; us per call through Index (results on the host)" % RADIUS)
    print("%-4s %6s %10s %5s %26s %26s %14s %14s %12s %12s" % ("dt", "burst", "pairs", "2nd", "components", "pairs", "dup_groups", "scipy union",
                                                                "bytes comp", "bytes pairs"))
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    n, dim = 1 << 16, 512
    for dt in ("f16",) if a.quick else ("f16", "i8"):
        for burst in (64, 256, 1024):
            ix = clip_cpp_amd.Index(clip, dim, dt)
            ix.add(burst_rows(np.random.default_rng(burst), n, dim, burst))
            ix.components(RADIUS)                   # warm: workspaces, code objects
            (labels, near, nid), tc = wall(lambda: ix.components(RADIUS), a.reps)
            ix.pairs(RADIUS)
            (i, j, d), tp = wall(lambda: ix.pairs(RADIUS), 2)
            groups, tg = wall(lambda: image_search.duplicate_groups(i, j, d), 1)

            def union():
                k, comp = connected_components(coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(n, n)).tocsr(), directed=False)
                return k - int(np.count_nonzero(np.bincount(comp) == 1))
            k, ts = wall(union, 1)
            got = image_search.component_groups(labels, near)
            assert got == groups and len(groups) == k, "the routes disagree"
            r = dict(kind="dense", dtype=dt, burst=burst, pairs=int(len(i)), second_pass=bool(len(i) > HIT_BUDGET), groups=len(groups),
                     components=tc, pairs_us=tp, duplicate_groups_us=tg, scipy_union_us=ts, bytes_components=20 * n,
                     bytes_pairs=int(16 * len(i) + 8 * (n + 1)))
            rows.append(r)
            print("%-4s %6d %10d %5s %26s %26s %14.1f %14.1f %12d %12d" % (dt, burst, len(i), "yes" if r["second_pass"] else "no", fmt(tc), fmt(tp),
                                                                           tg["median"], ts["median"], r["bytes_components"], r["bytes_pairs"]),
                  flush=True)
            del i, j, d, groups
            ix.close()
    clip.close()

    print(json.dumps(dict(radius=RADIUS, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
