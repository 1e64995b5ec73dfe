"""Query sets over the exact index: what the set fold costs on top of the scan it contains, and what the only earlier route cost.

    python scripts/sets_bench.py [--repeats 3] [--dtypes f16,f32,i8] [--rows 100000,1000000] [--group-sizes 5,17] [--set-sizes 5,17]
                                 [--n-sets 1,256,4096] [--ks 10,100] [--budget SECONDS] [--out profiles/sets_bench.txt]

Every point (dtype, rows, group size, set size, number of sets, k) at dim 512 records three numbers:
  sets      HIP-event microseconds of one clip_amd_index_search_sets_device (clip_amd_bench_search_sets): seeded random rows, row r in
            group r // group_size, n_sets sets of set_size seeded random query rows each
  grouped   the same for clip_amd_index_search_grouped_device over the same rows and the same n_sets x set_size query rows
            (clip_amd_bench_search_grouped): the scan and merge tree the new call contains, so sets - grouped is the cost of the fold
  host      wall microseconds of the route the library offered before for the same answer: Index.search_grouped with one result row per
            query row, every list copied to the host, and the definition applied per set with numpy (over random rows of the same shape,
            added from the host; the time to add them is not counted)
Medians of --repeats measurements, the three interleaved.  The points are walked cheapest first (by rows x query rows).  With --budget
SECONDS a point is measured only while its predicted time (its rows x query rows at the best rate seen so far, for the 1 + 3 x repeats
searches it takes) fits what is left of the budget; the others are listed as not measured, not estimated."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clip_cpp_amd                      # noqa: E402
from clip_cpp_amd import synth           # noqa: E402

DIM = 512


def host_fold(dist, ids, groups, set_size, k):
    """the definition over the per-row results of search_grouped: (distances, ids, qrows) per set"""
    n_sets = len(ids) // set_size
    out_d = np.full((n_sets, k), np.inf, dtype=np.float32)
    out_i = np.full((n_sets, k), -1, dtype=np.int64)
    out_q = np.full((n_sets, k), -1, dtype=np.int32)
    rowno = np.repeat(np.arange(len(ids)), ids.shape[1]).reshape(ids.shape)
    for s in range(n_sets):
        sl = slice(s * set_size, (s + 1) * set_size)
        d, r, q = dist[sl].ravel(), ids[sl].ravel(), rowno[sl].ravel()
        real = r >= 0
        d, r, q = d[real], r[real], q[real]
        order = np.lexsort((q, r, d))
        d, r, q = d[order], r[order], q[order]
        first = np.sort(np.unique(groups[r], return_index=True)[1])[:k]
        out_d[s, :len(first)], out_i[s, :len(first)], out_q[s, :len(first)] = d[first], r[first], q[first]
    return out_d, out_i, out_q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtypes", default="f16,f32,i8")
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--group-sizes", default="5,17")
    ap.add_argument("--set-sizes", default="5,17")
    ap.add_argument("--n-sets", default="1,256,4096")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--budget", type=float, default=1e9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    points = [(n, ns * ss, dtype, gs, ss, ns, k) for dtype in a.dtypes.split(",") for n in ints(a.rows) for gs in ints(a.group_sizes)
              for ss in ints(a.set_sizes) for ns in ints(a.n_sets) for k in ints(a.ks)]
    points.sort(key=lambda p: (p[0] * p[1], p[0], p[2], p[3:]))
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    say("sets_bench: query sets against the grouped search they contain and against the earlier host route; dim %d, microseconds, medians of %d"
        " interleaved measurements (sets, grouped: HIP events; host: wall)" % (DIM, a.repeats))
    say("  %-5s %8s %6s %5s %6s %4s %12s %12s %10s %8s %14s %8s" % ("dtype", "rows", "group", "set", "n_sets", "k", "sets us", "grouped us",
                                                                   "fold us", "fold %", "host route us", "x sets"))
    t_start = time.perf_counter()
    indexes, skipped, rate = {}, [], 0.0                    # rate: the best (rows x query rows) per second of a sets search so far
    rng = np.random.default_rng(7)
    for n, nq, dtype, gs, ss, ns, k in points:
        left = a.budget - (time.perf_counter() - t_start)
        if left <= 0 or (rate > 0 and (1 + 3 * a.repeats) * n * nq / rate > left):
            skipped.append((dtype, n, gs, ss, ns, k))
            continue
        if (dtype, n) not in indexes:                       # the host route's index: random rows of the same shape, kept for later points
            indexes[(dtype, n)] = clip_cpp_amd.Index(clip, DIM, dtype)
            for r0 in range(0, n, 65536):
                indexes[(dtype, n)].add(rng.standard_normal((min(65536, n - r0), DIM), dtype=np.float32))
        index = indexes[(dtype, n)]
        groups = (np.arange(n) // gs).astype(np.int32)
        q = rng.standard_normal((nq, DIM), dtype=np.float32)
        probe = clip_cpp_amd.bench_search_sets(dtype, n, DIM, ns, ss, k, gs, 1)
        iters = 10 if 0 <= probe < 20000 else (3 if probe < 200000 else 1)
        sets, grouped, host = [], [], []
        for _ in range(a.repeats):
            sets.append(clip_cpp_amd.bench_search_sets(dtype, n, DIM, ns, ss, k, gs, iters))
            grouped.append(clip_cpp_amd.bench_search_grouped(dtype, n, DIM, nq, k, gs, iters))
            t0 = time.perf_counter()
            d, i = index.search_grouped(q, k, groups)
            host_fold(d, i, groups, ss, k)
            host.append((time.perf_counter() - t0) * 1e6)
        if min(sets + grouped) < 0:
            say("  %-5s %8d %6d %5d %6d %4d  a benchmark hook failed: %r" % (dtype, n, gs, ss, ns, k, (sets, grouped)))
            continue
        s, g, h = statistics.median(sets), statistics.median(grouped), statistics.median(host)
        rate = max(rate, n * nq / (s * 1e-6))
        say("  %-5s %8d %6d %5d %6d %4d %12.1f %12.1f %10.1f %7.1f%% %14.1f %7.1fx" % (dtype, n, gs, ss, ns, k, s, g, s - g, 100 * (s - g) / g, h, h / s))
        flush_out()
    for index in indexes.values():
        index.close()
    clip.close()
    if skipped:
        say()
        say("not measured (the --budget of %.0f s was used up): %d points" % (a.budget, len(skipped)))
        for p in skipped:
            say("  %-5s rows %d, groups of %d, sets of %d, %d sets, k %d" % p)
    flush_out()


if __name__ == "__main__":
    main()
