"""One exact index searched with the rows of another (clip_amd_index_search_index through clip_amd_bench_cross): the tiled route (the CROSS
instantiations of k_graph.hip) against the scan route (rows gathered from the second store, then the scan of k_search.hip), and against
what a caller who had kept the f32 vectors on the device could do today, clip_amd_index_search_device.

    python scripts/cross_bench.py [--quick] [--reps N] [--out FILE]

Writes a table plus one JSON line to FILE (default profiles/cross_bench.txt) and to stdout, line by line as it goes.  Seeded random rows,
dim 512, every dtype.  Per shape:
  tiled_us / scan_us   median over --reps measurements, the two routes alternated, of the wall time of one synchronous
                       clip_amd_index_search_index with ids == NULL (scoring, selection, merge, results copied to the host block by block);
                       every measurement builds both indexes, makes one warm call and times the next
  device_us            the baseline: median over --reps of clip_amd_bench_search, the device time (HIP events) of one
                       clip_amd_index_search_device of as many f32 queries already on the device: it normalises / quantises them and
                       leaves the results on the device, so it has no copy to the host in it and the two routes do
  TFLOP/s              rows x queries x 2 x Dpad over tiled_us: an end-to-end rate, not a kernel's
Sections: "label" (256 and 1024 index rows x 10^5 and 10^6 queries, k 5), "merge" (10^6 index rows x 10^5 queries, k 1) and "crossover" (a
sweep of the query count at index sizes 256, 1024 and 10^6, both routes): the crossover of an index size is the smallest swept query
count from which on the tiled route's median is below the scan route's on every dtype; CROSS_TILED_MIN_QUERIES in search.cpp is the
largest of them.  One process; run it under a time limit of its own.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402

DTYPES = ("f16", "i8", "f32")
DIM = 512


def dpad(dtype, dim):
    return (dim + 63) // 64 * 64 if dtype == "i8" else (dim + 31) // 32 * 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")

    def emit(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    def routes(dt, rows, nq, k):
        """(median tiled us, median scan us), alternated"""
        t, s = [], []
        for _ in range(a.reps):
            t.append(clip_cpp_amd.bench_cross(dt, rows, nq, DIM, k, 2, 1))
            s.append(clip_cpp_amd.bench_cross(dt, rows, nq, DIM, k, 1, 1))
        if min(t + s) < 0:
            raise RuntimeError("clip_amd_bench_cross failed: %r %r" % (t, s))
        return statistics.median(t), statistics.median(s)

    emit("# python scripts/cross_bench.py --reps %d%s (MI355X, gfx950): one exact index searched with the rows of another" % (a.reps, " --quick" if a.quick else ""))
    emit("# (clip_amd_index_search_index, ids == NULL; dim %d).  tiled_us / scan_us: median of %d wall times of one synchronous call, results" % (DIM, a.reps))
    emit("# copied to the host, each after a warm call, the two routes alternated.  device_us: median of %d clip_amd_bench_search, the device" % a.reps)
    emit("# time of clip_amd_index_search_device of as many f32 queries already on the device, results left there (no host copy in it).")
    emit("# TFLOP/s: rows x queries x 2 x Dpad over tiled_us, end to end.")
    label = [(dt, rows, nq, 5) for dt in DTYPES for rows in (256, 1024) for nq in (100000, 1000000)]
    merge = [(dt, 1000000, 100000, 1) for dt in DTYPES]
    sweeps = [(256, 5, [128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]),
              (1024, 5, [128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]),
              (1000000, 1, [128, 256, 512, 1024, 2048, 4096, 8192])]
    if a.quick:
        label, merge = label[:1], []
        sweeps = [(256, 5, [128, 4096])]
    rows_out = []
    for name, shapes in (("label", label), ("merge", merge)):
        emit("# %s" % name)
        emit("%-4s %8s %8s %3s %12s %9s %12s %12s %9s %9s" % ("dt", "rows", "queries", "k", "tiled_us", "TFLOP/s", "scan_us", "device_us", "scan/tiled",
                                                              "dev/tiled"))
        for dt, rows, nq, k in shapes:
            t, s = routes(dt, rows, nq, k)
            d = statistics.median([clip_cpp_amd.bench_search(dt, rows, DIM, nq, k, 1) for _ in range(a.reps)])
            r = dict(section=name, dtype=dt, rows=rows, queries=nq, k=k, tiled_us=round(t, 1), scan_us=round(s, 1), device_us=round(d, 1),
                     tflops=round(rows * nq * 2.0 * dpad(dt, DIM) / t / 1e6, 1))
            rows_out.append(r)
            emit("%-4s %8d %8d %3d %12.1f %9.1f %12.1f %12.1f %8.2fx %8.2fx" % (dt, rows, nq, k, t, r["tflops"], s, d, s / t, d / t))
    emit("# crossover: both routes, per index size a sweep of the query count")
    emit("%-4s %8s %8s %3s %12s %12s" % ("dt", "rows", "queries", "k", "tiled_us", "scan_us"))
    sweep_out, constants = [], {}
    for rows, k, counts in sweeps:
        wins = {nq: True for nq in counts}
        for dt in DTYPES:
            for nq in counts:
                t, s = routes(dt, rows, nq, k)
                sweep_out.append(dict(dtype=dt, rows=rows, queries=nq, k=k, tiled_us=round(t, 1), scan_us=round(s, 1)))
                wins[nq] = wins[nq] and t < s
                emit("%-4s %8d %8d %3d %12.1f %12.1f" % (dt, rows, nq, k, t, s))
        first = None                                               # the smallest count from which on the tiled route wins on every dtype
        for nq in reversed(counts):
            if not wins[nq]:
                break
            first = nq
        constants[rows] = first
        emit("# index of %d rows: %s" % (rows, "the tiled route wins on every dtype from %d queries on" % first if first else
                                          "the tiled route does not win on every dtype at the largest swept count: automatic stays on the scan route"))
    if all(constants.values()):
        emit("# CROSS_TILED_MIN_QUERIES (search.cpp) is the largest of these: %d" % max(constants.values()))
    emit(json.dumps(dict(rows=rows_out, crossover=sweep_out, constants=constants)))
    out.close()


if __name__ == "__main__":
    main()
