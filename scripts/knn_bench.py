"""The k-NN graph of the exact index (clip_amd_index_knn_graph through clip_amd_bench_knn): the tiled kernel of k_graph.hip against the scan
route and two yardsticks that are not the code under test.

    python scripts/knn_bench.py [--quick] [--iters N] [--out FILE]

Writes a table plus one JSON line to FILE (default profiles/knn_bench.txt) and to stdout.  Per shape (seeded random rows):
  tiled_us   wall time of one synchronous clip_amd_index_knn_graph on the tiled route (scoring, selection, merge, results copied to the
             host block by block), after one warm call; --iters calls, one at N = 1 M
  TFLOP/s    n^2 x 2 x Dpad over that time
  scan_us    the scan route: measured the same way (route 1) up to N = 65 536 ("direct"); above, clip_amd_bench_search of 1024 queries at
             the same k over 1 M rows of the same dtype and dim, scaled to n queries over n rows ("scaled": the scan is linear in both,
             the way pairs_bench.py forms its route_us)
  parent_us  yardstick (a), the route of the parent commit: clip_amd_bench_search at k + 1 (k = 1024 has none), 1024 queries, scaled to n
             queries over n rows; device time, without the host-side filter of the self hit
  2pairs_us  yardstick (b): twice the pairs line of the same shape in profiles/pairs_bench.txt, the same tile engine over the full square
             without any selection
The section "crossover" measures both routes directly at small N (f16, dim 512, k = 10) for the constant of the automatic route.
One process; run it under a time limit of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402


def dpad(dtype, dim):
    return (dim + 63) // 64 * 64 if dtype == "i8" else (dim + 31) // 32 * 32


def pairs_lines():
    """{(dtype, n, dim): us} of the pairs rows of profiles/pairs_bench.txt"""
    out = {}
    try:
        with open(os.path.join(ROOT, "profiles", "pairs_bench.txt")) as f:
            for line in f:
                if line.startswith("{"):
                    for r in json.loads(line)["rows"]:
                        if r["kind"] == "pairs":
                            out[(r["dtype"], r["n"], r["dim"])] = r["us"]
    except OSError:
        pass
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python scripts/knn_bench.py --iters %d%s (MI355X, gfx950): the k-NN graph of the exact index (clip_amd_bench_knn, k_graph.hip)."
         % (a.iters, " --quick" if a.quick else ""))
    emit("# tiled_us / direct scan_us: wall time of one synchronous clip_amd_index_knn_graph, results copied to the host, after one warm call")
    emit("# (%d timed calls, 1 at N = 1 M); TFLOP/s = n^2 x 2 x Dpad over tiled_us.  scaled scan_us and parent_us: clip_amd_bench_search (device" % a.iters)
    emit("# time) of 1024 queries at k resp. k + 1 over 1 M rows of the same dtype and dim, scaled to n queries over n rows.  2pairs_us: twice the")
    emit("# pairs line of the same shape in profiles/pairs_bench.txt (the tile engine over the full square, no selection).")
    shapes = [(dt, n, dim, k) for dt in ("f16", "i8", "f32") for n in (1 << 16, 1 << 18, 1 << 20) for dim in (512, 768) for k in (10, 100)
              if not (dt == "f32" and n > 1 << 18)]
    cross = [512, 1024, 2048, 4096, 8192, 16384, 32768]
    if a.quick:
        shapes = [s for s in shapes if s[1] == 1 << 16 and s[2] == 512 and s[3] == 10]
        cross = [1024, 4096]
    pairs = pairs_lines()
    per_row = {}

    def search_us_per_query_row(dt, dim, k):
        key = (dt, dim, k)
        if key not in per_row:
            per_row[key] = clip_cpp_amd.bench_search(dt, 1 << 20, dim, 1024, k, 2) / 1024.0 / float(1 << 20)
        return per_row[key]

    rows = []
    emit("%-4s %8s %5s %5s %12s %9s %12s %-7s %12s %12s %9s %9s" % ("dt", "N", "dim", "k", "tiled_us", "TFLOP/s", "scan_us", "scan", "parent_us",
                                                                    "2pairs_us", "vs_parent", "vs_2pairs"))
    for dt, n, dim, k in shapes:
        iters = 1 if n >= 1 << 20 else a.iters
        tiled = clip_cpp_amd.bench_knn(dt, n, dim, k, 2, iters)
        if n <= 1 << 16:
            scan, how = clip_cpp_amd.bench_knn(dt, n, dim, k, 1, iters), "direct"
        else:
            scan, how = search_us_per_query_row(dt, dim, k) * n * n, "scaled"
        parent = search_us_per_query_row(dt, dim, k + 1) * n * n
        two = 2.0 * pairs.get((dt, n, dim), -0.5)
        r = dict(dtype=dt, n=n, dim=dim, k=k, tiled_us=round(tiled, 1), tflops=round(n * n * 2.0 * dpad(dt, dim) / tiled / 1e6, 1) if tiled > 0 else None,
                 scan_us=round(scan, 1), scan_how=how, parent_us=round(parent, 1), two_pairs_us=round(two, 1),
                 parent_over_tiled=round(parent / tiled, 2) if tiled > 0 else None, tiled_over_two_pairs=round(tiled / two, 2) if two > 0 and tiled > 0 else None)
        rows.append(r)
        emit("%-4s %8d %5d %5d %12.1f %9.1f %12.1f %-7s %12.1f %12.1f %8.2fx %8.2fx" % (dt, n, dim, k, tiled, r["tflops"] or 0, scan, how, parent, two,
                                                                                     r["parent_over_tiled"] or 0, r["tiled_over_two_pairs"] or 0))
    emit("# crossover: f16, dim 512, k = 10, both routes direct")
    emit("%-4s %8s %12s %12s" % ("dt", "N", "tiled_us", "scan_us"))
    crossover = []
    for n in cross:
        t, s = clip_cpp_amd.bench_knn("f16", n, 512, 10, 2, 5), clip_cpp_amd.bench_knn("f16", n, 512, 10, 1, 5)
        crossover.append(dict(n=n, tiled_us=round(t, 1), scan_us=round(s, 1)))
        emit("%-4s %8d %12.1f %12.1f" % ("f16", n, t, s))
    emit(json.dumps(dict(rows=rows, crossover=crossover)))
    ok = [r for r in rows if r["tiled_us"] > 0]
    slower = [r for r in ok if r["tiled_us"] >= r["parent_us"]]
    emit("")
    emit("# Goals of the issue:")
    emit("#   the tiled route is faster than the parent's route (a) at every measured N >= 65 536:  %s (%d of %d shapes; parent / tiled %.1fx ... %.1fx)"
         % ("MET" if ok and not slower and len(ok) == len(rows) else "NOT MET", len(ok) - len(slower), len(rows),
            min([r["parent_over_tiled"] for r in ok] or [0]), max([r["parent_over_tiled"] for r in ok] or [0])))
    with_b = [r for r in ok if r["tiled_over_two_pairs"]]
    emit("#   distance from the floor (b), tiled / (2 x pairs):  %.2fx ... %.2fx over %d shapes"
         % (min([r["tiled_over_two_pairs"] for r in with_b] or [0]), max([r["tiled_over_two_pairs"] for r in with_b] or [0]), len(with_b)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
