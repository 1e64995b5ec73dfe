"""k-NN voting over the exact index (clip_amd_index_vote / _vote_graph, k_vote.hip) against the searches it contains and against the
composition a caller had before it.

    python scripts/vote_bench.py [--quick] [--repeats N] [--out FILE]

Writes tables plus one JSON line to FILE (default profiles/vote_bench.txt) and to stdout.  Setting: dim 512, 64 classes, every row labelled
(a seeded hash of the row number in section 1, seeded random labels in sections 2 and 3), seeded random rows.
  1  vote_graph against the knn_graph call it contains, both with their results on the host: clip_amd_bench_vote_graph against
     clip_amd_bench_knn over the same seeded rows, wall time of one synchronous call after one warm call.  N = 65 536 on both routes,
     N = 1 048 576 on the tiled route (the scan route is not run there: profiles/knn_bench.txt has it 20x and more behind at that size).
  2  Index.vote_graph against Index.knn_graph plus a vectorised numpy fold (votes by bincount, first ranks by one assignment per rank,
     the m best by argsort): what a caller composed before.  Wall time of the Python calls.  N = 1 048 576 is measured at k = 16 only: at
     k = 128 the k-NN graph alone is 1.5 GB of results on the host.
  3  Index.vote of 256 vector queries over 1 048 576 rows against Index.search(allow=voters) with the same k: wall time of the Python calls.
Medians of --repeats interleaved measurements (one at N = 1 048 576 in section 1).  One process; run it under a time limit of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import synth           # noqa: E402

DIM = 512
CLASSES = 64
BIG = 1 << 20


def numpy_fold(ids, labels, m):
    """the vote of every row of a k-NN graph (ids [n, k], -1 padded), vectorised: (classes, votes, first ranks) [n, m]"""
    n, k = ids.shape
    cls = np.where(ids >= 0, labels[np.maximum(ids, 0)], CLASSES)      # an empty slot votes for a class of its own, dropped below
    rows = np.repeat(np.arange(n), k)
    votes = np.bincount(rows * (CLASSES + 1) + cls.ravel(), minlength=n * (CLASSES + 1)).reshape(n, CLASSES + 1)[:, :CLASSES]
    first = np.full((n, CLASSES + 1), k, dtype=np.int64)
    r = np.arange(n)
    for rank in range(k - 1, -1, -1):
        first[r, cls[:, rank]] = rank
    first = first[:, :CLASSES]
    best = np.argsort(first - votes * (k + 1), axis=1, kind="stable")[:, :m]
    return best, np.take_along_axis(votes, best, axis=1), np.take_along_axis(first, best, axis=1)


def wall(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vote_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    sizes = [1 << 16] if a.quick else [1 << 16, BIG]
    emit("# python scripts/vote_bench.py --repeats %d%s (MI355X, gfx950): k-NN voting over the exact index (k_vote.hip); dim %d, %d classes,"
         % (a.repeats, " --quick" if a.quick else "", DIM, CLASSES))
    emit("# every row labelled, seeded random rows; microseconds, medians of %d interleaved measurements (1 at N = %d in section 1)." % (a.repeats, BIG))
    emit("# 1: vote_graph against the knn_graph it contains (clip_amd_bench_vote_graph, clip_amd_bench_knn: wall time of one synchronous call with")
    emit("#    the results copied to the host, after one warm call; vote - knn is what the fold and the smaller copy change)")
    emit("%-4s %8s %4s %2s %-6s %12s %12s %12s %8s" % ("dt", "N", "k", "m", "route", "vote_us", "knn_us", "vote-knn", "vote/knn"))
    graph = []
    for dt in ("f16", "i8"):
        for n in sizes:
            for k in (16, 128):
                for route in ((1, 2) if n < BIG else (2,)):
                    reps = 1 if n >= BIG else a.repeats
                    iters = 1 if n >= BIG else 2
                    knn, vote = [], {1: [], 3: []}
                    for _ in range(reps):
                        knn.append(clip_cpp_amd.bench_knn(dt, n, DIM, k, route, iters))
                        for m in (1, 3):
                            vote[m].append(clip_cpp_amd.bench_vote_graph(dt, n, DIM, k, m, CLASSES, route, iters))
                    kn = statistics.median(knn)
                    for m in (1, 3):
                        v = statistics.median(vote[m])
                        graph.append(dict(dtype=dt, n=n, k=k, m=m, route="scan" if route == 1 else "tiled", vote_us=round(v, 1), knn_us=round(kn, 1),
                                          ratio=round(v / kn, 3) if kn > 0 and v > 0 else None))
                        emit("%-4s %8d %4d %2d %-6s %12.1f %12.1f %12.1f %7.3fx" % (dt, n, k, m, graph[-1]["route"], v, kn, v - kn, v / kn if kn > 0 else 0))
                    flush_out()
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    rng = np.random.default_rng(7)
    emit("# 2: Index.vote_graph against Index.knn_graph + a vectorised numpy fold (wall time of the Python calls, automatic route)")
    emit("# 3: Index.vote of 256 vector queries against Index.search(allow=voters), N = %d (wall time of the Python calls)" % BIG)
    emit("%-4s %8s %4s %2s %12s %12s %12s %12s %8s" % ("dt", "N", "k", "m", "vote_us", "knn_us", "fold_us", "knn+fold", "x vote"))
    composed, queries = [], []
    q = rng.standard_normal((256, DIM), dtype=np.float32)
    for dt in ("f16", "i8"):
        for n in sizes:
            index = clip_cpp_amd.Index(clip, DIM, dt)
            for r0 in range(0, n, 65536):
                index.add(rng.standard_normal((min(65536, n - r0), DIM), dtype=np.float32))
            labels = rng.integers(0, CLASSES, size=n).astype(np.int32)
            index.vote_graph(16, labels, m=1)                 # warm: workspaces
            for k in ((16, 128) if n < BIG else (16,)):
                for m in (1, 3):
                    vs, ks, fs = [], [], []
                    for _ in range(a.repeats if n < BIG else 1):
                        vs.append(wall(lambda: index.vote_graph(k, labels, m=m)))
                        t0 = time.perf_counter()
                        _, ids = index.knn_graph(k)
                        t1 = time.perf_counter()
                        numpy_fold(ids, labels, m)
                        t2 = time.perf_counter()
                        ks.append((t1 - t0) * 1e6)
                        fs.append((t2 - t1) * 1e6)
                        del ids
                    v, kn, fo = statistics.median(vs), statistics.median(ks), statistics.median(fs)
                    composed.append(dict(dtype=dt, n=n, k=k, m=m, vote_us=round(v, 1), knn_us=round(kn, 1), fold_us=round(fo, 1), speedup=round((kn + fo) / v, 2)))
                    emit("%-4s %8d %4d %2d %12.1f %12.1f %12.1f %12.1f %7.2fx" % (dt, n, k, m, v, kn, fo, kn + fo, (kn + fo) / v))
                    flush_out()
            if n >= BIG:
                voters = np.ones(n, dtype=np.bool_)
                for k in (16, 128):
                    for m in (1, 3):
                        index.vote(q, k, labels, m=m)
                        index.search(q, k, allow=voters)
                        vs, ss = [], []
                        for _ in range(a.repeats):
                            vs.append(wall(lambda: index.vote(q, k, labels, m=m)))
                            ss.append(wall(lambda: index.search(q, k, allow=voters)))
                        v, s = statistics.median(vs), statistics.median(ss)
                        queries.append(dict(dtype=dt, n=n, k=k, m=m, vote_us=round(v, 1), search_us=round(s, 1), ratio=round(v / s, 3)))
            index.close()
    emit("%-4s %8s %4s %2s %12s %12s %8s" % ("dt", "N", "k", "m", "vote_us", "search_us", "vote/srch"))
    for r in queries:
        emit("%-4s %8d %4d %2d %12.1f %12.1f %7.3fx" % (r["dtype"], r["n"], r["k"], r["m"], r["vote_us"], r["search_us"], r["ratio"]))
    clip.close()
    emit(json.dumps(dict(graph=graph, composed=composed, queries=queries)))
    flush_out()


if __name__ == "__main__":
    main()
