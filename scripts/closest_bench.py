"""Closest pairs (k_closest.hip, clip_amd_index_closest_pairs) against what it is built on and what it replaces, measured in one run.

    python scripts/closest_bench.py [--quick] [--reps N] [--out FILE]

Rows: dim 512, 65 536 and 262 144 of them (--quick: the first only), f16 and i8, "sparse" (independent random rows: no two are near) and
"bursts" (64 noisy copies of each base row, in row order).  Per index and n_pairs in {16, 1024}:
  closest     Index.closest_pairs(n_pairs)
  components  Index.components(0.05) on the same index: the same tile loop with an almost empty ending
  knn + sort  at 65 536 rows only: Index.knn_graph(n_pairs) (size x n_pairs results to the host) and the host selection of the n_pairs best
              pairs from it, the exact route there was; its result must equal closest_pairs bit for bit.

Every time is the wall time of the synchronous host call in microseconds, after a warm call of the same shape.  A figure is the median
of --reps repetitions with (min ... max) behind it, the repetitions of the things compared taken in turn.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import synth  # noqa: E402

RADIUS = 0.05
KNN_ROWS = 1 << 16


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"]) if s else "not measured"


def in_turn(calls, reps):
    """{name: stats of the wall time} of the named calls: one warm call each, then repetition by repetition in turn"""
    for f in calls.values():
        f()
    got = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            got[k].append((time.perf_counter() - t0) * 1e6)
    return {k: stats(v) for k, v in got.items()}


def make_rows(rng, n, dim, burst):
    rows = np.repeat(rng.standard_normal((n // burst, dim), dtype=np.float32), burst, axis=0)
    for r0 in range(0, n, 1 << 14) if burst > 1 else ():    # the noise in pieces: no second array of the whole size
        rows[r0:r0 + (1 << 14)] += 0.05 * rng.standard_normal((min(1 << 14, n - r0), dim), dtype=np.float32)
    return rows


def from_graph(ix, k):
    """the k closest pairs by the route there was: the k-NN graph on the host, the entries lo < hi, the k best in the order (d, lo, hi)"""
    dist, ids = ix.knn_graph(k)
    row = np.repeat(np.arange(len(ix), dtype=np.int64), k)
    dist, ids = dist.reshape(-1), ids.reshape(-1)
    up = ids > row
    row, ids, dist = row[up], ids[up], dist[up]
    near = np.flatnonzero(dist <= np.partition(dist, k - 1)[k - 1])
    order = near[np.lexsort((ids[near], row[near], dist[near]))[:k]]
    return row[order], ids[order], dist[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    dim = 512
    say("# closest_bench: %s; dim %d; us per synchronous host call, median (min ... max) of %d repetitions taken in turn"
        % (torch.cuda.get_device_name(0), dim, a.reps))
    say("# components at radius %g; knn + sort at %d rows only (one repetition at n_pairs 1024)" % (RADIUS, KNN_ROWS))
    say("%-4s %7s %-7s %7s %34s %34s %34s %7s %9s" % ("dt", "N", "rows", "n_pairs", "closest", "components", "knn_graph + host sort", "c / co", "knn / c"))
    losses = []
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 18):
        for name, burst in (("sparse", 1), ("bursts", 64)):
            rows = make_rows(np.random.default_rng(burst), n, dim, burst)
            for dt in ("f16", "i8"):
                ix = clip_cpp_amd.Index(clip, dim, dt)
                for r0 in range(0, n, 1 << 16):
                    ix.add(rows[r0:r0 + (1 << 16)])
                for k in (16, 1024):
                    s = in_turn({"closest": lambda: ix.closest_pairs(k), "components": lambda: ix.components(RADIUS)}, a.reps)
                    g = None
                    if n == KNN_ROWS:
                        g = in_turn({"graph": lambda: from_graph(ix, k)}, a.reps if k == 16 else 1)["graph"]
                        same = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                                   for x, y in zip(ix.closest_pairs(k), from_graph(ix, k)))
                        assert same, "closest_pairs and the k-NN graph route disagree"
                    over = s["closest"]["median"] / s["components"]["median"]
                    say("%-4s %7d %-7s %7d %34s %34s %34s %7.3f %9s" % (dt, n, name, k, fmt(s["closest"]), fmt(s["components"]), fmt(g), over,
                                                                       "%.1f" % (g["median"] / s["closest"]["median"]) if g else "-"))
                    if g and g["median"] < s["closest"]["median"]:
                        losses.append("%s %d %s n_pairs %d: slower than knn_graph + host sort" % (dt, n, name, k))
                    if over > 1.5:
                        losses.append("%s %d %s n_pairs %d: %.2f x components" % (dt, n, name, k, over))
                ix.close()
            del rows
    say("\n# points where closest_pairs loses (slower than the k-NN graph route, or more than 1.5 x components): %s" % ("; ".join(losses) or "none"))
    clip.close()
    out.close()


if __name__ == "__main__":
    main()
