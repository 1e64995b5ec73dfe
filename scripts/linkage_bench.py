"""The single-linkage tree of the exact index (k_linkage.hip, clip_amd_index_linkage) against one connected-components call on the same
rows, measured in one run and written to profiles/linkage_bench.txt (--out).

    python scripts/linkage_bench.py [--quick] [--reps N] [--max-rows N] [--out FILE]

A round of the tree is one sweep over the pairs (the tile loop of `pairs`) plus O(n) work, and `Index.components` is one such sweep with a
union-find as its ending; it exists on the parent commit and is the yardstick.  Per row count (4 096, 65 536, 262 144), dtype (f16, i8)
and data, through a real Index, dim 512:

  sparse    seeded random rows, every 64th a small perturbation of an earlier one (the data of scripts/components_bench.py)
  bursts    groups of 64 noisy copies of one row (the dense data of scripts/modes_bench.py)

  components(R)    one Index.components call at R = 0.05
  linkage(R)       Index.linkage(link = R): the forest at the same radius, the rounds that did work, and
                   ratio = time / (rounds x components time)
  linkage()        the whole tree (link = inf: every pair is near in every round), its rounds and the same ratio

and, over the seeded rows of clip_amd_bench_modes, clip_amd_bench_linkage (the whole tree) against clip_amd_bench_components.
The forest at R is checked against components(R) on the way (cut_linkage of the edges = the labels).

Every time is the wall time of the synchronous host call in microseconds: the median of --reps calls with (min ... max) behind it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libclip.so: tests/conftest.py says why)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import synth  # noqa: E402

RADIUS = 0.05
DIM = 512


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%12.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def wall(f, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return out, stats(ts)


def sparse_rows(rng, n, dim):
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    src = np.arange(63, n, 64)
    rows[src] = rows[src - 37] + 0.02 * rng.standard_normal((len(src), dim), dtype=np.float32)
    return rows


def burst_rows(rng, n, dim, burst=64):
    base = rng.standard_normal((n // burst, dim), dtype=np.float32)
    return np.repeat(base, burst, axis=0) + 0.05 * rng.standard_normal((n, dim), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkage_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/linkage_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d, R = %g; us per call through Index (results on the host), median (min ... max) of %d calls;" % (DIM, RADIUS, a.reps))
    say("# ratio = time / (rounds x components time): a round is one sweep over the pairs plus O(n) work, components is one sweep")
    say("%-4s %-7s %7s %30s | %30s %6s %6s %7s | %30s %6s %7s" % ("dt", "data", "rows", "components(R)", "linkage(R)", "edges", "rounds", "ratio",
                                                                 "linkage(): the whole tree", "rounds", "ratio"))
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    sizes = [n for n in ((4096, 65536) if a.quick else (4096, 65536, 262144)) if n <= a.max_rows]
    for n in sizes:
        for data, make in (("sparse", sparse_rows), ("bursts", burst_rows)):
            host = make(np.random.default_rng(n + len(data)), n, DIM)
            for dt in ("f16", "i8"):
                ix = clip_cpp_amd.Index(clip, DIM, dt)
                ix.add(host)
                labels = ix.components(RADIUS)[0]                    # warm: workspaces, code objects
                edges = ix.linkage(RADIUS)
                assert np.array_equal(clip_cpp_amd.cut_linkage(n, *edges), labels), "the forest at R is not components(R)"
                _, tc = wall(lambda: ix.components(RADIUS), a.reps)
                _, tf = wall(lambda: ix.linkage(RADIUS), a.reps)
                rf = ix.linkage_rounds()
                whole = ix.linkage()
                assert len(whole[0]) == n - 1
                _, tw = wall(lambda: ix.linkage(), max(1, a.reps if n <= 65536 else 1))
                rw = ix.linkage_rounds()
                r = dict(dtype=dt, data=data, n=n, components=tc, forest=tf, forest_edges=int(len(edges[0])), forest_rounds=rf,
                         forest_ratio=round(tf["median"] / (rf * tc["median"]), 3), tree=tw, tree_rounds=rw,
                         tree_ratio=round(tw["median"] / (rw * tc["median"]), 3))
                rows.append(r)
                say("%-4s %-7s %7d %30s | %30s %6d %6d %7.3f | %30s %6d %7.3f" % (dt, data, n, fmt(tc), fmt(tf), r["forest_edges"], rf,
                                                                                 r["forest_ratio"], fmt(tw), rw, r["tree_ratio"]))
                ix.close()
            del host
    clip.close()
    say()
    say("# the seeded rows of clip_amd_bench_modes, N = 65536: clip_amd_bench_linkage (the whole tree) against clip_amd_bench_components(R)")
    say("%-4s %-7s %16s %6s %16s %7s" % ("dt", "data", "linkage", "rounds", "components(R)", "ratio"))
    for dt in ("f16", "i8"):
        us, rounds = clip_cpp_amd.bench_linkage(dt, 65536, DIM, 0, 2)
        uc = clip_cpp_amd.bench_components(dt, 65536, DIM, RADIUS, 2)
        if us < 0 or uc < 0:
            raise RuntimeError("bench hook failed: %s %s" % (us, uc))
        rows.append(dict(kind="hooks", dtype=dt, linkage_us=round(us, 1), rounds=rounds, components_us=round(uc, 1)))
        say("%-4s %-7s %16.1f %6d %16.1f %7.3f" % (dt, "sparse", us, rounds, uc, us / (rounds * uc)))
    say()
    say(json.dumps(dict(radius=RADIUS, dim=DIM, reps=a.reps, rows=rows)))
    out.close()


if __name__ == "__main__":
    main()
