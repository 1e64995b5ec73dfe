"""The mutual-reachability tree of the exact index (clip_amd_index_linkage_core) against its two halves, the k-NN graph and the
single-linkage tree, measured on one index in one run and written to profiles/linkage_core_bench.txt (--out).

    python scripts/linkage_core_bench.py [--quick] [--iters N] [--max-rows N] [--out FILE]

One linkage_core call is a neighbour search (the core distances; its results stay on the device) and the Boruvka rounds of the tree over
w = max(d, core, core).  So the yardstick is the sum of one knn_graph(k) call and one linkage() call on the same rows; no threshold is
set, the file states the ratios.  Per row count (65 536, 262 144), dtype (f16, i8), k (4, 16) and data, dim 512, through
clip_amd_bench_linkage_core (the rows of clip_amd_bench_modes, generated on the device):

  sparse    seeded random rows, every 64th a small perturbation of an earlier one
  bursts    groups of a row and 63 noisy copies of it

  linkage_core   one clip_amd_index_linkage_core call (host form, the whole tree, core wanted) and the rounds that did work
  knn_graph      one clip_amd_index_knn_graph(k) call (results to the host)
  linkage        one clip_amd_index_linkage call (the whole tree) and its rounds
  core column    the neighbour search of linkage_core alone: the same kernels as knn_graph with the device-side sink
  ratio          linkage_core / (knn_graph + linkage)
  tree part      linkage_core - core column, and tree part / linkage: what the core distances cost the rounds, per call; per round it is
                 (tree part / rounds) / (linkage / its rounds)

Every time is wall time of the synchronous host call in microseconds, the mean of --iters calls after one warm call of each; the four
calls of an iteration run one after another on the one index, so all four see the same clocks and the same rows.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before libclip.so: tests/conftest.py says why)

import clip_cpp_amd  # noqa: E402

DIM = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkage_core_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/linkage_core_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d; us per call (host forms, the whole tree), mean of %d calls (1 at 262 144 rows) after a warm one, the four calls interleaved"
        % (DIM, a.iters))
    say("# on one index; ratio = linkage_core / (knn_graph + linkage); tree = linkage_core - core column; per round = (tree / rounds) /")
    say("# (linkage / its rounds)")
    say("%-4s %-7s %7s %3s %13s %6s %12s %13s %6s %12s %7s %13s %8s %9s" % ("dt", "data", "rows", "k", "linkage_core", "rounds", "knn_graph",
                                                                        "linkage", "rounds", "core column", "ratio", "tree", "/linkage",
                                                                        "per round"))
    sizes = [n for n in ((65536,) if a.quick else (65536, 262144)) if n <= a.max_rows]
    for n in sizes:
        for data, copies in (("sparse", 0), ("bursts", 63)):
            for dt in ("f16", "i8"):
                for k in (4, 16):
                    r = clip_cpp_amd.bench_linkage_core(dt, n, DIM, k, copies, a.iters if n <= 65536 else 1)
                    if min(r["linkage_core"], r["knn_graph"], r["linkage"], r["core_column"]) < 0:
                        raise RuntimeError("bench hook failed: %r" % (r,))
                    tree = r["linkage_core"] - r["core_column"]
                    r.update(dtype=dt, data=data, n=n, k=k, ratio=round(r["linkage_core"] / (r["knn_graph"] + r["linkage"]), 3),
                             tree=round(tree, 1), tree_ratio=round(tree / r["linkage"], 3),
                             round_ratio=round((tree / max(r["rounds"], 1)) / (r["linkage"] / max(r["linkage_rounds"], 1)), 3))
                    rows.append(r)
                    say("%-4s %-7s %7d %3d %13.1f %6d %12.1f %13.1f %6d %12.1f %7.3f %13.1f %8.3f %9.3f"
                        % (dt, data, n, k, r["linkage_core"], r["rounds"], r["knn_graph"], r["linkage"], r["linkage_rounds"], r["core_column"],
                           r["ratio"], tree, r["tree_ratio"], r["round_ratio"]))
    say()
    say(json.dumps(dict(dim=DIM, iters=a.iters, rows=rows)))
    out.close()


if __name__ == "__main__":
    main()
