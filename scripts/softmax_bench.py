"""Softmax queries of the exact index (k_softmax.hip, clip_amd_index_softmax_device) against three yardsticks, measured in one run and
written to profiles/softmax_bench.txt (--out).

    python scripts/softmax_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), 1, 16 and 256 queries, k = 10, scale 100, over the seeded
rows of clip_amd_bench_search.  softmax is clip_amd_bench_softmax: device time (HIP events) of one clip_amd_index_softmax_device, all four
outputs: the search, the second query preparation, the sweep and the finish.  Yardsticks:
(a) search   clip_amd_bench_search with the same queries and k = 10 over the same N: the search the call contains.  softmax - search is
             what the probabilities cost; softmax / search the ratio.
(b) rank     clip_amd_bench_rank with as many columns over the same N: the same sweep with a compare and an integer add per pair in the
             place of v_exp_f32 and an f32 add (its key kernel and finish included).  (softmax - search) / rank compares the sweeps.
(c) torch    what a user would write without the entry point: the rows as an [N, dim] f16 tensor on the device, s = q @ rows.T,
             softmax(100 s), topk(10).  Not bit-exact with the index, there for the time only; f16 rows for both dtypes.

A figure is the median of --reps repetitions with (min ... max) behind it, the repetitions of the things compared taken in turn.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libclip.so: tests/conftest.py says why)

import clip_cpp_amd  # noqa: E402

DIM, K = 512, 10


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%9.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def device_us(f):
    """device time of f() in microseconds, between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def torch_softmax(rows, q):
    return torch.softmax((q @ rows.T).float() * 100.0, dim=1).topk(K, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/softmax_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d, k %d, scale 100; us, median (min ... max) of %d repetitions, the four taken in turn" % (DIM, K, a.reps))
    say("%-4s %8s %4s %30s %30s %8s %30s %8s %30s %8s" % ("dt", "N", "nq", "softmax", "search (k 10)", "sm/a", "rank", "(sm-a)/b", "torch (f16 rows)",
                                                       "c/sm"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        rows = torch.nn.functional.normalize(torch.randn(n, DIM, device="cuda"), dim=1).to(torch.float16)
        for dt in ("f16", "i8"):
            for nq in (1, 16, 256):
                q = torch.nn.functional.normalize(torch.randn(nq, DIM, device="cuda"), dim=1).to(torch.float16)
                torch_softmax(rows, q)
                got = {k: [] for k in ("softmax", "search", "rank", "torch")}
                for _ in range(a.reps):
                    got["softmax"].append(clip_cpp_amd.bench_softmax(dt, n, DIM, nq, K, 20))
                    got["search"].append(clip_cpp_amd.bench_search(dt, n, DIM, nq, K, 20))
                    got["rank"].append(clip_cpp_amd.bench_rank(dt, n, DIM, nq, 20))
                    got["torch"].append(device_us(lambda: torch_softmax(rows, q)))
                if min(min(v) for v in got.values()) < 0:
                    raise RuntimeError("a benchmark hook failed: %r" % (got,))
                s = {k: stats(v) for k, v in got.items()}
                extra = s["softmax"]["median"] - s["search"]["median"]
                r = dict(dtype=dt, n=n, nq=nq, softmax_over_search=round(s["softmax"]["median"] / s["search"]["median"], 3),
                         extra_over_rank=round(extra / s["rank"]["median"], 3), torch_over_softmax=round(s["torch"]["median"] / s["softmax"]["median"], 3), **s)
                rows_out.append(r)
                say("%-4s %8d %4d %30s %30s %8.3f %30s %8.3f %30s %8.3f" % (dt, n, nq, fmt(s["softmax"]), fmt(s["search"]), r["softmax_over_search"],
                                                                          fmt(s["rank"]), r["extra_over_rank"], fmt(s["torch"]), r["torch_over_softmax"]))
        del rows
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()


if __name__ == "__main__":
    main()
