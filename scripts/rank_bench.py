"""Rank queries of the exact index (k_rank.hip, clip_amd_index_rank_device) against three yardsticks, measured in one run and written to
profiles/rank_bench.txt (--out).

    python scripts/rank_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), 1, 16 and 256 queries of one target each, over the seeded
rows of clip_amd_bench_search.  rank is clip_amd_bench_rank: device time (HIP events) of one clip_amd_index_rank_device, ranks and
distances out: the query preparation, the key kernel, the count scan and the finish.  Yardsticks:
(a) search   clip_amd_bench_search with the same queries and k = 1 over the same N: the cheapest scan the index has.  rank / search is
             the ratio; above 1 rank is the slower one.  The expectation to confirm or refute: never above 1.
(b) spread   one pick of clip_amd_bench_spread (n_max 16, per step): the gallery-read rate reached here.
(c) torch    what a user would write without the entry point: the rows as an [N, dim] f16 tensor on the device (random unit rows made
             there: the time does not depend on the values), s = q @ rows.T, the compare against the gathered target score, sum.  Not
             bit-exact with the index (another dot product, no tie rule), there for the time only; f16 rows for both dtypes.
key          the key kernel alone (device time), and host: one host-form clip_amd_index_rank of ONE query (wall time, staging and the
             copy back included), both from clip_amd_bench_rank_parts of the rank call of that line.
gallery GB/s N * row bytes / rank time: the rate at which the count scan reads the gallery (once per block of 64 columns).

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

DIM = 512
ROW_BYTES = {"f16": 2 * DIM, "i8": DIM}


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


def torch_rank(rows, q, targets):
    s = q @ rows.T
    return (s > s.gather(1, targets[:, None])).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/rank_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d; us, median (min ... max) of %d repetitions, the four taken in turn; one target per query" % (DIM, a.reps))
    say("%-4s %8s %4s %30s %30s %8s %30s %30s %8s %8s %8s %7s" % ("dt", "N", "nq", "rank", "search (k 1)", "rank/a", "spread step", "torch (f16 rows)",
                                                               "c/rank", "key", "host 1q", "GB/s"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        rows = torch.nn.functional.normalize(torch.randn(n, DIM, device="cuda"), dim=1).to(torch.float16)
        for dt in ("f16", "i8"):
            for nq in (1, 16, 256):
                q = torch.nn.functional.normalize(torch.randn(nq, DIM, device="cuda"), dim=1).to(torch.float16)
                targets = torch.randint(0, n, (nq,), device="cuda")
                torch_rank(rows, q, targets)
                got = {k: [] for k in ("rank", "search", "spread", "torch")}
                key, host = [], []
                for _ in range(a.reps):
                    us, k_us, h_us = clip_cpp_amd.bench_rank(dt, n, DIM, nq, 20, parts=True)
                    got["rank"].append(us)
                    key.append(k_us)
                    host.append(h_us)
                    got["search"].append(clip_cpp_amd.bench_search(dt, n, DIM, nq, 1, 20))
                    got["spread"].append(clip_cpp_amd.bench_spread(dt, n, DIM, 16, 0, 1) / 16.0)
                    got["torch"].append(device_us(lambda: torch_rank(rows, q, targets)))
                if min(min(v) for v in got.values()) < 0 or min(key + host) < 0:
                    raise RuntimeError("a benchmark hook failed: %r" % (got,))
                s = {k: stats(v) for k, v in got.items()}
                gbs = n * ROW_BYTES[dt] / s["rank"]["median"] / 1e3
                r = dict(dtype=dt, n=n, nq=nq, rank_over_search=round(s["rank"]["median"] / s["search"]["median"], 3),
                         torch_over_rank=round(s["torch"]["median"] / s["rank"]["median"], 3), key_us=stats(key)["median"],
                         host_1q_us=stats(host)["median"], gallery_gbs=round(gbs, 1), **s)
                rows_out.append(r)
                say("%-4s %8d %4d %30s %30s %8.3f %30s %30s %8.3f %8.1f %8.1f %7.0f" % (dt, n, nq, fmt(s["rank"]), fmt(s["search"]), r["rank_over_search"],
                                                                                       fmt(s["spread"]), fmt(s["torch"]), r["torch_over_rank"],
                                                                                       r["key_us"], r["host_1q_us"], gbs))
        del rows
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()


if __name__ == "__main__":
    main()
