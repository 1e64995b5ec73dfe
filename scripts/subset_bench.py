"""Subset search of the exact index (the masked instantiation of search_scan_kernel through clip_amd_bench_search_subset) against three
yardsticks measured in the same process, interleaved round by round:

    python scripts/subset_bench.py [--quick] [--iters N] [--rounds N] [--dtypes f16,f32,i8] [--no-torch]

Per dtype, allowed fraction (1.0, 0.5, 0.1, 0.01) and shape of the allowed set (a seeded random selection / one contiguous id range), on
1 M x 512 rows, 64 queries, k = 100, microseconds per search:
  masked    clip_amd_bench_search_subset: the index holds every row, the scan honours the allowed set
  unmasked  clip_amd_bench_search on an index of the same seeded rows (each hook call builds its own): what the search costs when every
            row is eligible (the over-fetch route starts here)
  ideal     clip_amd_bench_search on an index that holds only round(fraction N) rows: nothing a mask could beat
  torch     torch.mm + masked_fill(-inf on the scores of the excluded rows) + torch.topk on f16 rows (f32 for f32; i8 has no torch form: f16)
Each figure is the median over the rounds; `spread` is (max - min) / median of the masked figure over the rounds, the run-to-run noise a
difference has to exceed.  Seeded data; only times are compared, the results are the business of tests/test_gpu_index_subset.py.
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

FRACTIONS = (1.0, 0.5, 0.1, 0.01)


class TorchMasked:
    """torch.mm + masked_fill + topk over one gallery, the excluded set changing per call"""

    def __init__(self, dtype, n, dim, nq):
        dt = torch.float32 if dtype == "f32" else torch.float16
        g = torch.Generator(device="cuda").manual_seed(5)
        self.rows = torch.randn((n, dim), generator=g, device="cuda", dtype=dt)
        self.q = torch.randn((nq, dim), generator=g, device="cuda", dtype=dt)
        self.u = torch.rand((n,), generator=g, device="cuda")
        self.n = n

    def us(self, fraction, contiguous, k, iters):
        if contiguous:
            cnt = int(round(fraction * self.n))
            start = (self.n - cnt) // 2
            ids = torch.arange(self.n, device="cuda")
            excluded = (ids < start) | (ids >= start + cnt)
        else:
            excluded = self.u >= fraction
        run = lambda: torch.topk(torch.mm(self.q, self.rows.t()).masked_fill_(excluded[None, :], float("-inf")), k, dim=1)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="64 K rows: a rehearsal of the script, not a measurement")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dtypes", default="f16,f32,i8")
    a = ap.parse_args()
    torch.cuda.init()
    n, dim, nq, k = (1 << 16 if a.quick else 1 << 20), 512, 64, 100
    print("N = %d, dim = %d, nq = %d, k = %d, %d iterations per figure, median of %d interleaved rounds" % (n, dim, nq, k, a.iters, a.rounds))
    print("%-4s %8s %-10s %10s %10s %10s %10s %7s %9s %9s" % ("dt", "fraction", "set", "masked_us", "unmasked", "ideal_us", "torch_us", "spread",
                                                            "vs_unmask", "vs_ideal"))
    out = []
    for dtype in a.dtypes.split(","):
        tm = None if a.no_torch else TorchMasked(dtype, n, dim, nq)
        for fraction in FRACTIONS:
            for contiguous in (False, True):
                m, u, i, t = [], [], [], []
                for _ in range(a.rounds):                       # the figures that are compared, alternating
                    m.append(clip_cpp_amd.bench_search_subset(dtype, n, dim, nq, k, fraction, contiguous, a.iters))
                    u.append(clip_cpp_amd.bench_search(dtype, n, dim, nq, k, a.iters))
                    i.append(clip_cpp_amd.bench_search(dtype, max(1, int(round(fraction * n))), dim, nq, k, a.iters))
                    t.append(tm.us(fraction, contiguous, k, a.iters) if tm else -1.0)
                if min(m + u + i) <= 0:
                    raise SystemExit("a benchmark hook failed: %r %r %r" % (m, u, i))
                med = statistics.median
                r = dict(dtype=dtype, fraction=fraction, set="contiguous" if contiguous else "random", masked_us=round(med(m), 1),
                         unmasked_us=round(med(u), 1), ideal_us=round(med(i), 1), torch_us=round(med(t), 1),
                         spread=round((max(m) - min(m)) / med(m), 3), unmasked_spread=round((max(u) - min(u)) / med(u), 3))
                out.append(r)
                print("%-4s %8.2f %-10s %10.1f %10.1f %10.1f %10.1f %7.3f %9.2f %9.2f" % (
                    dtype, fraction, r["set"], r["masked_us"], r["unmasked_us"], r["ideal_us"], r["torch_us"], r["spread"],
                    r["masked_us"] / r["unmasked_us"], r["masked_us"] / r["ideal_us"]), flush=True)
        del tm
        torch.cuda.empty_cache()
    print(json.dumps(dict(n=n, dim=dim, nq=nq, k=k, rows=out)))


if __name__ == "__main__":
    main()
