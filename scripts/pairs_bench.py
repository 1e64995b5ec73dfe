"""Near-duplicate pairs and range search of the exact index (k_join.hip through clip_amd_bench_range) against two yardsticks measured in
the same run: torch blockwise on the same shapes (f16 rows: torch.mm over the upper-triangle blocks + nonzero(S >= 1 - r)) and the
existing route (clip_amd_bench_search of 1024 queries at k = 100, scaled to N queries).

    python scripts/pairs_bench.py [--quick] [--iters N] [--no-torch]

Per configuration: microseconds per call (wall time of the synchronous host call: scoring, counts to the host, sort, copy-out), the
algorithmic FLOP/s over it — n(n-1)/2 x 2 x Dpad for pairs, n x nq x 2 x Dpad for a range search — and its fraction of the dtype's dense
MFMA peak (fp16 2.5 PF, i8 5 POPS, f32 157 TF).  Seeded random rows, every 64th a perturbation of an earlier one, radius 0.05: the
output is sparse (N / 64 pairs) but not empty.  Range search rows compare against search at k = 5 with the same nq; bench_search times
that on the device (HIP events over asynchronous calls), so the ratio is biased against the synchronous range-search call.  f32 pairs run at
N <= 256 K only (1 M would take tens of seconds per call at the f32 rate).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402

PEAK = {"f16": 2.5e15, "i8": 5.0e15, "f32": 157e12}
RADIUS = 0.05


def dpad(dtype, dim):
    return (dim + 63) // 64 * 64 if dtype == "i8" else (dim + 31) // 32 * 32


def torch_pairs_us(n, dim, radius, block=16384):
    """torch.mm over the upper-triangle blocks of normalised f16 rows + nonzero(S >= 1 - r); one warm run, one timed"""
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.nn.functional.normalize(torch.randn((n, dim), generator=g, device="cuda"), dim=1).half()
    thr = 1.0 - radius

    def once():
        found = 0
        for i0 in range(0, n, block):
            a = rows[i0:i0 + block]
            for j0 in range(i0, n, block):
                s = torch.mm(a, rows[j0:j0 + block].t())
                if j0 == i0:
                    s = torch.triu(s, diagonal=1)
                found += torch.nonzero(s >= thr).shape[0]
        return found
    once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    once()
    e1.record()
    torch.cuda.synchronize()
    del rows
    torch.cuda.empty_cache()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    out = []
    print("%-5s %-4s %8s %5s %5s %12s %9s %6s %12s %12s" % ("kind", "dt", "N", "dim", "nq", "us", "TFLOP/s", "peak", "torch_us", "route_us"))
    pairs = [(dt, n, dim) for dt in ("f16", "i8", "f32") for n in (1 << 16, 1 << 18, 1 << 20) for dim in (512, 768)
             if not (dt == "f32" and n > 1 << 18)]
    ranges = [(dt, 1 << 20, 512, nq) for dt in ("f16", "i8") for nq in (1, 16, 1024)]
    if a.quick:
        pairs = [(dt, n, 512) for dt, n, dim in pairs if dim == 512 and n in (1 << 16, 1 << 20)]
        ranges = [r for r in ranges if r[0] == "f16"]
    route = {}
    for dt, n, dim in pairs:
        us = clip_cpp_amd.bench_range(dt, n, dim, 0, RADIUS, a.iters)
        flop = n * (n - 1) / 2 * 2 * dpad(dt, dim)
        tu = -1.0 if a.no_torch or dt == "f32" else torch_pairs_us(n, dim, RADIUS)
        key = (dt, dim)
        if key not in route:
            route[key] = clip_cpp_amd.bench_search(dt, 1 << 20, dim, 1024, 100, 2) / 1024.0    # µs per query row at N = 1 M
        ru = route[key] * n * n / float(1 << 20)       # scaled: n queries over n rows (the scan is linear in both)
        r = dict(kind="pairs", dtype=dt, n=n, dim=dim, nq=0, us=round(us, 1), tflops=round(flop / us / 1e6, 1) if us > 0 else None,
                 frac=round(flop / (us * 1e-6) / PEAK[dt], 3) if us > 0 else None, torch_us=round(tu, 1), route_us=round(ru, 1))
        out.append(r)
        print("%-5s %-4s %8d %5d %5d %12.1f %9.1f %6.3f %12.1f %12.1f" % ("pairs", dt, n, dim, 0, us, r["tflops"] or 0, r["frac"] or 0, tu, ru),
              flush=True)
    for dt, n, dim, nq in ranges:
        us = clip_cpp_amd.bench_range(dt, n, dim, nq, RADIUS, max(a.iters, 5))
        flop = n * nq * 2 * dpad(dt, dim)
        su = clip_cpp_amd.bench_search(dt, n, dim, nq, 5, max(a.iters, 5))
        r = dict(kind="range", dtype=dt, n=n, dim=dim, nq=nq, us=round(us, 1), tflops=round(flop / us / 1e6, 1) if us > 0 else None,
                 frac=round(flop / (us * 1e-6) / PEAK[dt], 4) if us > 0 else None, search_k5_us=round(su, 1),
                 vs_search=round(us / su, 3) if us > 0 and su > 0 else None)
        out.append(r)
        print("%-5s %-4s %8d %5d %5d %12.1f %9.1f %6.4f  search(k=5) %10.1f  ratio %.3f" % ("range", dt, n, dim, nq, us, r["tflops"] or 0,
                                                                                          r["frac"] or 0, su, r["vs_search"] or 0), flush=True)
    print(json.dumps(dict(radius=RADIUS, rows=out)))


if __name__ == "__main__":
    main()
