"""Exact nearest-neighbour search (k_search.hip through clip_amd_bench_search) against the vendor yardstick on the same shapes:
torch.mm (the score matrix written out) + torch.topk.

    python scripts/search_bench.py [--quick] [--iters N] [--dtypes f16,f32,i8] [--no-torch]

Per configuration: microseconds per search, the gallery bytes read once per search divided by that time (GB/s), its fraction of the HBM
rate measured here with a device-to-device copy, and the torch time.  Seeded random data (the torch gallery is its own seeded
random tensor of the same shape and dtype: only the timing is compared, not the results).  i8 rows count N x Dpad (dim rounded up to
64) bytes plus the 4-byte inverse norm per row; torch has no int8 mm + topk here, so their yardstick is the f16 one of the same shape.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libclip.so: conftest.py says why)

import clip_cpp_amd  # noqa: E402


def hbm_rate():
    """GB/s of a 4 GiB device-to-device copy (read + write bytes)"""
    a = torch.empty(1 << 31, dtype=torch.float16, device="cuda")
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 5 / 1e3
    del a, b
    torch.cuda.empty_cache()
    return 2 * (1 << 31) * 2 / s / 1e9


def torch_us(dtype, n, dim, nq, k, iters):
    dt = torch.float32 if dtype == "f32" else torch.float16
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randn((n, dim), generator=g, device="cuda", dtype=dt)
    q = torch.randn((nq, dim), generator=g, device="cuda", dtype=dt)
    for _ in range(2):
        torch.topk(torch.mm(q, rows.t()), k, dim=1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        torch.topk(torch.mm(q, rows.t()), k, dim=1)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    del rows, q
    torch.cuda.empty_cache()
    return us


def gallery_bytes(dtype, n, dim):
    if dtype == "i8":
        return n * ((dim + 63) // 64 * 64 + 4)
    return n * ((dim + 31) // 32 * 32) * (2 if dtype == "f16" else 4)


def configs(quick, dtypes):
    out = []
    for dtype in dtypes:
        for nq in (1, 16, 64, 256, 1024):
            for k in (5, 100, 1024):
                out.append((dtype, 1 << 20, 512, nq, k))
        for n in (1 << 16, 1 << 22):
            for dim in (512, 768, 1024):
                out.append((dtype, n, dim, 16, 100))
    if quick:
        out = [c for c in out if c[3] in (1, 64) and c[4] in (5, 100) and c[1] == 1 << 20] + [(d, 1 << 22, 512, 16, 100) for d in dtypes]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dtypes", default="f16,f32,i8")
    a = ap.parse_args()
    torch.cuda.init()
    rate = hbm_rate()
    print("HBM copy rate: %.0f GB/s" % rate)
    print("%-4s %8s %5s %5s %5s %10s %8s %6s %10s %7s" % ("dt", "N", "dim", "nq", "k", "us", "GB/s", "frac", "torch_us", "speedup"))
    rows = []
    for dtype, n, dim, nq, k in configs(a.quick, a.dtypes.split(",")):
        us = clip_cpp_amd.bench_search(dtype, n, dim, nq, k, a.iters)
        gb = gallery_bytes(dtype, n, dim) / 1e9
        tu = -1.0 if a.no_torch else torch_us(dtype, n, dim, nq, k, a.iters)
        r = dict(dtype=dtype, n=n, dim=dim, nq=nq, k=k, us=round(us, 1), gbs=round(gb / (us * 1e-6), 0) if us > 0 else None,
                 frac=round(gb / (us * 1e-6) / rate, 3) if us > 0 else None, torch_us=round(tu, 1))
        rows.append(r)
        print("%-4s %8d %5d %5d %5d %10.1f %8.0f %6.3f %10.1f %7.2f" % (dtype, n, dim, nq, k, us, r["gbs"] or 0, r["frac"] or 0, tu,
                                                                          tu / us if us > 0 and tu > 0 else 0), flush=True)
    print(json.dumps(dict(hbm_gbs=round(rate), rows=rows)))


if __name__ == "__main__":
    main()
