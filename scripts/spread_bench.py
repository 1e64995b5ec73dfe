"""Farthest-first selection of the exact index (k_spread.hip, clip_amd_index_spread) against two yardsticks, measured in one run and written
to profiles/spread_bench.txt (--out).

    python scripts/spread_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), n_max = 16, 256 and 1024, over the seeded rows of
clip_amd_bench_range.  spread is clip_amd_bench_spread: device time (HIP events) of one clip_amd_index_spread_device of n_max centres, all
outputs, no seeds, no stop radius, so n_max sweeps of the gallery plus the init and finish launches; per step = that time / n_max.
Yardsticks:
(a) search   clip_amd_bench_search with one query and k = 5 over the same N: a greedy step reads the same gallery bytes and selects one
             row where the scan selects five per chunk.  step / search is the ratio; above 1 the step is the slower one.
(b) torch    what a user would write without the entry point: the rows as an [N, dim] f16 tensor on the device (random unit rows made
             there: the time does not depend on the values), gap = +inf, then per step d = 1 - rows @ rows[pick]; gap = minimum(gap, d);
             pick = argmax(gap), n_max steps between two events.  Not bit-exact with the index (another dot product, no tie rule, no
             owners), there for the time only; f16 rows for both dtypes, torch having no int8 matrix-vector product on the device.
copy         the device's copy rate in the same run: a 1 GiB device-to-device copy, bytes read per second (as many are written).
gallery GB/s N * row bytes / per-step time: the rate at which a step reads the gallery, to set against `copy`.

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
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def in_turn(calls, reps):
    """{name: stats} of the named calls, repetition by repetition in turn"""
    got = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            us = f()
            if us < 0:
                raise RuntimeError("%s failed: %s" % (k, us))
            got[k].append(us)
    return {k: stats(v) for k, v in got.items()}


def device_us(f):
    """device time of f() in microseconds, between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def torch_spread(rows, n_max):
    gap = torch.full((rows.shape[0],), float("inf"), dtype=torch.float16, device=rows.device)
    pick = torch.zeros((), dtype=torch.int64, device=rows.device)
    for _ in range(n_max):
        d = 1.0 - torch.mv(rows, rows[pick])
        gap = torch.minimum(gap, d)
        pick = torch.argmax(gap)
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/spread_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy = stats([device_us(lambda: dst.copy_(src)) for _ in range(a.reps)])
    copy_gbs = (1 << 30) / copy["median"] / 1e3
    del src, dst
    say("# copy: 1 GiB device to device in %s us: %.0f GB/s read (and as much written)" % (fmt(copy).strip(), copy_gbs))
    say("# dim %d; us, median (min ... max) of %d repetitions; per step = spread / n_max" % (DIM, a.reps))
    say("%-4s %8s %6s %34s %10s %30s %8s %34s %8s %8s %7s" % ("dt", "N", "n_max", "spread", "per step", "search (1 query, k 5)", "step/a",
                                                               "torch loop (f16 rows)", "per step", "b/spread", "GB/s"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        rows = torch.nn.functional.normalize(torch.randn(n, DIM, device="cuda"), dim=1).to(torch.float16)
        for dt in ("f16", "i8"):
            for n_max in (16, 256, 1024):
                iters = 3 if n_max * n <= (256 << 16) else 1
                torch_spread(rows, 4)
                s = in_turn({"spread": lambda: clip_cpp_amd.bench_spread(dt, n, DIM, n_max, 0, iters),
                             "search": lambda: clip_cpp_amd.bench_search(dt, n, DIM, 1, 5, 20),
                             "torch": lambda: device_us(lambda: torch_spread(rows, n_max))}, a.reps)
                step = s["spread"]["median"] / n_max
                tstep = s["torch"]["median"] / n_max
                gbs = n * ROW_BYTES[dt] / step / 1e3
                r = dict(dtype=dt, n=n, n_max=n_max, step_us=round(step, 2), step_over_search=round(step / s["search"]["median"], 3),
                         torch_step_us=round(tstep, 2), torch_over_spread=round(s["torch"]["median"] / s["spread"]["median"], 3),
                         gallery_gbs=round(gbs, 1), copy_gbs=round(copy_gbs, 1), **s)
                rows_out.append(r)
                say("%-4s %8d %6d %34s %10.2f %30s %8.3f %34s %8.2f %8.3f %7.0f" % (dt, n, n_max, fmt(s["spread"]), step, fmt(s["search"]),
                                                                                     r["step_over_search"], fmt(s["torch"]), tstep,
                                                                                     r["torch_over_spread"], gbs))
        del rows
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()


if __name__ == "__main__":
    main()
