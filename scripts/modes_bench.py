"""Density modes of the exact index (k_modes.hip, clip_amd_index_modes) against what there was, measured in one run and written to
profiles/modes_bench.txt (--out).

    python scripts/modes_bench.py [--quick] [--reps N] [--parent-lib PATH/libclip.so] [--out FILE]

1. sparse   the data of scripts/components_bench.py (seeded random rows, every 64th a perturbation of an earlier one: N / 64 pairs), radius =
            link = 0.05, dim 512, f16 and i8, N = 65 536: clip_amd_bench_modes against clip_amd_bench_components of this build and, with
            --parent-lib, of the parent commit's library loaded next to it.  modes runs the scoring pass twice (density, ascend),
            components once.
2. dense    N = 65 536 rows in bursts of 64 / 256 / 1024 noisy copies (radius 0.05: every pair of a burst is near), through a real Index:
            Index.modes against Index.components at the same radius and against the only composition there was, Index.pairs(max(radius,
            link)) and then the contract in numpy (tests/modes_common.py: from_pairs; both parts timed, the numpy part only up to
            --numpy-max-pairs pairs).  The two routes must agree bit for bit.
3. passes   where the time of a dense call goes, by switching a pass's output off with a scale below every distance: modes(-1, -1) scores
            twice and emits nothing, modes(R, -1) adds the density pass's atomic adds, modes(-1, R) the ascend pass's loads and atomicMin
            folds (all densities 0 there: the lower id outranks), modes(R, R) is the whole call.  Bursts of 64 / 256 / 1024 copies from
            clip_amd_bench_modes' planted groups.

Every time is the wall time of the synchronous host call in microseconds.  A figure is the median of --reps repetitions (each the hook's
mean over its own iterations) with (min ... max) behind it, the repetitions of the things compared taken in turn.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libclip.so: tests/conftest.py says why)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import synth  # noqa: E402
from modes_common import from_pairs  # noqa: E402

RADIUS = 0.05
DT = {"f32": 0, "f16": 1, "i8": 3}


def parent_components(path):
    """clip_amd_bench_components of another build of the library (the parent commit's), or None"""
    if not path:
        return None
    L = C.CDLL(path)
    L.clip_amd_bench_components.restype = C.c_float
    L.clip_amd_bench_components.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_float, C.c_int]
    return lambda dt, n, dim, r, iters: float(L.clip_amd_bench_components(DT[dt], n, dim, r, iters))


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"]) if s else "         -"


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


def wall(f, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return out, stats(ts)


def burst_rows(rng, n, dim, burst):
    base = rng.standard_normal((n // burst, dim), dtype=np.float32)
    return np.repeat(base, burst, axis=0) + 0.05 * rng.standard_normal((n, dim), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--numpy-max-pairs", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modes_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    parent = parent_components(a.parent_lib)
    rows = []
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/modes_bench.py%s%s on %s" % (" --quick" if a.quick else "", " --parent-lib (the parent commit's build)" if parent else "",
                                               torch.cuda.get_device_name(0)))
    n, dim = 1 << 16, 512
    say("# 1. sparse: N = %d, N / 64 pairs, dim %d, radius = link = %g; us per call, median (min ... max) of %d repetitions" % (n, dim, RADIUS, a.reps))
    say("%-4s %32s %32s %32s %8s" % ("dt", "modes", "components", "components (parent build)", "m / c"))
    for dt in ("f16", "i8"):
        calls = {"modes": lambda: clip_cpp_amd.bench_modes(dt, n, dim, RADIUS, RADIUS, 0, a.iters),
                 "components": lambda: clip_cpp_amd.bench_components(dt, n, dim, RADIUS, a.iters)}
        if parent:
            calls["components_parent"] = lambda: parent(dt, n, dim, RADIUS, a.iters)
        s = in_turn(calls, a.reps)
        yard = s.get("components_parent", s["components"])
        ratio = s["modes"]["median"] / yard["median"]
        rows.append(dict(kind="sparse", dtype=dt, n=n, ratio=round(ratio, 4), **s))
        say("%-4s %32s %32s %32s %8.4f" % (dt, fmt(s["modes"]), fmt(s["components"]), fmt(s.get("components_parent")), ratio))

    say()
    say("# 3. passes: N = %d, dim %d, groups of a row and its noisy copies, R = %g; us per call (scores twice in every column)" % (n, dim, RADIUS))
    say("%-4s %6s %28s %28s %28s %28s %10s %10s" % ("dt", "group", "modes(-1, -1)", "modes(R, -1)", "modes(-1, R)", "modes(R, R)", "density", "ascend"))
    for dt in ("f16",) if a.quick else ("f16", "i8"):
        for group in (64, 256, 1024):
            calls = {"none": lambda: clip_cpp_amd.bench_modes(dt, n, dim, -1.0, -1.0, group - 1, a.iters),
                     "density": lambda: clip_cpp_amd.bench_modes(dt, n, dim, RADIUS, -1.0, group - 1, a.iters),
                     "ascend": lambda: clip_cpp_amd.bench_modes(dt, n, dim, -1.0, RADIUS, group - 1, a.iters),
                     "both": lambda: clip_cpp_amd.bench_modes(dt, n, dim, RADIUS, RADIUS, group - 1, a.iters)}
            s = in_turn(calls, a.reps)
            dens, asc = s["density"]["median"] - s["none"]["median"], s["ascend"]["median"] - s["none"]["median"]
            rows.append(dict(kind="passes", dtype=dt, group=group, density_extra_us=round(dens, 1), ascend_extra_us=round(asc, 1), **s))
            say("%-4s %6d %28s %28s %28s %28s %10.1f %10.1f" % (dt, group, fmt(s["none"]), fmt(s["density"]), fmt(s["ascend"]), fmt(s["both"]), dens, asc))

    say()
    say("# 2. dense: N = %d, dim %d, bursts of noisy copies, radius = link = %g; us per call through Index (results on the host)" % (n, dim, RADIUS))
    say("%-4s %6s %10s %6s %28s %28s %8s %28s %14s" % ("dt", "burst", "pairs", "modes", "Index.modes", "Index.components", "m / c", "Index.pairs",
                                                      "numpy contract"))
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    for dt in ("f16",) if a.quick else ("f16", "i8"):
        for burst in (64, 256, 1024):
            ix = clip_cpp_amd.Index(clip, dim, dt)
            ix.add(burst_rows(np.random.default_rng(burst), n, dim, burst))
            ix.modes(RADIUS)                        # warm: workspaces, code objects
            ix.components(RADIUS)
            got, tm = wall(lambda: ix.modes(RADIUS), a.reps)
            _, tc = wall(lambda: ix.components(RADIUS), a.reps)
            ix.pairs(RADIUS)
            (i, j, d), tp = wall(lambda: ix.pairs(RADIUS), 2)
            tn = None
            if len(i) <= a.numpy_max_pairs:
                want, tn = wall(lambda: from_pairs(n, i, j, d, RADIUS, RADIUS), 1)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want[:4])), "the routes disagree"
            k = int(np.count_nonzero(got[0] == np.arange(n)))
            r = dict(kind="dense", dtype=dt, burst=burst, pairs=int(len(i)), modes_found=k, modes=tm, components=tc,
                     ratio=round(tm["median"] / tc["median"], 4), pairs_us=tp, numpy_contract_us=tn)
            rows.append(r)
            say("%-4s %6d %10d %6d %28s %28s %8.4f %28s %14s" % (dt, burst, len(i), k, fmt(tm), fmt(tc), r["ratio"], fmt(tp),
                                                               "%.1f" % tn["median"] if tn else "not run"))
            del i, j, d
            ix.close()
    clip.close()
    say()
    say(json.dumps(dict(radius=RADIUS, reps=a.reps, iters=a.iters, rows=rows)))
    out.close()


if __name__ == "__main__":
    main()
