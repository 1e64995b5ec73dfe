"""Extents of a labelling (k_extents.hip, clip_amd_index_extents) against the other endings of the pairs tile loop, measured in one run.

    python scripts/extents_bench.py [--quick] [--reps N] [--out FILE]

1. index    dim 512, f16 and i8, N = 65 536 and 262 144 rows in bursts of 64 and of 1024 noisy copies, through a real Index: the rows of a
            burst lie together (labels sorted: row r carries r / burst) or the same rows are scattered over the index by one fixed
            permutation (labels shuffled: every tile of 128 rows holds labels from the whole range).  Index.extents(labels) against
            Index.components(0.05) on the same index (its labels are the bursts) and against one round of Index.linkage() on the same index
            (the call's time over the rounds that ran: the other ending that sees every pair), with the tile pairs extents computed
            (clip_amd_test_index_extents_route) out of all N / 128 (N / 128 + 1) / 2, and the time with the tile skip off (route 1).
2. hook     the same shapes through clip_amd_bench_extents (no Python, seeded rows on the device), as a check of section 1.
3. numpy    the route there was: Index.pairs(4.0) + the contract in numpy (tests/extents_common.py, vectorised here), on the first 4 096
            rows of the 65 536-row f16 indexes (the pair list of 65 536 rows is 2^31 pairs, 34 GB: it does not fit), against Index.extents on
            an index of those rows; the outputs must agree bit for bit.

Every time is the wall time of the synchronous host call in microseconds, after a warm call of the same shape.  A figure is the median
of --reps repetitions with (min ... max) behind it, the repetitions of the things compared taken in turn.
"""
import argparse
import json
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
SUBSET = 4096


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


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


def burst_rows(rng, n, dim, burst):
    base = rng.standard_normal((n // burst, dim), dtype=np.float32)
    rows = np.repeat(base, burst, axis=0)
    for r0 in range(0, n, 1 << 14):                     # the noise in pieces: no second array of the whole size
        rows[r0:r0 + (1 << 14)] += 0.05 * rng.standard_normal((min(1 << 14, n - r0), dim), dtype=np.float32)
    return rows


def numpy_extents(n, labels, pi, pj, pd):
    """the contract over a pair list, vectorised: (centre, radius, diameter, reach, far); no NaN, no negative label, every row a member"""
    keep = labels[pi] == labels[pj]
    a, b, d = np.concatenate([pi[keep], pj[keep]]), np.concatenate([pj[keep], pi[keep]]), np.concatenate([pd[keep], pd[keep]])
    order = np.lexsort((b, -d.astype(np.float64), a))    # per row: the largest distance first, the lowest other id among equals
    a, b, d = a[order], b[order], d[order]
    first = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])[:a.size]
    reach = np.zeros(n, dtype=np.float32)
    far = np.full(n, -1, dtype=np.int64)
    reach[a[first]], far[a[first]] = d[first], b[first]
    rows = np.lexsort((np.arange(n), reach, labels))     # per group: the smallest reach first, the lowest id among equals
    head = np.flatnonzero(np.r_[True, labels[rows][1:] != labels[rows][:-1]])
    size = np.diff(np.r_[head, n])
    centre = np.empty(n, dtype=np.int64)
    centre[rows] = np.repeat(rows[head], size)
    diameter = np.empty(n, dtype=np.float32)
    diameter[rows] = np.repeat(np.maximum.reduceat(reach[rows], head), size)
    return centre, reach[centre], diameter, reach, far


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extents_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    dim, results, subset = 512, [], {}
    say("# extents_bench: %s; us per synchronous host call, median (min ... max) of %d repetitions taken in turn"
        % (torch.cuda.get_device_name(0), a.reps))
    say("# 1. index: dim %d; components at radius %g; linkage round = Index.linkage() / the rounds that ran" % (dim, RADIUS))
    say("%-4s %7s %6s %-8s %30s %30s %30s %30s %8s %14s %7s %7s" % ("dt", "N", "burst", "labels", "extents", "extents, skip off", "components",
                                                                  "linkage round", "rounds", "tiles computed", "e / c", "e / l"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 18):
        for burst in (64, 1024):
            rows = burst_rows(np.random.default_rng(burst), n, dim, burst)
            sorted_labels = np.arange(n, dtype=np.int64) // burst
            perm = np.random.default_rng(n + burst).permutation(n)
            for dt in ("f16", "i8"):
                for name in ("sorted", "shuffled"):
                    ix = clip_cpp_amd.Index(clip, dim, dt)
                    labels = sorted_labels if name == "sorted" else sorted_labels[perm]
                    for r0 in range(0, n, 1 << 16):
                        ix.add(rows[r0:r0 + (1 << 16)] if name == "sorted" else rows[perm[r0:r0 + (1 << 16)]])
                    rounds = []

                    def linkage():
                        ix.linkage()
                        rounds.append(ix.linkage_rounds())

                    def skip_off():
                        ix.extents_route(1)
                        ix.extents(labels)
                        ix.extents_route(0)
                    s = in_turn({"extents": lambda: ix.extents(labels), "off": skip_off, "components": lambda: ix.components(RADIUS),
                                 "linkage": linkage}, a.reps)
                    ix.extents(labels)
                    computed, tiles = ix.extents_route(0), (n // 128) * (n // 128 + 1) // 2
                    lowest = np.full(n, n, dtype=np.int64)
                    np.minimum.at(lowest, labels, np.arange(n))
                    assert np.array_equal(ix.components(RADIUS)[0], lowest[labels]), "components at %g are not the bursts" % RADIUS
                    assert len(set(rounds)) == 1
                    per_round = {k: round(v / rounds[0], 1) for k, v in s["linkage"].items()}
                    r = dict(dtype=dt, n=n, burst=burst, labels=name, extents=s["extents"], extents_skip_off=s["off"], components=s["components"],
                             linkage_round=per_round, rounds=rounds[0], tiles_computed=computed, tiles=tiles,
                             over_components=round(s["extents"]["median"] / s["components"]["median"], 3),
                             over_linkage_round=round(s["extents"]["median"] / per_round["median"], 3))
                    results.append(r)
                    say("%-4s %7d %6d %-8s %30s %30s %30s %30s %8d %14s %7.3f %7.3f"
                        % (dt, n, burst, name, fmt(s["extents"]), fmt(s["off"]), fmt(s["components"]), fmt(per_round), rounds[0],
                           "%d / %d" % (computed, tiles), r["over_components"], r["over_linkage_round"]))
                    if n == 1 << 16 and dt == "f16":
                        subset[(burst, name)] = (rows[:SUBSET] if name == "sorted" else rows[perm[:SUBSET]], labels[:SUBSET].copy())
                    ix.close()
            del rows

    say("\n# 2. hook: clip_amd_bench_extents (seeded rows on the device, the host form's copies included), us per call")
    say("%-4s %7s %6s %30s %30s" % ("dt", "N", "burst", "sorted", "shuffled"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 18):
        for burst in (64, 1024):
            for dt in ("f16", "i8"):
                got = {k: [] for k in (1, 0)}
                for _ in range(a.reps):
                    for k in got:
                        us = clip_cpp_amd.bench_extents(dt, n, dim, burst, bool(k), 3)
                        if us < 0:
                            raise RuntimeError("clip_amd_bench_extents failed: %s" % us)
                        got[k].append(us)
                s = {k: stats(v) for k, v in got.items()}
                results.append(dict(kind="hook", dtype=dt, n=n, burst=burst, sorted=s[1], shuffled=s[0]))
                say("%-4s %7d %6d %30s %30s" % (dt, n, burst, fmt(s[1]), fmt(s[0])))

    say("\n# 3. numpy: the first %d rows of the 65 536-row f16 indexes; Index.pairs(4.0) + the contract in numpy against Index.extents" % SUBSET)
    say("%6s %-8s %10s %30s %30s %30s %10s" % ("burst", "labels", "pairs", "extents", "pairs(4.0)", "numpy over the pairs", "ratio"))
    for (burst, name), (rows, labels) in subset.items():
        ix = clip_cpp_amd.Index(clip, dim, "f16")
        ix.add(rows)
        labels = np.unique(labels, return_inverse=True)[1].astype(np.int64)      # below the subset's size
        kept = {}

        def pairs():
            kept["p"] = ix.pairs(4.0)
        s = in_turn({"extents": lambda: kept.__setitem__("e", ix.extents(labels)), "pairs": pairs}, min(a.reps, 3))
        t = in_turn({"numpy": lambda: kept.__setitem__("n", numpy_extents(SUBSET, labels, *kept["p"]))}, 1)
        same = all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
                   for g, w in zip(kept["e"], kept["n"]))
        assert same, "Index.extents and the numpy route disagree"
        ratio = (s["pairs"]["median"] + t["numpy"]["median"]) / s["extents"]["median"]
        results.append(dict(kind="numpy", burst=burst, labels=name, pairs=int(len(kept["p"][0])), extents=s["extents"], pairs_us=s["pairs"],
                            numpy_us=t["numpy"], ratio=round(ratio, 1)))
        say("%6d %-8s %10d %30s %30s %30s %10.1f" % (burst, name, len(kept["p"][0]), fmt(s["extents"]), fmt(s["pairs"]), fmt(t["numpy"]), ratio))
        kept.clear()
        ix.close()
    clip.close()
    say()
    say(json.dumps(dict(radius=RADIUS, reps=a.reps, rows=results)))
    out.close()


if __name__ == "__main__":
    main()
