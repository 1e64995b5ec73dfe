"""Biased search of the exact index (k_bias.hip, Index.search_biased) against the search it is a variant of and the exact route that
existed before it, and Index.hubness against the cross-index call it contains, measured in one run and written to
profiles/bias_bench.txt (--out).

    python scripts/bias_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), 1, 16 and 256 queries, k = 10 and 100, seeded normal rows,
bias uniform in [-0.3, 0.3).  What is timed is the host call, wall time, results on the host:
(a) biased   Index.search_biased(q, k, bias)
(b) search   Index.search(q, k) on the same index with the same queries: the parent's code path
(n) no column Index.search_biased(q, k, None): the plain search through the biased host form (three result arrays), so (a) - (n) is what
             the column costs a host call (its check, its upload, the biased scan and finish) and (n) - (b) what the form costs
(c) range    the exact route that existed: Index.range_search(q, 4.0) (every distance leaves the device), a numpy f32 add of the bias and a
             lexsort by (score, id) per query, at N = 65 536 only (at 1 048 576 rows x 256 queries the hit list is 3 GB)
hubness: Index.hubness(bank) over a bank of 4096 rows, CSLS (k 10) against bank.search_index(ix, 10), inverted softmax against
bank.softmax_index(ix, 1), the calls they contain plus the fold and a column of 4 bytes per row in the place of [N, k] results.

A figure is the time per call, the median of --reps repetitions with (min ... max) behind it; a repetition of a short call times a batch
of calls that fills about 20 ms, after a warm call, and the repetitions of the things compared are taken in turn.
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

DIM, BANK = 512, 4096


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def wall_us(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e6


BATCH_US = 20000.0       # wall time a timed window of a short call is brought to, by repeating the call


def in_turn(calls, reps):
    """{name: stats} of the wall time per call, each call warmed once; a repetition times a batch of calls (as many as bring the window to
    about BATCH_US, from one trial call; a call longer than that is timed alone) and the repetitions of the calls are taken in turn"""
    batch = {}
    for k, f in calls.items():
        f()
        batch[k] = max(1, min(200, int(BATCH_US / max(wall_us(f), 1.0))))
    got = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            got[k].append(wall_us(lambda: [f() for _ in range(batch[k])]) / batch[k])
    return {k: stats(v) for k, v in got.items()}


def range_route(ix, q, k, bias):
    lims, d, ids = ix.range_search(q, 4.0)
    for i in range(len(q)):
        s = d[lims[i]:lims[i + 1]] + bias[ids[lims[i]:lims[i + 1]]]
        np.lexsort((ids[lims[i]:lims[i + 1]], s))[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/bias_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d; host-call wall time per call, us, median (min ... max) of %d repetitions of a ~20 ms batch of calls, taken in turn" % (DIM, a.reps))
    say("%-4s %8s %4s %4s %34s %34s %7s %34s %34s %7s" % ("dt", "N", "nq", "k", "biased", "search", "a/b", "no column", "range + numpy", "c/a"))
    rng = np.random.default_rng(1)
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        rows = rng.standard_normal((n, DIM), dtype=np.float32)
        bank_rows = rng.standard_normal((BANK, DIM), dtype=np.float32)
        bias = rng.uniform(-0.3, 0.3, n).astype(np.float32)
        for dt in ("f16", "i8"):
            ix, bank = clip_cpp_amd.Index(clip, DIM, dt), clip_cpp_amd.Index(clip, DIM, dt)
            ix.add(rows)
            bank.add(bank_rows)
            for nq in (1, 16, 256):
                q = rng.standard_normal((nq, DIM), dtype=np.float32)
                for k in (10, 100):
                    calls = dict(biased=lambda: ix.search_biased(q, k, bias), search=lambda: ix.search(q, k), none=lambda: ix.search_biased(q, k, None))
                    if n == 1 << 16:
                        calls["range"] = lambda: range_route(ix, q, k, bias)
                    s = in_turn(calls, a.reps)
                    r = dict(dtype=dt, n=n, nq=nq, k=k, biased_over_search=round(s["biased"]["median"] / s["search"]["median"], 3), **s)
                    if "range" in s:
                        r["range_over_biased"] = round(s["range"]["median"] / s["biased"]["median"], 2)
                    rows_out.append(r)
                    say("%-4s %8d %4d %4d %34s %34s %7.3f %34s %34s %7s" % (dt, n, nq, k, fmt(s["biased"]), fmt(s["search"]), r["biased_over_search"],
                                                                           fmt(s["none"]), fmt(s["range"]) if "range" in s else "not run", r.get("range_over_biased", "-")))
            h = in_turn(dict(csls=lambda: ix.hubness(bank, "csls", k=10), search_index=lambda: bank.search_index(ix, 10),
                             softmax=lambda: ix.hubness(bank, "softmax", scale=100.0), softmax_index=lambda: bank.softmax_index(ix, 1, 100.0)), a.reps)
            r = dict(dtype=dt, n=n, bank=BANK, csls_over_search_index=round(h["csls"]["median"] / h["search_index"]["median"], 3),
                     softmax_over_softmax_index=round(h["softmax"]["median"] / h["softmax_index"]["median"], 3), **h)
            rows_out.append(r)
            say("%-4s %8d hubness over a bank of %d: csls %s  search_index %s  ratio %.3f | softmax %s  softmax_index %s  ratio %.3f" % (
                dt, n, BANK, fmt(h["csls"]), fmt(h["search_index"]), r["csls_over_search_index"], fmt(h["softmax"]), fmt(h["softmax_index"]),
                r["softmax_over_softmax_index"]))
            ix.close()
            bank.close()
    say()
    say("# device time (HIP events) of the searches alone, the bias column already on the device: clip_amd_bench_search_biased against")
    say("# clip_amd_bench_search over the same seeded rows and queries; what the host form adds on top is the column's upload and check")
    say("%-4s %8s %4s %4s %34s %34s %7s" % ("dt", "N", "nq", "k", "biased (device)", "search (device)", "a/b"))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        for dt in ("f16", "i8"):
            for nq in (1, 16, 256):
                for k in (10, 100):
                    got = dict(biased=[], search=[])
                    for _ in range(a.reps):
                        got["biased"].append(clip_cpp_amd.bench_search_biased(dt, n, DIM, nq, k, 20))
                        got["search"].append(clip_cpp_amd.bench_search(dt, n, DIM, nq, k, 20))
                    if min(min(v) for v in got.values()) < 0:
                        raise RuntimeError("a benchmark hook failed: %r" % (got,))
                    s = {key: stats(v) for key, v in got.items()}
                    r = dict(device=True, dtype=dt, n=n, nq=nq, k=k, biased_over_search=round(s["biased"]["median"] / s["search"]["median"], 3), **s)
                    rows_out.append(r)
                    say("%-4s %8d %4d %4d %34s %34s %7.3f" % (dt, n, nq, k, fmt(s["biased"]), fmt(s["search"]), r["biased_over_search"]))
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()
    clip.close()


if __name__ == "__main__":
    main()
