"""Class probabilities of the exact index (k_classes.hip, Index.class_probs) against three yardsticks, measured in one run and written to
profiles/classes_bench.txt (--out).

    python scripts/classes_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), 1, 16 and 256 queries, 16 and 512 classes (random labels),
scale 100, m = 1, no matrix.  Every figure is the wall time of a host call through Index (queries up, results back), microseconds, the
median of --reps calls with (min ... max) behind it, the calls of the things compared taken in turn.  Yardsticks:
(a) softmax  Index.softmax with the same queries and k = 1: the sweep this one extends.  classes / softmax shows what the accumulation
             into the LDS table costs over one register per column.
(b) vote     Index.vote with k = 16, m = 1: the hard vote over the same labels.
(c) torch    what a user would write without the entry point: the rows as an [N, dim] f16 tensor on the device, s = q @ rows.T,
             exp(100 (s - max)), index_add_ into [nq, classes], normalise; device time between two events.  Not bit-exact with the index,
             there for the time only; f16 rows for both dtypes.
device       clip_amd_bench_class_probs: device time (HIP events, 20 calls) of clip_amd_index_class_probs_device over the seeded rows and
             hashed labels of the hook, the same N, queries and class count: the call without the uploads and the wait ("-" for "one",
             which the hook does not make).
Worst case: "one" = 512 classes with every row in class 0 (one row in class 511), where 16 lanes of a turn hit one class.
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

DIM, SCALE = 512, 100.0


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%10.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def wall_us(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e6


def device_us(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def torch_classes(rows, q, labels, n_classes):
    s = (q @ rows.T).float()
    w = torch.exp(SCALE * (s - s.max(dim=1, keepdim=True).values))
    acc = torch.zeros(q.shape[0], n_classes, device=q.device).index_add_(1, labels, w)
    return acc / acc.sum(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# scripts/classes_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d, scale %g, m 1; us per host call (torch: device time), median (min ... max) of %d, taken in turn" % (DIM, SCALE, a.reps))
    say("%-4s %8s %4s %5s %34s %34s %7s %34s %7s %34s %7s %9s" % ("dt", "N", "nq", "cls", "class_probs", "softmax (k 1)", "cp/a", "vote (k 16)", "cp/b",
                                                                  "torch (f16 rows)", "c/cp", "device"))
    clip = clip_cpp_amd.Clip(synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32"), verbosity=0, device=0)
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        rng = np.random.default_rng(n)
        host = rng.standard_normal((n, DIM), dtype=np.float32)
        rows = torch.nn.functional.normalize(torch.from_numpy(host).cuda(), dim=1).to(torch.float16)
        for dt in ("f16", "i8"):
            ix = clip_cpp_amd.Index(clip, DIM, dt)
            ix.add(host)
            for nq in (1, 16, 256):
                q = rng.standard_normal((nq, DIM), dtype=np.float32)
                dq = torch.nn.functional.normalize(torch.from_numpy(q).cuda(), dim=1).to(torch.float16)
                for name, n_classes in (("16", 16), ("512", 512), ("one", 512)):
                    labels = rng.integers(0, n_classes, n).astype(np.int32) if name != "one" else np.zeros(n, dtype=np.int32)
                    labels[-1] = n_classes - 1
                    dl = torch.from_numpy(labels.astype(np.int64)).cuda()
                    calls = dict(classes=lambda: wall_us(lambda: ix.class_probs(q, labels, scale=SCALE)),
                                 softmax=lambda: wall_us(lambda: ix.softmax(q, 1, scale=SCALE)),
                                 vote=lambda: wall_us(lambda: ix.vote(q, 16, labels)),
                                 torch=lambda: device_us(lambda: torch_classes(rows, dq, dl, n_classes)))
                    for f in calls.values():                           # warm: workspaces, code objects
                        f()
                    got = {k: [] for k in calls}
                    for _ in range(a.reps):
                        for k, f in calls.items():
                            got[k].append(f())
                    s = {k: stats(v) for k, v in got.items()}
                    dev = clip_cpp_amd.bench_class_probs(dt, n, DIM, nq, n_classes, 20) if name != "one" else None
                    if dev is not None and dev < 0:
                        raise RuntimeError("clip_amd_bench_class_probs failed: %r" % dev)
                    r = dict(dtype=dt, n=n, nq=nq, classes_case=name, device_us=None if dev is None else round(dev, 1), over_softmax=round(s["classes"]["median"] / s["softmax"]["median"], 3),
                             over_vote=round(s["classes"]["median"] / s["vote"]["median"], 3),
                             torch_over=round(s["torch"]["median"] / s["classes"]["median"], 3), **s)
                    rows_out.append(r)
                    say("%-4s %8d %4d %5s %34s %34s %7.3f %34s %7.3f %34s %7.3f %9s" % (dt, n, nq, name, fmt(s["classes"]), fmt(s["softmax"]), r["over_softmax"],
                                                                                      fmt(s["vote"]), r["over_vote"], fmt(s["torch"]), r["torch_over"],
                                                                                      "-" if dev is None else "%.1f" % dev))
            ix.close()
        del rows
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()
    clip.close()


if __name__ == "__main__":
    main()
