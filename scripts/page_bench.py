"""Selection at any depth (k_select.hip: Index.search_page_device / select_device) against its yardsticks, measured in one run and
written to profiles/page_bench.txt (--out).

    python scripts/page_bench.py [--quick] [--reps N] [--out FILE]

Points: f16 and i8, dim 512, N = 65 536 and 1 048 576 (--quick: 65 536 only), 1, 16 and 256 queries, over seeded random unit rows made
on the device (no two rows at the same distance: the tie runs the id digits exist for are the tests' business, not a cost).
Timed, per point:
  page      search_page_device at offsets 0 and 10 000, k = 100 and 1024
  select    select_device, one rank (10 000) per query
Yardsticks:
  search    search_device with the same k (what offset 0 costs today)
  rank      one rank_device call of as many columns (one target per query): one sweep without selection.  `sweeps` is the number of
            sweeps the call makes (4 + the id digits of N, a page one more); page / (sweeps x rank) says whether "a pass costs about one
            rank sweep" holds: 1 if it does.
  range     N = 65 536, 1 and 16 queries only: Index.range_search(q, 4.0) and a host lexsort per query, the exhaustive route to the same
            hits (host form, wall time with the copies).
A time is the wall time of `iters` calls enqueued back to back and ended by one synchronise of the context's stream, divided by iters:
it includes the launches a call makes (a page enqueues up to 18), which is what a caller pays.  A figure is the median of --reps such
windows with (min ... max) behind it, the things compared taken in turn.  Before anything is timed each point checks, bit for bit, that
the page at offset 0 is search's result and that select(10 000) is the first entry of the page at 10 000.
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

DIM = 512
DEEP = 10000


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def fmt(s):
    return "%9.1f (%.1f ... %.1f)" % (s["median"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_bench.txt"))
    a = ap.parse_args()
    from oracle import fixtures
    if clip_cpp_amd.device_count() < 1:
        raise RuntimeError("page_bench: no HIP device")
    torch.cuda.init()
    clip = clip_cpp_amd.Clip(fixtures.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32"), verbosity=0,
                             device=0)
    out = open(a.out, "w")
    rows_out = []

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def wall_us(f, iters):
        clip.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            f()
        clip.synchronize()
        return (time.perf_counter() - t0) * 1e6 / iters

    say("# scripts/page_bench.py%s on %s" % (" --quick" if a.quick else "", torch.cuda.get_device_name(0)))
    say("# dim %d; us per call, median (min ... max) of %d windows of back-to-back calls ended by one synchronise" % (DIM, a.reps))
    for n in (1 << 16,) if a.quick else (1 << 16, 1 << 20):
        gen = torch.Generator(device="cuda").manual_seed(n)
        for dt in ("f16", "i8"):
            ix = clip_cpp_amd.Index(clip, DIM, dt)
            for r0 in range(0, n, 1 << 16):
                block = torch.nn.functional.normalize(torch.randn(1 << 16, DIM, device="cuda", generator=gen), dim=1)
                torch.cuda.synchronize()
                ix.add_device(block.data_ptr(), block.shape[0])
                clip.synchronize()
            sweeps = 4 + (int(n - 1).bit_length() + 7) // 8
            for nq in (1, 16, 256):
                q = torch.nn.functional.normalize(torch.randn(nq, DIM, device="cuda", generator=gen), dim=1)
                dist, ids = torch.empty(nq * 1024, device="cuda"), torch.empty(nq * 1024, dtype=torch.int64, device="cuda")
                dist2, ids2 = torch.empty_like(dist), torch.empty_like(ids)
                ranks = torch.full((nq,), DEEP, dtype=torch.int64, device="cuda")
                targets = torch.randint(0, n, (nq,), device="cuda", generator=gen)
                torch.cuda.synchronize()
                qp, dp, ip = q.data_ptr(), dist.data_ptr(), ids.data_ptr()
                calls = {"select": lambda: ix.select_device(qp, nq, ranks.data_ptr(), dp, ip),
                         "rank": lambda: ix.rank_device(qp, nq, targets.data_ptr(), ip, dp)}
                for k in (100, 1024):
                    calls["search k%d" % k] = lambda k=k: ix.search_device(qp, nq, k, dp, ip)
                    for off in (0, DEEP):
                        calls["page k%d @%d" % (k, off)] = lambda k=k, off=off: ix.search_page_device(qp, nq, k, dp, ip, offset=off)
                # results must not differ: offset 0 is search, select is the head of its page
                ix.search_device(qp, nq, 100, dp, ip)
                ix.search_page_device(qp, nq, 100, dist2.data_ptr(), ids2.data_ptr())
                clip.synchronize()
                assert torch.equal(ids[:nq * 100], ids2[:nq * 100]) and torch.equal(dist[:nq * 100].view(torch.int32), dist2[:nq * 100].view(torch.int32))
                ix.select_device(qp, nq, ranks.data_ptr(), dp, ip)
                ix.search_page_device(qp, nq, 1, dist2.data_ptr(), ids2.data_ptr(), offset=DEEP)
                clip.synchronize()
                assert torch.equal(ids[:nq], ids2[:nq]) and torch.equal(dist[:nq].view(torch.int32), dist2[:nq].view(torch.int32))
                iters = {}
                for name, f in calls.items():                      # warm-up, and windows of about 50 ms
                    iters[name] = int(min(200, max(3, 50000.0 / max(wall_us(f, 3), 1.0))))
                got = {name: [] for name in calls}
                for _ in range(a.reps):
                    for name, f in calls.items():
                        got[name].append(wall_us(f, iters[name]))
                s = {name: stats(v) for name, v in got.items()}
                r = dict(dtype=dt, n=n, nq=nq, sweeps_select=sweeps, sweeps_page=sweeps + 1, **s)
                say("%-4s N %8d nq %4d   sweeps: select %d, page %d" % (dt, n, nq, sweeps, sweeps + 1))
                for name in calls:
                    say("    %-16s %s" % (name, fmt(s[name])))
                rank = s["rank"]["median"]
                r["select_over_sweeps_x_rank"] = round(s["select"]["median"] / (sweeps * rank), 3)
                say("    select / (%d x rank)                 %.3f" % (sweeps, r["select_over_sweeps_x_rank"]))
                for k in (100, 1024):
                    for off in (0, DEEP):
                        p = s["page k%d @%d" % (k, off)]["median"]
                        r["page_k%d_at%d_over_sweeps_x_rank" % (k, off)] = round(p / ((sweeps + 1) * rank), 3)
                        r["page_k%d_at%d_over_search" % (k, off)] = round(p / s["search k%d" % k]["median"], 3)
                        say("    page k%d @%d: / (%d x rank) %.3f, / search k%d %.3f" % (k, off, sweeps + 1, r["page_k%d_at%d_over_sweeps_x_rank" % (k, off)],
                                                                                      k, r["page_k%d_at%d_over_search" % (k, off)]))
                if n == 1 << 16 and nq <= 16:                      # the exhaustive route: every distance off the device, a host sort
                    qh = q.cpu().numpy()
                    ex = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        lims, d, i = ix.range_search(qh, 4.0)
                        for lo, hi in zip(lims[:-1], lims[1:]):
                            np.lexsort((i[lo:hi], d[lo:hi]))[DEEP:DEEP + 1024]
                        ex.append((time.perf_counter() - t0) * 1e6)
                    r["range_and_sort"] = stats(ex)
                    say("    %-16s %s   (host form, wall; / page k1024 @%d: %.1f)" % ("range + sort", fmt(r["range_and_sort"]), DEEP,
                                                                                   r["range_and_sort"]["median"] / s["page k1024 @%d" % DEEP]["median"]))
                rows_out.append(r)
            ix.close()
    say()
    say("# json: " + json.dumps(rows_out))
    out.close()
    clip.close()


if __name__ == "__main__":
    main()
