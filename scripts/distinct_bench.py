"""Distinct search over the exact index: what the near bitmap and the walk cost on top of the search they follow, and what composing the
same answer on the host from the existing calls costs.

    python scripts/distinct_bench.py [--repeats 5] [--rows 100000,1000000] [--dtype f16] [--copies 4] [--radius 0.02]
                                     [--points 1:5:64,1:100:1024,256:10:80,256:100:1024] [--out profiles/distinct_bench.txt]

The gallery: rows in groups of copies + 1, a random unit vector followed by `copies` noisy copies of it (base + 0.1 / sqrt(dim) N(0, I):
a copy at distance ~0.005 from its base and ~0.01 from another copy, all within the radius), made on the device and added with
Index.add_device.  Queries: stored rows plus noise, so a burst leads every pool.  Every point (n_queries, k, pool) at dim 512 records
  distinct  wall microseconds of one Index.search_distinct_device followed by the context's synchronise
  search    the same for one Index.search_device with k = pool on the same index: the search that distinct contains, so distinct - search
            is what the near bitmap (distinct_near_kernel) and the walk (distinct_pick_kernel) add
  host      wall microseconds of the composition from the calls that existed before: Index.search with k = pool, per query
            Index.search_ids of the hits with the hits as `allow`, and the walk in numpy (per query: the near relation of a pool is its own)
Medians of --repeats measurements after one warm-up of each, the three interleaved in one process.  The results of the device call and
of the host route are compared once per point: they must be the same bits."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

if torch.cuda.is_available():
    torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clip_cpp_amd                      # noqa: E402
from clip_cpp_amd import synth           # noqa: E402

DIM = 512


def host_route(index, q, k, pool, radius):
    """(distances, ids, counts) from search, search_ids and a walk in numpy"""
    dist, ids = index.search(q, pool)
    nq = len(q)
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_c = np.zeros((nq, k), dtype=np.int32)
    r = np.float32(radius)
    for t in range(nq):
        members = ids[t][ids[t] >= 0]
        m = len(members)
        nd, ni = index.search_ids(members, max(m - 1, 1), exclude_self=True, allow=members)
        rank = {int(x): a for a, x in enumerate(members)}
        near = np.zeros((m, m), dtype=bool)
        hit = (ni > members[:, None]) & (nd <= r)              # the entry whose query id is lower than its row id
        for a, c in zip(*np.nonzero(hit)):
            b = rank[int(ni[a, c])]
            near[a, b] = near[b, a] = True
        suppressed = np.zeros(m, dtype=bool)
        kept = 0
        for a in range(m):
            if kept == k:
                break
            if suppressed[a]:
                continue
            mine = near[a] & ~suppressed
            mine[:a + 1] = False
            out_d[t, kept], out_i[t, kept], out_c[t, kept] = dist[t, a], members[a], int(mine.sum())
            suppressed |= mine
            kept += 1
    return out_d, out_i, out_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--radius", type=float, default=0.02)
    ap.add_argument("--points", default="1:5:64,1:100:1024,256:10:80,256:100:1024")
    ap.add_argument("--host-queries", type=int, default=16, help="queries of a point the host route is timed on (its time is scaled to the point)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    points = [tuple(int(v) for v in p.split(":")) for p in a.points.split(",") if p]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    say("distinct_bench: Index.search_distinct_device against the search it contains and against the host composition; %s rows of dim %d in"
        " groups of 1 + %d copies, radius %g, microseconds (wall, each call followed by a synchronise), medians of %d interleaved measurements"
        % (a.dtype, DIM, a.copies, a.radius, a.repeats))
    say("  host route: Index.search (k = pool), per query Index.search_ids of the hits with the hits as allow, the walk in numpy; timed on at"
        " most %d queries of the point and scaled to its n_queries (the route is a loop over queries)" % a.host_queries)
    say("  %8s %5s %5s %5s %12s %12s %10s %8s %14s %9s %6s" % ("rows", "nq", "k", "pool", "distinct us", "search us", "added us", "added %",
                                                           "host route us", "x distinct", "same"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for n in [int(v) for v in a.rows.split(",") if v]:
        index = clip_cpp_amd.Index(clip, DIM, a.dtype)
        per = a.copies + 1
        piece = 65536 // per * per                             # whole groups per add
        sample = None
        for r0 in range(0, n, piece):
            m = min(piece, n - r0)
            g = (m + per - 1) // per
            base = torch.randn((g, DIM), generator=gen, device="cuda", dtype=torch.float32)
            base = base / base.norm(dim=1, keepdim=True)
            rows = base[:, None, :] + (0.1 / DIM ** 0.5) * torch.randn((g, per, DIM), generator=gen, device="cuda", dtype=torch.float32)
            rows[:, 0, :] = base
            rows = rows.reshape(-1, DIM)[:m].contiguous()
            torch.cuda.synchronize()
            index.add_device(rows.data_ptr(), m)
            clip.synchronize()
            if sample is None:
                sample = rows[:4096].clone()
        for nq, k, pool in points:
            pick = torch.randint(0, len(sample), (nq,), generator=gen, device="cuda")
            tq = (sample[pick] + (0.3 / DIM ** 0.5) * torch.randn((nq, DIM), generator=gen, device="cuda", dtype=torch.float32)).contiguous()
            q = tq.cpu().numpy()
            td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            tc = torch.empty((nq, k), dtype=torch.int32, device="cuda")
            pd = torch.empty((nq, pool), dtype=torch.float32, device="cuda")
            pi = torch.empty((nq, pool), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            hq = min(nq, a.host_queries)

            def distinct():
                index.search_distinct_device(tq.data_ptr(), nq, k, a.radius, td.data_ptr(), ti.data_ptr(), tc.data_ptr(), pool=pool)
                clip.synchronize()

            def search():
                index.search_device(tq.data_ptr(), nq, pool, pd.data_ptr(), pi.data_ptr())
                clip.synchronize()

            def timed(f):
                t0 = time.perf_counter()
                r = f()
                return (time.perf_counter() - t0) * 1e6, r

            distinct()
            search()
            want = host_route(index, q[:hq], k, pool, a.radius)
            got = (td[:hq].cpu().numpy(), ti[:hq].cpu().numpy(), tc[:hq].cpu().numpy())
            same = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(got, want))
            folded = float(got[2].sum()) / max(1, int((got[1] >= 0).sum()))
            ds, ss, hs = [], [], []
            for _ in range(a.repeats):
                ds.append(timed(distinct)[0])
                ss.append(timed(search)[0])
                hs.append(timed(lambda: host_route(index, q[:hq], k, pool, a.radius))[0] * nq / hq)
            d, s, h = statistics.median(ds), statistics.median(ss), statistics.median(hs)
            say("  %8d %5d %5d %5d %12.1f %12.1f %10.1f %7.1f%% %14.1f %8.1fx %6s   (%.2f rows folded per hit)"
                % (n, nq, k, pool, d, s, d - s, 100 * (d - s) / s, h, h / d, "yes" if same else "NO", folded))
            flush_out()
        index.close()
    clip.close()
    flush_out()


if __name__ == "__main__":
    main()
