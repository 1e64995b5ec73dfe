"""Diversified (MMR) search over the exact index: what the fused walk of k_mmr.hip costs on top of the search it follows, against distinct
search with the same pool, its two routes against each other, and what composing the same answer on the host from the existing calls
costs.

    python scripts/mmr_bench.py [--repeats 7] [--calls 20] [--rows 65536,1048576] [--dtypes f16,i8] [--copies 4] [--lam 0.5]
                                [--points 1:16:128,16:16:128,256:16:128,16:128:1024] [--host-rows 65536] [--out profiles/mmr_bench.txt]

The gallery: rows in bursts of copies + 1, a random unit vector followed by `copies` noisy copies of it (base + 0.1 / sqrt(dim) N(0, I)),
made on the device and added with Index.add_device.  Queries: stored rows plus noise, so a burst leads every pool.  Every point
(n_queries, k, pool) at dim 512 records wall microseconds of one call followed by the context's synchronise:
  mmr        Index.search_mmr_device, automatic route
  search     Index.search_device with k = pool on the same index: the search that mmr contains, so mmr - search is the walk
  distinct   Index.search_distinct_device with the same k and pool (radius 0.02)
  resident   mmr with the route forced to resident ("-" where the pool does not fit the LDS: the library refuses that)
  streaming  mmr with the route forced to streaming
  host       the composition from the calls that existed before: Index.search with k = pool, per query Index.search_ids of the hits with
             the hits as `allow`, and the greedy loop in numpy float32; only at --host-rows rows, timed on at most --host-queries queries
             and scaled to the point
A measurement is the wall time of --calls calls in a row (each with its synchronise) over --calls.  Medians of --repeats measurements
after one warm-up of each, interleaved in one process; the resident and streaming columns also give the least and the largest measurement
(min..max), so that a difference between the two can be held against their spread.  The device result and the host route are
compared once per point where the host route runs, and the two routes at every point: they must be the same bits."""
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
LDS = 160 * 1024


def host_route(index, q, k, pool, lam):
    """(distances, ids, gaps) from search, search_ids and the greedy loop in numpy float32 (one rounding per operation)"""
    dist, ids = index.search(q, pool)
    nq = len(q)
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_g = np.full((nq, k), np.inf, dtype=np.float32)
    lam = np.float32(lam)
    mu = np.float32(1.0) - lam
    for t in range(nq):
        members = ids[t][ids[t] >= 0]
        m = len(members)
        nd, ni = index.search_ids(members, max(m - 1, 1), exclude_self=True, allow=members)
        rank = np.full(len(index), -1, dtype=np.int64)
        rank[members] = np.arange(m)
        pair = np.zeros((m, m), dtype=np.float32)
        a, c = np.nonzero(ni > members[:, None])               # the entry whose query id is lower than its row id
        b = rank[ni[a, c]]
        pair[a, b] = pair[b, a] = nd[a, c]
        gap = np.full(m, np.inf, dtype=np.float32)
        free = np.ones(m, dtype=bool)
        for s in range(min(k, m)):
            score = lam * dist[t, :m] - mu * (gap if s else np.zeros(m, dtype=np.float32))
            score[~free] = np.inf
            x = int(np.argmin(score))                          # the first of equal scores: the lower rank
            out_d[t, s], out_i[t, s], out_g[t, s] = dist[t, x], members[x], gap[x]
            free[x] = False
            gap = np.minimum(gap, pair[x])
    return out_d, out_i, out_g


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls in a row per measurement")
    ap.add_argument("--rows", default="65536,1048576")
    ap.add_argument("--dtypes", default="f16,i8")
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--points", default="1:16:128,16:16:128,256:16:128,16:128:1024")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--host-queries", type=int, default=4, help="queries of a point the host route is timed on (its time is scaled to the point)")
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
    L = clip_cpp_amd.lib()
    say("mmr_bench: Index.search_mmr_device (lambda %g) against the search it contains, distinct search with the same pool, its two routes"
        " and the host composition; rows of dim %d in bursts of 1 + %d copies, microseconds (wall, each call followed by a synchronise),"
        " medians of %d interleaved measurements of %d calls each; resident / streaming: median (min..max)" % (a.lam, DIM, a.copies, a.repeats, a.calls))
    say("  host route: Index.search (k = pool), per query Index.search_ids of the hits with the hits as allow, the greedy loop in numpy; at %d"
        " rows only, timed on at most %d queries of the point and scaled to its n_queries" % (a.host_rows, a.host_queries))
    say("  %5s %8s %4s %4s %5s %10s %10s %9s %11s %26s %26s %14s %8s %5s" % ("dtype", "rows", "nq", "k", "pool", "mmr us", "search us", "walk us",
                                                                            "distinct us", "resident us", "streaming us", "host route us", "x mmr", "same"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for dtype in [d for d in a.dtypes.split(",") if d]:
        es = {"f32": 4, "f16": 2, "i8": 1}[dtype]
        for n in [int(v) for v in a.rows.split(",") if v]:
            index = clip_cpp_amd.Index(clip, DIM, dtype)
            per = a.copies + 1
            piece = 65536 // per * per                         # whole bursts per add
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
                tg = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                tc = torch.empty((nq, k), dtype=torch.int32, device="cuda")
                pd = torch.empty((nq, pool), dtype=torch.float32, device="cuda")
                pi = torch.empty((nq, pool), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                fits = ((pool + 63) // 64 * 64) * 20 + 32 + pool * (DIM * es + 16) <= LDS      # (mmr_lds_bytes of k_mmr.hip)
                host = n == a.host_rows
                hq = min(nq, a.host_queries)

                def mmr(route=0):
                    assert L.clip_amd_test_index_mmr_route(index.handle, route) == route
                    index.search_mmr_device(tq.data_ptr(), nq, k, a.lam, td.data_ptr(), ti.data_ptr(), tg.data_ptr(), pool=pool)
                    clip.synchronize()
                    L.clip_amd_test_index_mmr_route(index.handle, 0)

                def result(route):
                    mmr(route)
                    return td.cpu().numpy(), ti.cpu().numpy(), tg.cpu().numpy()

                def distinct():
                    index.search_distinct_device(tq.data_ptr(), nq, k, 0.02, td.data_ptr(), ti.data_ptr(), tc.data_ptr(), pool=pool)
                    clip.synchronize()

                def search():
                    index.search_device(tq.data_ptr(), nq, pool, pd.data_ptr(), pi.data_ptr())
                    clip.synchronize()

                def timed(f, *args, calls=a.calls):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        f(*args)
                    return (time.perf_counter() - t0) * 1e6 / calls

                def spread(v):
                    return "%.1f (%.1f..%.1f)" % (statistics.median(v), min(v), max(v))

                distinct()
                search()
                got = result(2)
                same = (not fits or same_bits(result(1), got)) and same_bits(result(0), got)
                if host:
                    same = same and same_bits([x[:hq] for x in got], host_route(index, q[:hq], k, pool, a.lam))
                ms, ss, ds, rs, ts, hs = [], [], [], [], [], []
                for _ in range(a.repeats):
                    ms.append(timed(mmr))
                    ss.append(timed(search))
                    ds.append(timed(distinct))
                    if fits:
                        rs.append(timed(mmr, 1))
                    ts.append(timed(mmr, 2))
                    if host:
                        hs.append(timed(host_route, index, q[:hq], k, pool, a.lam, calls=1) * nq / hq)
                mm, s, d = (statistics.median(v) for v in (ms, ss, ds))
                say("  %5s %8d %4d %4d %5d %10.1f %10.1f %9.1f %11.1f %26s %26s %14s %8s %5s"
                    % (dtype, n, nq, k, pool, mm, s, mm - s, d, spread(rs) if fits else "-", spread(ts),
                       "%.1f" % statistics.median(hs) if host else "-", "%.1fx" % (statistics.median(hs) / mm) if host else "-",
                       "yes" if same else "NO"))
                flush_out()
            index.close()
    clip.close()
    flush_out()


if __name__ == "__main__":
    main()
