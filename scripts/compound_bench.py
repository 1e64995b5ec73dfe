"""Compound queries over the exact index: what one Index.search_compound_device costs against the plain scan work it contains, and against
the only exact composition of the same answer from the calls that existed before.

    python scripts/compound_bench.py [--repeats 7] [--rows 1000000] [--dtypes f16,i8] [--ks 10,100] [--terms 2,4,8] [--queries 1,16,256]
                                     [--fold-entries 40000000] [--out profiles/compound_bench.txt]

The gallery: seeded random unit rows of dim 512, made on the device and added with Index.add_device.  Terms: seeded random vectors, every
term an "all" term (the fold of a filter term is one compare more per row; the row traffic and the MFMA chain are the same).  Every point
(dtype, k, terms, n_queries) records
  compound  wall microseconds of one Index.search_compound_device followed by the context's synchronise
  (a) plain the same for one Index.search_device of the n_queries x terms term vectors as plain queries at the same k: the scan work the
            compound call contains (as many query rows against every stored row), without the fold
  (b) fold  host forms on both sides: Index.search_compound against Index.range_search of all terms at radius 4 (every row's distance to
            every term, n x terms x n_queries entries to the host) plus the fold in numpy (scatter, max over the terms, the k best by
            (score, id)).  Only at the points whose entries fit --fold-entries; the results of the two are compared once: the same bits.
Medians of --repeats measurements after a warm-up of each, the calls of a point interleaved in one process; next to every ratio the
spread: the lowest and highest ratio of a pair of neighbouring measurements."""
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


def fold(index, terms, nq, n_terms, k):
    """(distances, ids) of all-of queries from range_search at radius 4 and numpy"""
    n = len(index)
    lims, dist, ids = index.range_search(terms, 4.0)
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for c in range(nq):
        score = np.full(n, -np.inf, dtype=np.float32)
        seen = np.zeros(n, dtype=np.int32)
        for t in range(c * n_terms, (c + 1) * n_terms):
            rows = ids[lims[t]:lims[t + 1]]
            d = np.full(n, np.inf, dtype=np.float32)
            d[rows] = dist[lims[t]:lims[t + 1]]
            np.maximum(score, d, out=score)
            seen[rows] += 1
        score[seen < n_terms] = np.inf
        kk = min(k, n)
        part = np.argpartition(score, kk - 1)[:kk] if kk < n else np.arange(n)
        cut = score[part].max()
        cand = np.flatnonzero(score <= cut)                      # every row at the cut's score, so that ties break by id
        cand = cand[np.lexsort((cand, score[cand]))][:kk]
        cand = cand[np.isfinite(score[cand])]
        out_d[c, :len(cand)], out_i[c, :len(cand)] = score[cand], cand
    return out_d, out_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dtypes", default="f16,i8")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--terms", default="2,4,8")
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--fold-entries", type=int, default=40000000, help="(b) is measured where rows x terms x queries is at most this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",") if v]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e6

    def ratio(xs, ys):
        """median(xs) / median(ys) and the lowest and highest xs[i] / ys[i] of the interleaved pairs"""
        pairs = [x / y for x, y in zip(xs, ys)]
        return statistics.median(xs) / statistics.median(ys), min(pairs), max(pairs)

    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "tiny", "f32")
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    n = a.rows
    say("compound_bench: Index.search_compound_device against (a) Index.search_device over n_queries x terms plain queries at the same k and"
        " (b) host forms: Index.search_compound against Index.range_search at radius 4 of all terms + the fold in numpy; %d random unit rows of"
        " dim %d, every term an all-term; microseconds (wall, each device call followed by a synchronise), medians of %d interleaved"
        " measurements; [lo .. hi]: the lowest and highest ratio of one interleaved pair" % (n, DIM, a.repeats))
    say("  (b) only where rows x terms x queries <= %d entries (12 bytes each on the host); '-' = not measured" % a.fold_entries)
    say("  %5s %4s %5s %4s %12s %12s %22s %14s %14s %22s %5s" % ("dtype", "k", "terms", "nq", "compound us", "(a) plain us", "compound / (a)",
                                                               "host form us", "(b) fold us", "(b) / host form", "same"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    for dtype in a.dtypes.split(","):
        index = clip_cpp_amd.Index(clip, DIM, dtype)
        for r0 in range(0, n, 65536):
            m = min(65536, n - r0)
            rows = torch.randn((m, DIM), generator=gen, device="cuda", dtype=torch.float32)
            torch.cuda.synchronize()
            index.add_device(rows.data_ptr(), m)
            clip.synchronize()
        for k in ints(a.ks):
            for n_terms in ints(a.terms):
                for nq in ints(a.queries):
                    total = nq * n_terms
                    tq = torch.randn((total, DIM), generator=gen, device="cuda", dtype=torch.float32)
                    terms = tq.cpu().numpy()
                    kinds = np.zeros(total, dtype=np.int32)
                    bounds = np.zeros(total, dtype=np.float32)
                    lims = np.arange(nq + 1, dtype=np.int64) * n_terms
                    cd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                    ci = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                    pd = torch.empty((total, k), dtype=torch.float32, device="cuda")
                    pi = torch.empty((total, k), dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    queries = [[(terms[c * n_terms + t], "all") for t in range(n_terms)] for c in range(nq)]

                    def compound():
                        index.search_compound_device(tq.data_ptr(), None, kinds, bounds, lims, k, cd.data_ptr(), ci.data_ptr())
                        clip.synchronize()

                    def plain():
                        index.search_device(tq.data_ptr(), total, k, pd.data_ptr(), pi.data_ptr())
                        clip.synchronize()

                    compound()
                    plain()
                    cs, ps = [], []
                    for _ in range(a.repeats):
                        cs.append(timed(compound))
                        ps.append(timed(plain))
                    r, lo, hi = ratio(cs, ps)
                    host = folded = "-"
                    rb = same = "-"
                    if n * total <= a.fold_entries:
                        got = index.search_compound(queries, k)
                        want = fold(index, terms, nq, n_terms, k)
                        same = "yes" if np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) else "NO"
                        hs, fs = [], []
                        for _ in range(max(3, a.repeats // 2)):
                            hs.append(timed(lambda: index.search_compound(queries, k)))
                            fs.append(timed(lambda: fold(index, terms, nq, n_terms, k)))
                        rr, rlo, rhi = ratio(fs, hs)
                        host, folded = "%.1f" % statistics.median(hs), "%.1f" % statistics.median(fs)
                        rb = "%.1fx [%.1f .. %.1f]" % (rr, rlo, rhi)
                    say("  %5s %4d %5d %4d %12.1f %12.1f %22s %14s %14s %22s %5s" % (dtype, k, n_terms, nq, statistics.median(cs), statistics.median(ps),
                                                                               "%.3f [%.3f .. %.3f]" % (r, lo, hi), host, folded, rb, same))
                    flush_out()
        index.close()
    clip.close()
    flush_out()


if __name__ == "__main__":
    main()
