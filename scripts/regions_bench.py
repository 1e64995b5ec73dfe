"""Regions through the encoder and grouped search: what the two pieces of a region index cost.

    python scripts/regions_bench.py [--repeats 5] [--files 256] [--threads 16] [--rows 1000000] [--skip-files] [--skip-search]
                                    [--out profiles/regions_bench.txt]

1. Grid encode over files.  Folders of JPEGs at 640x480 and at 1600x1200 (4:2:0, quality 85, written with PIL into a temporary directory),
   model: the ViT-B/32-shaped synthetic q4_0 model of clip_cpp_amd.synth (vision tower only), windows of 64 images.  Routes:
    crops   what a caller could do before: clip_image_load_from_file per file and the 1 + 3 x 3 boxes copied out on the host, on a pool of
            T host threads (the load and the copies run outside the interpreter lock), then clip_amd_image_batch_encode_u8 over the crops
    grid=3  Clip.encode_image_files(grid=3, n_threads=T): threaded decode, the JPEG pixel half on the GPU once per image, every region read
            from the uploaded (or device-made) pixels
    grid=1  Clip.encode_image_files(n_threads=T) without regions: the same decoding, a tenth of the rows
   crops and grid=3 run with T = 1 and with T = --threads, so every comparison is between routes with the same thread count; every line
   names its T.  What the threaded decode and the device JPEG half gain on their own is profiles/files_bench.txt, not this file.
   A measurement times as many whole passes over the folder as take about half a second; interleaved repeats, medians, spread = (max -
   min) / median.  grid=3 and crops give the same rows (checked on the first window).
2. Grouped search.  clip_amd_bench_search_grouped against clip_amd_bench_search at the same n, dim, dtype and k (same seeded rows and
   queries; both scans read the same rows, so the difference is the selection and the merge): HIP-event microseconds per search,
   median of the repeats, group sizes 1 (the result equals the plain search's) and 10."""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clip_cpp_amd                      # noqa: E402
from clip_cpp_amd import synth           # noqa: E402
from files_bench import make_folder      # noqa: E402  (the same folders as scripts/files_bench.py)

BATCH = 64
GRID = 3


def load(L, path):
    im = L.clip_image_u8_make()
    try:
        if not L.clip_image_load_from_file(os.fsencode(path), im):
            return None
        c = im.contents
        return np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    finally:
        L.clip_image_u8_free(im)


def load_and_crop(L, path):
    img = load(L, path)
    if img is None:
        return []
    return [np.ascontiguousarray(img[y:y + h, x:x + w]) for x, y, w, h in clip_cpp_amd.grid_boxes(img.shape[1], img.shape[0], GRID).tolist()]


def route_crops(clip, L, paths, pool):
    """pool: a ThreadPoolExecutor of T threads that load and crop, or None for one thread"""
    out = []
    for pos in range(0, len(paths), BATCH):
        window = paths[pos:pos + BATCH]
        per_file = pool.map(lambda p: load_and_crop(L, p), window) if pool else [load_and_crop(L, p) for p in window]
        out.append(clip.encode_images_u8([c for crops in per_file for c in crops], normalize=True))
    return np.concatenate(out)


def route_files(clip, paths, threads, grid):
    out, pos, prepared = [], 0, clip.ImageFileList(paths)
    while pos < len(paths):
        res = clip.encode_image_files(prepared, normalize=True, n_threads=threads, max_images=BATCH, start=pos, grid=grid)
        out.append(res[0])
        pos += res[2]
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if not a.skip_files:
        L = clip_cpp_amd.lib()
        model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "b32", "q4_0", text=False, vision=True)
        clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
        R = 1 + GRID * GRID
        T = a.threads
        pool = ThreadPoolExecutor(max_workers=T)
        say("regions_bench 1: grid encode over files: %d JPEGs per folder, windows of %d images, T = 1 and T = %d host threads, %d interleaved repeats,"
            " model b32 q4_0 (synthetic)" % (a.files, BATCH, T, a.repeats))
        routes = [("crops, T = 1: load + host crops + encode_u8", lambda p: route_crops(clip, L, p, None), R),
                  ("grid=%d, T = 1: encode_image_files" % GRID, lambda p: route_files(clip, p, 1, GRID), R),
                  ("crops, T = %d: load + host crops + encode_u8" % T, lambda p: route_crops(clip, L, p, pool), R),
                  ("grid=%d, T = %d: encode_image_files" % (GRID, T), lambda p: route_files(clip, p, T, GRID), R),
                  ("grid=1, T = %d: encode_image_files" % T, lambda p: route_files(clip, p, T, 1), 1)]
        with tempfile.TemporaryDirectory() as tmp:
            for fname, h, w in (("jpeg 640x480", 480, 640), ("jpeg 1600x1200", 1200, 1600)):
                paths = make_folder(tmp, "j%d" % w, a.files, h, w)
                ref = routes[0][1](paths[:BATCH])                        # warm-up, and the rows the grid call must give
                same = all(np.array_equal(fn(paths[:BATCH]).view(np.uint32), ref.view(np.uint32)) for _, fn, rows in routes[1:] if rows == R)
                routes[4][1](paths[:BATCH])
                passes = {}
                for rname, fn, _ in routes:                              # one untimed-for-the-record pass sizes the measurement: about 0.5 s
                    t0 = time.perf_counter()
                    fn(paths)
                    passes[rname] = max(1, int(math.ceil(0.5 / max(time.perf_counter() - t0, 1e-4))))
                times = {r[0]: [] for r in routes}
                for _ in range(a.repeats):
                    for rname, fn, _ in routes:
                        t0 = time.perf_counter()
                        for _ in range(passes[rname]):
                            fn(paths)
                        times[rname].append((time.perf_counter() - t0) / passes[rname])
                say()
                say("%s: %d files; first window, every grid=%d and crops route against the serial crop loop: %s"
                    % (fname, len(paths), GRID, "same bits" if same else "DIFFERENT ROWS"))
                for rname, _, rows in routes:
                    v = times[rname]
                    med = statistics.median(v)
                    say("  %-46s %8.1f img/s %9.1f rows/s  (median of %d x %d passes: %.3f s per pass, spread %4.1f %%)"
                        % (rname, len(paths) / med, len(paths) * rows / med, len(v), passes[rname], med, 100 * (max(v) - min(v)) / med))
                m = [statistics.median(times[r[0]]) for r in routes]
                say("  grid=%d over the crop loop at the same thread count: x%.2f images/s at T = 1, x%.2f at T = %d"
                    % (GRID, m[0] / m[1], m[2] / m[3], T))
                say("  grid=%d costs x%.2f of grid=1's time at T = %d for x%d the rows" % (GRID, m[3] / m[4], T, R))
                flush_out()
        pool.shutdown()
        clip.close()

    if not a.skip_search:
        say()
        say("regions_bench 2: grouped search against the plain search: n = %d rows, dim 512, microseconds per search (HIP events, 10 searches"
            " per measurement, median of %d measurements)" % (a.rows, a.repeats))
        say("  %-5s %4s %4s %12s %14s %8s %14s %8s" % ("dtype", "k", "nq", "plain us", "groups of 1", "ratio", "groups of 10", "ratio"))
        for dtype in ("f16", "i8"):
            for k in (10, 100):
                for nq in (1, 64):
                    plain, g1, g10 = [], [], []
                    for _ in range(a.repeats):                          # interleaved: drift hits the three alike
                        plain.append(clip_cpp_amd.bench_search(dtype, a.rows, 512, nq, k, 10))
                        g1.append(clip_cpp_amd.bench_search_grouped(dtype, a.rows, 512, nq, k, 1, 10))
                        g10.append(clip_cpp_amd.bench_search_grouped(dtype, a.rows, 512, nq, k, 10, 10))
                    if min(plain + g1 + g10) < 0:
                        say("  %-5s %4d %4d  a benchmark hook failed: %r" % (dtype, k, nq, (plain, g1, g10)))
                        continue
                    p, a1, a10 = statistics.median(plain), statistics.median(g1), statistics.median(g10)
                    say("  %-5s %4d %4d %12.1f %14.1f %7.2fx %14.1f %7.2fx" % (dtype, k, nq, p, a1, a1 / p, a10, a10 / p))
                    flush_out()
    flush_out()


if __name__ == "__main__":
    main()
