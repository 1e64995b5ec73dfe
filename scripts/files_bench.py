"""Files in, embeddings out: what the step in front of the encoder costs, and whether the JPEG pixel half belongs on the GPU.

    python scripts/files_bench.py [--repeats 3] [--files 256] [--out profiles/files_bench.txt]

Folders (written with PIL into a temporary directory): JPEGs at 640x480 and at 1600x1200 (4:2:0, quality 85), and one of mixed formats.
Model: the ViT-B/32-shaped synthetic q4_0 model of clip_cpp_amd.synth (vision tower only).
Routes, each walking a folder in windows of 64 loadable images, as `image_search build` does:
    A   clip_image_load_from_file per file on one thread, then clip_amd_image_batch_encode_u8 per 64 (what `build` did before)
    B   clip_amd_image_batch_encode_files with CLIP_AMD_JPEG_DEVICE=0 (every decoder's pixel half on the host threads), 1 / 4 / 16 threads
    C   the same call with CLIP_AMD_JPEG_DEVICE=1: the JPEG pixel half on the GPU (jpeg_idct_kernel + jpeg_rgb_kernel), 1 / 4 / 16 threads
The repeats are interleaved (A, B1, C1, B4, C4, B16, C16, then again): drift hits every route alike.  Reported: the median images/s of each
route and its spread ((max - min) / median over the repeats), the ratios to A, and the two kernels' own times from HIP events with the
bytes they must move.  All routes give the same embeddings (checked)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clip_cpp_amd                      # noqa: E402
from clip_cpp_amd import synth           # noqa: E402

BATCH = 64


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(np.sin(xx / 17.0 + yy / 31.0) * 0.5 + 0.5) * 255, (np.cos(yy / 13.0) * 0.5 + 0.5) * 255, (xx * 3 + yy * 5) % 256], -1)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def make_folder(base, name, n, h, w, mixed=False):
    """n files; 16 distinct pictures, the others shifted copies (the bytes differ, the generator runs 16 times)"""
    from PIL import Image
    d = os.path.join(base, name)
    os.makedirs(d)
    bases = [photo(h, w, 50 + k) for k in range(16)]
    paths = []
    for i in range(n):
        arr = np.roll(bases[i % 16], (3 * (i // 16), 5 * (i // 16)), axis=(0, 1))
        kind = ("jpg", "jpg", "png", "jpg", "bmp", "jpg", "gif", "jpg")[i % 8] if mixed else "jpg"
        p = os.path.join(d, "img%04d.%s" % (i, kind))
        pim = Image.fromarray(arr)
        if kind == "jpg":
            pim.save(p, "JPEG", quality=85, subsampling=2, progressive=bool(mixed and i % 3 == 0))
        elif kind == "gif":
            pim.convert("P").save(p, "GIF")
        else:
            pim.save(p, kind.upper())
        paths.append(p)
    return paths


def route_a(clip, L, paths):
    out = []
    for pos in range(0, len(paths), BATCH):
        imgs = []
        for p in paths[pos:pos + BATCH]:
            im = L.clip_image_u8_make()
            if L.clip_image_load_from_file(os.fsencode(p), im):
                imgs.append(im)
            else:
                L.clip_image_u8_free(im)
        arr = (clip_cpp_amd.ClipImageU8 * len(imgs))(*[im.contents for im in imgs])
        vec = np.empty((len(imgs), clip.vision_config["projection_dim"]), dtype=np.float32)
        assert L.clip_amd_image_batch_encode_u8(clip.ctx, arr, len(imgs), vec.ctypes.data_as(C.POINTER(C.c_float)), True)
        for im in imgs:
            L.clip_image_u8_free(im)
        out.append(vec)
    return np.concatenate(out)


def route_files(clip, paths, threads, device):
    os.environ["CLIP_AMD_JPEG_DEVICE"] = "1" if device else "0"
    out, pos, prepared = [], 0, clip.ImageFileList(paths)
    while pos < len(paths):
        vecs, ok, consumed = clip.encode_image_files(prepared, normalize=True, n_threads=threads, max_images=BATCH, start=pos)
        out.append(vecs)
        pos += consumed
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = clip_cpp_amd.lib()
    model = synth.cached_model(os.environ.get("CLIP_AMD_FIXTURE_CACHE", "/tmp/clip_amd_fixtures"), "b32", "q4_0", text=False, vision=True)
    clip = clip_cpp_amd.Clip(model, verbosity=0, device=0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("files_bench: %d files per JPEG folder, windows of %d, %d interleaved repeats, model b32 q4_0 (synthetic), threads capped at 16" % (a.files, BATCH, a.repeats))
    routes = [("A serial load + encode_u8", None, None)] + [("%s %2d threads" % (n, t), t, dev) for t in (1, 4, 16) for n, dev in (("B host pixel half", False), ("C device pixel half", True))]
    verdict = {}
    with tempfile.TemporaryDirectory() as tmp:
        folders = [("jpeg 640x480", make_folder(tmp, "j640", a.files, 480, 640)), ("jpeg 1600x1200", make_folder(tmp, "j1600", a.files, 1200, 1600)),
                   ("mixed 640x480 (jpeg / progressive jpeg / png / bmp / gif)", make_folder(tmp, "mixed", max(8, a.files // 2), 480, 640, mixed=True))]
        for fname, paths in folders:
            ref = route_a(clip, L, paths[:BATCH])                                   # warm-up (allocations, file cache) + the rows every route must give
            for _, t, dev in routes[1:]:
                got = route_files(clip, paths[:BATCH], t, dev)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "route gives other embeddings"
            times = {r[0]: [] for r in routes}
            for _ in range(a.repeats):
                for rname, t, dev in routes:
                    t0 = time.perf_counter()
                    route_a(clip, L, paths) if t is None else route_files(clip, paths, t, dev)
                    times[rname].append(time.perf_counter() - t0)
            say()
            say("%s: %d files, %.1f MB on disk" % (fname, len(paths), sum(os.path.getsize(p) for p in paths) / 1e6))
            med = {k: statistics.median(v) for k, v in times.items()}
            base = len(paths) / med[routes[0][0]]
            for rname, _, _ in routes:
                v = times[rname]
                say("  %-30s %9.1f img/s  (median of %d: %.3f s, spread %4.1f %%)  x%.2f of A" % (
                    rname, len(paths) / med[rname], len(v), med[rname], 100 * (max(v) - min(v)) / med[rname], len(paths) / med[rname] / base))
            b, c = times["B host pixel half 16 threads"], times["C device pixel half 16 threads"]
            b_spread = (max(b) - min(b)) / statistics.median(b)
            gain = statistics.median(b) / statistics.median(c) - 1.0
            verdict[fname] = (gain, b_spread)
            say("  C over B at 16 threads: %+.1f %%; spread between the B repeats: %.1f %%" % (100 * gain, 100 * b_spread))
        # the kernels alone
        say()
        say("kernels alone (HIP events, median of 20 runs, 64 copies of one file in one launch):")
        for fname, paths in folders[:2]:
            data = open(paths[0], "rb").read()
            ms, nbytes = (C.c_float * 2)(), (C.c_double * 2)()
            rc = L.clip_amd_bench_jpeg_kernels(data, len(data), 64, 20, ms, nbytes)
            assert rc == 0, rc
            for k, kname in enumerate(("jpeg_idct_kernel", "jpeg_rgb_kernel")):
                say("  %-15s %-17s %8.3f ms for %7.1f MB it must move: %7.1f GB/s, %6.0f images/s" % (fname, kname, ms[k], nbytes[k] / 1e6, nbytes[k] / ms[k] / 1e6, 64 / ms[k] * 1e3))
    say()
    jpeg_folders = [k for k in verdict if k.startswith("jpeg")]
    wins = all(verdict[k][0] > verdict[k][1] for k in jpeg_folders)
    say("default: the device pixel half %s B at 16 threads on both JPEG folders by more than the spread between B's repeats -> CLIP_AMD_JPEG_DEVICE defaults to %s"
        % ("exceeds" if wins else "does not exceed", "1 (device)" if wins else "0 (host); =1 opts in"))
    clip.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
