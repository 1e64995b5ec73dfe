"""Attention kernels past the whole-row limit (k_attn_long.hip) and a long-sequence tower end to end.

    python scripts/attn_bench.py                      kernel table + ViT-H/14-378 f16 tower at B = 1, 32, 128
    python scripts/attn_bench.py --kernels-only       kernel table only
    python scripts/attn_bench.py --tower-only --batches 128 --reps 2     (the form to run under rocprofv3 --kernel-trace --stats)
    python scripts/attn_bench.py --stats FILE_kernel_stats.csv           attention's share of the kernel time in a rocprofv3 stats file

Kernel times: clip_amd_bench_attention (HIP events, seeded random q / k / v).  FLOPs: 4 T^2 d_head per (sequence, head), the non-causal
count of the two contractions; share of the fp16 dense MFMA peak (~2.5 PFLOP/s, MI355X spec) = FLOPs / peak / time.  At T = 577, d_head 64
the whole-row kernel (k_attn.hip, what the layers run there) and the streaming kernel are timed alternately in one process.
The tower: a seeded synthetic ViT-H/14 at 378 px (T = 730, d_head 80, 32 layers, f16 weights; clip_cpp_amd.synth) written to a temporary
file, images/s through Clip.encode_images (host f32 images in, host embeddings out)."""
import argparse
import csv
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F16 = 2.5e15       # FLOP/s, dense fp16 MFMA (MI355X spec)
H14_378 = dict(v=dict(S=378, P=14, h=1280, L=32, nh=16, ff=5120, proj=1024), t=dict(h=1024, L=1, nh=16, ff=4096, proj=1024, npos=77))


def attn_flops(nseq, T, h, nh):
    return 4.0 * nseq * nh * T * T * (h // nh)


def kernel_table(L, iters, rounds):
    def bench(nseq, T, h, nh, kernel):
        us = L.clip_amd_bench_attention(nseq, T, h, nh, 0, kernel, iters)
        if us < 0:
            raise RuntimeError("clip_amd_bench_attention(%d, %d, %d, %d, kernel %d) = %g" % (nseq, T, h, nh, kernel, us))
        return us

    def line(tag, nseq, T, h, nh, kernel, us):
        fl = attn_flops(nseq, T, h, nh)
        print("%-34s nseq %3d  T %5d  d_head %3d  %-9s %9.1f us  %6.1f TFLOP/s  %5.1f %% of fp16 peak"
              % (tag, nseq, T, h // nh, "streaming" if kernel == 2 else "whole-row", us, fl / us * 1e-6, 100.0 * fl / PEAK_F16 / (us * 1e-6)), flush=True)

    # T = 577, d_head 64 (ViT-L/14 at 336 px), 32 sequences x 16 heads: both kernels, alternated
    shape = (32, 577, 1024, 16)
    for k in (1, 2):
        bench(*shape, k)                                   # warm-up
    t = {1: [], 2: []}
    for _ in range(rounds):
        for k in (1, 2):
            t[k].append(bench(*shape, k))
    for k in (1, 2):
        print("  %s rounds: %s" % ("whole-row" if k == 1 else "streaming", " ".join("%.1f" % v for v in t[k])))
        line("l14_336 (alternated, median)", *shape, k, statistics.median(t[k]))
    ratio = statistics.median(t[2]) / statistics.median(t[1])
    print("streaming / whole-row at T = 577, d_head 64: %.3f (bar: <= 1.3)" % ratio, flush=True)
    for tag, s in (("h14_378", (32, 730, 1280, 16)), ("l14_448", (32, 1025, 1024, 16)), ("b16_512", (32, 1025, 768, 12)),
                   ("h14_378 one image", (1, 730, 1280, 16)), ("bigG_336", (32, 577, 1664, 16))):
        bench(*s, 2)
        line(tag, *s, 2, statistics.median(bench(*s, 2) for _ in range(rounds)))
    return ratio


def tower(clip_cpp_amd, batches, reps):
    import numpy as np
    from clip_cpp_amd import synth
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "h14_378_f16.gguf")
        t0 = time.time()
        synth.write_model(path, H14_378, "f16", text=False, vision=True, seed=1234)
        print("synthetic ViT-H/14-378 f16 vision tower written in %.1f s (%.2f GB)" % (time.time() - t0, os.path.getsize(path) / 1e9), flush=True)
        clip = clip_cpp_amd.Clip(path, device=0)
        S = clip.vision_config["image_size"]
        T = (S // clip.vision_config["patch_size"]) ** 2 + 1
        v = H14_378["v"]
        per_img_attn = attn_flops(1, T, v["h"], v["nh"]) * v["L"]
        per_img_gemm = 2.0 * T * (4 * v["h"] * v["h"] + 2 * v["h"] * v["ff"]) * v["L"]
        print("T = %d: per image %.1f GFLOP of attention, %.1f GFLOP of layer GEMMs (attention %.1f %% of the FLOPs)"
              % (T, per_img_attn * 1e-9, per_img_gemm * 1e-9, 100.0 * per_img_attn / (per_img_attn + per_img_gemm)), flush=True)
        rng = np.random.default_rng(3)
        for B in batches:
            imgs = rng.standard_normal((B, S, S, 3), dtype=np.float32)
            emb = clip.encode_images(imgs)                  # warm-up (workspace, graphs)
            assert np.all(np.isfinite(emb))
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                clip.encode_images(imgs)
                ts.append(time.perf_counter() - t0)
            print("tower B = %3d: %8.2f img/s  (median of %d calls, %.1f ms per call; %.0f TFLOP/s of layer work)"
                  % (B, B / statistics.median(ts), reps, 1e3 * statistics.median(ts), B * (per_img_attn + per_img_gemm) / statistics.median(ts) * 1e-12),
                  flush=True)
        clip.close()


def stats_share(path):
    tot = attn = 0.0
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            tot += ns
            if "attn" in r["Name"]:
                attn += ns
            rows.append((ns, r["Name"], r["Calls"]))
    rows.sort(reverse=True)
    for ns, name, calls in rows[:12]:
        print("%6.2f %%  %10.3f ms  %6s calls  %s" % (100.0 * ns / tot, ns * 1e-6, calls, name[:110]))
    print("attention kernels: %.2f %% of %.1f ms kernel time (bar: <= 20 %%)" % (100.0 * attn / tot, tot * 1e-6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--tower-only", action="store_true")
    ap.add_argument("--batches", default="1,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        stats_share(a.stats)
        return
    try:
        import torch  # noqa: F401  (HIP runtime order, see tests/conftest.py)
    except Exception:
        pass
    import clip_cpp_amd
    L = clip_cpp_amd.lib()
    if clip_cpp_amd.device_count() < 1:
        sys.exit("attn_bench: no HIP device (every number here is a GPU measurement)")
    if not a.tower_only:
        kernel_table(L, a.iters, a.rounds)
    if not a.kernels_only:
        tower(clip_cpp_amd, [int(b) for b in a.batches.split(",")], a.reps)


if __name__ == "__main__":
    main()
