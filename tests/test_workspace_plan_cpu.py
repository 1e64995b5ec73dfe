"""CPU tier: the layout of a tower pass's activation buffers (forward.cpp carve_tower), read through clip_amd_test_tower_plan — host arithmetic, no
device.  With CLIP_AMD_WS_ALIAS=1 (the default) qkv, att, mid and the im2col matrix share one region; what is checked here is that no two
buffers that are LIVE TOGETHER overlap, whatever the shape, and that the switch at 0 gives the layout of separate buffers.

The lifetime table (STEP_IO) is written out from forward.cpp in launch order: what each step reads and what it writes, in the form with the
longest lifetimes (LayerNorm folded: xn, stats and mu are written by the step BEFORE the GEMM that reads them; the un-folded form writes xn
inside the `qkv` / `up` steps, which the table lists too).  A buffer is live from a step that writes it to the last step that reads that
value; two buffers are live together when both are live in one step."""
import ctypes as C
import itertools

import pytest

NAMES = ["stats", "mu", "x", "xn", "qkv", "att", "mid", "col", "pooled", "emb", "xp", "ap", "xnp", "midp", "region"]

# step: (reads, writes)
STEP_IO = {
    # vision_stage_patch, once per copy piece, every piece before `entry`: im2col, then the patch GEMM (scatters into x)
    "patch": (("col",), ("col", "x")),
    # launch_layernorm_prep (class-token rows + pre-LN, in place) / launch_text_embed
    "entry": (("x",), ("x", "xn", "stats", "mu")),
    # run_layers: norm_linear q/k/v (un-folded: a LayerNorm launch x -> xn first), attention, resid_linear, norm_linear FFN-up, resid_linear
    "qkv": (("x", "xn", "stats", "mu"), ("xn", "qkv", "mu")),
    "attn": (("qkv",), ("att",)),
    "out": (("att", "x", "mu"), ("x", "xn", "stats")),
    "up": (("x", "xn", "stats", "mu"), ("xn", "mid", "mu")),
    "down": (("mid", "x", "mu"), ("x", "xn", "stats")),
    # pooled_tail: gather, then out-projection / LayerNorm + FFN-up / FFN-down on the pooled rows
    "gather": (("x", "att"), ("xp", "ap")),
    "tail_out": (("ap", "xp"), ("xp",)),
    "tail_up": (("xp",), ("xnp", "midp")),
    "tail_down": (("midp", "xp"), ("xp",)),
    # run_tower: post-LN of the pooled rows (pruned: xp; else gathered from x), projection, L2 norm
    "post_ln": (("xp", "x"), ("pooled",)),
    "proj": (("pooled",), ("emb",)),
    "l2": (("emb",), ()),
}
LAYER = ["qkv", "attn", "out", "up", "down"]
PASSES = {
    # two full layers and the pruned last one (rows > sequences, beyond the small-M path)
    "pruned": ["patch", "patch", "entry"] + LAYER + LAYER + ["qkv", "attn", "gather", "tail_out", "tail_up", "tail_down", "post_ln", "proj", "l2"],
    # every layer on every row (small-M path, one row per sequence, CLIP_AMD_PRUNE_LAST=0)
    "full": ["patch", "patch", "entry"] + LAYER + LAYER + LAYER + ["post_ln", "proj", "l2"],
}


def live_steps(order, name):
    """indices of the steps of `order` in which `name` holds a value that a later (or the same) step reads"""
    live, start = set(), None
    for i, step in enumerate(order):
        reads, writes = STEP_IO[step]
        if name in reads and start is not None:
            live.update(range(start, i + 1))
        if name in writes:
            live.add(i)                                      # being written: nothing else may lie there in this step
            start = i
    return live


def live_together(a, b):
    return any(live_steps(order, a) & live_steps(order, b) for order in PASSES.values())


def test_the_lifetime_table_says_what_the_overlay_relies_on():
    assert live_together("qkv", "att")                       # attention reads one and writes the other
    for a, b in (("mid", "qkv"), ("mid", "att"), ("col", "qkv"), ("col", "att"), ("col", "mid")):
        assert not live_together(a, b), (a, b)
    for keep in ("x", "xn", "stats", "mu"):                  # the residual stream and the fold's operand and statistics span the whole layer
        for other in ("qkv", "att", "mid"):
            assert live_together(keep, other), (keep, other)
    assert live_together("x", "col")                         # the patch GEMM reads col and writes x
    for keep in ("xp", "ap"):                                # pooled_tail writes them while it reads att
        assert live_together(keep, "att"), keep
    every = set(n for r, w in STEP_IO.values() for n in r + w)
    assert every == set(NAMES) - {"region"}


def plan(L, rows, nseq, h, ff, proj, f32, col_halfs, alias):
    off, size = (C.c_int64 * len(NAMES))(), (C.c_int64 * len(NAMES))()
    total = C.c_int64(-1)
    assert L.clip_amd_test_tower_plan(rows, nseq, h, ff, proj, int(f32), col_halfs, int(alias), off, size, len(NAMES), C.byref(total)) == len(NAMES)
    return {n: (int(off[i]), int(size[i])) for i, n in enumerate(NAMES)}, int(total.value)


def align256(v):
    return (v + 255) // 256 * 256


def region_bytes(rows, h, ff, f32, col_halfs):
    """The formula of the overlay: mid, or qkv with att behind it, or col — whichever is largest."""
    ab = 4 if f32 else 2
    return max(ab * rows * ff, align256(ab * rows * 3 * h) + ab * rows * h, 2 * col_halfs)


def separate_layout(rows, nseq, h, ff, proj, f32, col_halfs):
    """Separate buffers in carve order, each start rounded up to 256 bytes, col (vision) behind the pooled buffers."""
    ab = 4 if f32 else 2
    stride = (rows + 63) // 64 * 64
    order = [("stats", (h // 16) * stride * 8), ("mu", 2 * stride * 4), ("x", rows * h * 4), ("xn", ab * rows * h), ("qkv", ab * rows * 3 * h),
             ("att", ab * rows * h), ("mid", ab * rows * ff), ("pooled", ab * nseq * h), ("emb", nseq * proj * 4), ("xp", nseq * h * 4),
             ("ap", ab * nseq * h), ("xnp", ab * nseq * h), ("midp", ab * nseq * ff)]
    if col_halfs:
        order.append(("col", 2 * col_halfs))
    at, out = 0, {}
    for name, size in order:
        at = align256(at)
        out[name] = (at, size)
        at += size
    return out, at


SHAPES = [(768, 3072), (512, 2048), (64, 128), (64, 512)]           # ViT-B/32 vision and text; ff < 4 h; ff > 4 h
ROWS = [1, 50, 85, 12800]


def col_sizes(rows, h, ff, f32):
    mid = (4 if f32 else 2) * rows * ff // 2                  # mid's size in fp16 elements
    return [0, max(1, mid // 3), 2 * mid + 7]                 # none (text), smaller than mid, larger than mid


CASES = [(h, ff, rows, f32, k) for (h, ff), rows, f32, k in itertools.product(SHAPES, ROWS, (False, True), range(3))]


@pytest.mark.parametrize("h,ff,rows,f32,which_col", CASES)
def test_buffers_live_together_are_disjoint_and_aligned(clip_lib, monkeypatch, h, ff, rows, f32, which_col):
    monkeypatch.delenv("CLIP_AMD_GUARD", raising=False)
    L = clip_lib.lib()
    nseq, proj = max(1, rows // 50), 32
    col_halfs = col_sizes(rows, h, ff, f32)[which_col]
    for alias in (1, 0):
        p, total = plan(L, rows, nseq, h, ff, proj, f32, col_halfs, alias)
        bufs = [n for n in NAMES if n != "region" and p[n][1] > 0]
        assert ("col" in bufs) == (col_halfs > 0)
        for n in bufs:
            off, size = p[n]
            assert off % 256 == 0 and off >= 0 and off + size <= total, (alias, n, p[n], total)
        for a, b in itertools.combinations(bufs, 2):
            if alias and not live_together(a, b):
                continue
            (ao, asz), (bo, bsz) = p[a], p[b]
            assert ao + asz <= bo or bo + bsz <= ao, "alias=%d: %s %s and %s %s overlap" % (alias, a, p[a], b, p[b])
        if alias:
            ro, rs = p["region"]
            assert rs == region_bytes(rows, h, ff, f32, col_halfs) and ro % 256 == 0
            for n in ("qkv", "att", "mid", "col"):
                if p[n][1]:
                    assert ro <= p[n][0] and p[n][0] + p[n][1] <= ro + rs, (n, p[n], p["region"])
            assert p["qkv"][0] == p["mid"][0] == ro and (not col_halfs or p["col"][0] == ro)
            assert p["att"][0] == ro + align256(p["qkv"][1])
            for n in bufs:                                   # everything else lies outside the region
                if n not in ("qkv", "att", "mid", "col"):
                    assert p[n][0] + p[n][1] <= ro or p[n][0] >= ro + rs, (n, p[n], p["region"])
        else:
            want, want_total = separate_layout(rows, nseq, h, ff, proj, f32, col_halfs)
            assert p["region"][1] == 0
            assert {n: p[n] for n in bufs} == want and total == want_total


def test_both_benchmark_towers_fit_the_infinity_cache_with_the_overlay(clip_lib, monkeypatch):
    """bench.py: 256 images (50 tokens each) and 256 texts of ViT-B/32, fp16 activations.  The bytes a layer cycles through — x, xn, the statistics
    and the shared region of both towers — stay under the 256 MiB of the Infinity Cache with the overlay and not without it; col is part of the sum
    only where it makes the region larger (it does not: 77 MB against mid's 79 MB)."""
    monkeypatch.delenv("CLIP_AMD_GUARD", raising=False)
    L = clip_lib.lib()
    n = 256
    v_rows, t_rows_max = n * 50, n * 77
    col = n * 49 * 3072                                      # [images x 49 patches][3 x 32 x 32]
    cyc = ("stats", "mu", "x", "xn")

    def cycled(rows, nseq, h, ff, col_halfs, alias):
        p, _ = plan(L, rows, nseq, h, ff, 512, False, col_halfs, alias)
        if alias:
            return sum(p[k][1] for k in cyc) + p["region"][1]
        return sum(p[k][1] for k in cyc + ("qkv", "att", "mid", "col"))

    def formula(rows, h, ff, col_halfs):
        stride = (rows + 63) // 64 * 64
        return (h // 16) * stride * 8 + 2 * stride * 4 + rows * h * 4 + rows * h * 2 + max(rows * ff * 2, align256(rows * 3 * h * 2) + rows * h * 2, col_halfs * 2)

    for t_rows in (10290, t_rows_max // 2):                  # the benchmark's ragged texts (about 40 tokens each), and half-full contexts
        with_overlay = cycled(v_rows, n, 768, 3072, col, 1) + cycled(t_rows, n, 512, 2048, 0, 1)
        assert with_overlay == formula(v_rows, 768, 3072, col) + formula(t_rows, 512, 2048, 0)
        assert with_overlay < 256 << 20, with_overlay
        without = cycled(v_rows, n, 768, 3072, col, 0) + cycled(t_rows, n, 512, 2048, 0, 0)
        assert without > 256 << 20, without


def test_the_hook_refuses_shapes_no_tower_has(clip_lib):
    L = clip_lib.lib()
    off, size = (C.c_int64 * 15)(*([-7] * 15)), (C.c_int64 * 15)(*([-7] * 15))
    for args in ((0, 1, 64, 128, 32, 0, 0, 1), (10, 0, 64, 128, 32, 0, 0, 1), (10, 11, 64, 128, 32, 0, 0, 1), (10, 1, 8, 128, 32, 0, 0, 1),
                 (10, 1, 72, 128, 32, 0, 0, 1), (10, 1, 64, 0, 32, 0, 0, 1), (10, 1, 64, 128, 0, 0, 0, 1), (10, 1, 64, 128, 32, 0, -1, 1)):
        assert L.clip_amd_test_tower_plan(*args, off, size, 15, None) == -3, args
    assert L.clip_amd_test_tower_plan(10, 1, 64, 128, 32, 0, 0, 1, None, size, 15, None) == -3
    assert list(off) == [-7] * 15 and list(size) == [-7] * 15
    assert "clip_amd_test_tower_plan" in clip_lib.AMD_SYMBOLS
