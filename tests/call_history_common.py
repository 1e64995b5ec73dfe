"""Shapes of the call-history tests (tests/test_gpu_call_history.py), shared with the CPU tier that pins the tile codes they rely on
(tests/test_call_history_shapes_cpu.py).

The GPU scenarios compare a context that has served other calls with a fresh one, bit for bit.  They only bite while the GEMM heuristic
(k_gemm.hip pick_tile, read through clip_amd_test_gemm_tile_ex: pure host arithmetic) sends these shapes down the branches named here, so
every code below is asserted on the CPU tier: a retune that makes a scenario vacuous fails there instead of passing silently.

How the shapes were chosen (each confirmed with the tile hook):

  hist_v    S = 68, P = 4 -> T = 290 tokens, h = 1024, ff = 4096, 2 layers.  32 images = 9280 rows: the largest batch the vision graph cache
            takes (B <= 32), ABOVE the 8400 rows up to which a tower this wide is split into two half-batches on two streams
            (forward.cpp vision_forward_launch) — at S = 64 (T = 257, 8224 rows) the call runs as two 4112-row halves that want no resident
            panel at all — and inside 8192 ... 32767 rows, where the out-projection and FFN-down of a block-quantised file run on resident
            panels (mask 2 | 8) and FFN-up of an f16 file runs on the 32 x 32 x 16 kernel unless the device is shared.  128 images = 37120
            rows >= 32768: q/k/v and FFN-up want panels too (bits 1 | 4) and the out-projection does not: the mask must GROW by bits it
            does not hold yet.
  hist_w    S = 72, P = 4 -> T = 325 tokens, h = 2048, ff = 4096, 2 layers, f16: the model of the device_shared flip.  Measured on the
            MI355X, the 32 x 32 x 16 kernel and the kernels that replace it on a shared device return the SAME bits on fp16 weights (hist_v
            f16 at 9280 rows: 0 of 2048 words differ; ViT-B/32 f16 at 12800 rows: 0 of 131072), so a shape that only swaps those kernels cannot
            show by its bits which setting a replayed graph was captured under.  What does change bits is the FORM of the layer chain:
            with LayerNorm folded into the GEMM epilogues the operand is rounded before the normalisation, without it after.  fold_pays
            (forward.cpp) folds unless one of the four GEMMs sits on a panel tile other than ...261.  At 32 images = 10400 rows of this
            tower (unsplit: > 8400; captured: B <= 32) the out-projection and FFN-down are on 192 x 128 in both settings, q/k/v and FFN-up
            on 256261 alone (fold) and on the 8-wave panel tile 160256 when shared (K >= 2048: no fold).  h = 2048 is the narrowest
            tower with that property below 32768 rows and the widest the fold consumer takes (32 statistics units).
  b32 text  h = 512, ff = 2048, 77-token texts.  528 texts = 40656 rows: the smallest count at which q/k/v and FFN-up are both on the
            320 x 256 tile, so panels 1 | 4 (| 8) are built.  206 texts = 15862 rows: the smallest count at which a FRESH context
            wants a panel of its own (FFN-down: 8) AND FFN-up on fp16 weights would run the 32 x 32 x 16 kernel — a context that kept
            the FFN-up panel of the large batch and used it here would run another kernel than the fresh one (fused dequantisation).
            (At 160 texts = 12320 rows nothing is wanted, the table is not even looked at, and no history can show.)
"""
from oracle import fixtures

HIST_V = dict(v=dict(S=68, P=4, h=1024, L=2, nh=16, ff=4096, proj=64), t=dict(h=64, L=2, nh=2, ff=128, proj=64, npos=77))
fixtures.CONFIGS.setdefault("hist_v", HIST_V)       # synthesised through the fixture cache like the built-in configurations

HIST_W = dict(v=dict(S=72, P=4, h=2048, L=2, nh=32, ff=4096, proj=64), t=dict(h=64, L=2, nh=2, ff=128, proj=64, npos=77))
fixtures.CONFIGS.setdefault("hist_w", HIST_W)
HIST_W_T = (HIST_W["v"]["S"] // HIST_W["v"]["P"]) ** 2 + 1          # 325
HIST_W_IMAGES = 32                                                  # 10400 rows

HIST_V_T = (HIST_V["v"]["S"] // HIST_V["v"]["P"]) ** 2 + 1          # 290
HIST_V_SMALL, HIST_V_LARGE = 32, 128                                # images: 9280 and 37120 rows
SPLIT_ROWS_MAX_WIDE = 8400       # forward.cpp vision_forward_launch: towers of h >= 1024 run 2000 ... 8400 rows as two halves
GRAPH_MAX_IMAGES = 32            # forward.cpp vision_forward_device: larger batches are never captured

B32_TEXT = fixtures.CONFIGS["b32"]["t"]
TEXT_LARGE, TEXT_MID = 528, 206                                     # texts of 77 tokens: 40656 and 15862 rows


def linears(h, ff):
    """(N, K) of a layer's four GEMMs in table order: 0 q/k/v, 1 out-projection, 2 FFN-up, 3 FFN-down."""
    return [(3 * h, h), (h, h), (ff, h), (h, ff)]


def tile_uses_panel(tile):
    """kernels.h gemm_tile_uses_panel."""
    bn = tile % 1000
    return (tile % 1000000) // 1000 != 65 and (bn == 256 or 258 <= bn <= 261)


def fold_pays(L, rows, h, ff, shared):
    """forward.cpp fold_pays for an f16 file: no GEMM of the layer on a panel tile other than ...261."""
    tiles = [L.clip_amd_test_gemm_tile_ex(rows, n, k, 0, int(shared)) for n, k in linears(h, ff)]
    return not any(tile_uses_panel(t) and t % 1000 != 261 for t in tiles)


def wanted_mask(L, rows, h, ff, shared):
    """forward.cpp wants_resident_panel for a block-quantised file, as a mask over the four weights."""
    tile = lambda i, sh: L.clip_amd_test_gemm_tile_ex(rows, linears(h, ff)[i][0], linears(h, ff)[i][1], 0, int(sh))
    m = 0
    for i in (0, 2):
        if rows >= 32768 and tile(i, shared) % 1000 == 261:
            m |= 1 << i
    if 4096 <= rows < 32768 and tile_uses_panel(tile(1, False)):
        m |= 2
    if rows >= 4096 and tile_uses_panel(tile(3, False)):
        m |= 8
    return m


def ctx_state(L, clip, which):
    """clip_amd_test_ctx_state as a dict: mask, entries, vgraphs, tgraphs, ws_bytes, panels (list of ints, 0 = none)."""
    import ctypes as C
    head = (C.c_int64 * 5)()
    n = L.clip_amd_test_ctx_state(clip.ctx, which, head, None, 0)
    assert n >= 0, n
    panels = (C.c_uint64 * max(n, 1))()
    assert L.clip_amd_test_ctx_state(clip.ctx, which, head, panels, n) == n
    return dict(mask=int(head[0]), entries=int(head[1]), vgraphs=int(head[2]), tgraphs=int(head[3]), ws_bytes=int(head[4]), panels=[int(panels[k]) for k in range(n)])
