"""CPU tier of the call-history tests: the tile codes that tests/test_gpu_call_history.py relies on (tests/call_history_common.py says why
each shape was chosen), read through clip_amd_test_gemm_tile_ex, and the argument checks of the read-only state hook
clip_amd_test_ctx_state.  No device is needed for either."""
import ctypes as C

import call_history_common as ch
from oracle import fixtures


def _tiles(L, rows, h, ff, quantised, shared):
    return [L.clip_amd_test_gemm_tile_ex(rows, n, k, int(quantised), int(shared)) for n, k in ch.linears(h, ff)]


def test_hist_v_small_batch_is_captured_unsplit_on_the_panel_and_gemm32_branches(clip_lib):
    L = clip_lib.lib()
    v = ch.HIST_V["v"]
    h, ff = v["h"], v["ff"]
    rows = ch.HIST_V_SMALL * ch.HIST_V_T
    assert ch.HIST_V_T == 290 and rows == 9280
    assert ch.HIST_V_SMALL <= ch.GRAPH_MAX_IMAGES                      # the graph cache takes the batch ...
    assert h >= 1024 and ch.SPLIT_ROWS_MAX_WIDE < rows < 32768         # ... and it is not split into two half-batches
    qkv, out, up, down = _tiles(L, rows, h, ff, False, False)          # fp16 weights (an f16 file, or a panel), device not shared
    assert out == 160256
    assert ch.tile_uses_panel(down) and down % 1000 != 261
    assert up == 320261
    assert qkv % 1000 == 261
    assert ch.wanted_mask(L, rows, h, ff, False) == 10                 # a q4_0 file at B = 32: out-projection and FFN-down panels
    assert ch.wanted_mask(L, rows, h, ff, True) == 10
    # shared device: FFN-up (and q/k/v) leave the 32 x 32 x 16 kernel — the two settings run different kernels on an f16 file
    assert all(t % 1000 != 261 for t in _tiles(L, rows, h, ff, False, True))
    # block-quantised weights without a panel: the fused-dequant kernels, never a panel tile at this row count
    assert not any(ch.tile_uses_panel(t) for t in _tiles(L, rows, h, ff, True, False))


def test_hist_v_large_batch_wants_bits_the_small_batch_did_not_build(clip_lib):
    L = clip_lib.lib()
    v = ch.HIST_V["v"]
    h, ff = v["h"], v["ff"]
    rows = ch.HIST_V_LARGE * ch.HIST_V_T
    assert rows == 37120 and rows >= 32768
    qkv, out, up, down = _tiles(L, rows, h, ff, False, False)
    assert qkv % 1000 == 261 and up % 1000 == 261 and ch.tile_uses_panel(down)
    small = ch.wanted_mask(L, ch.HIST_V_SMALL * ch.HIST_V_T, h, ff, False)
    large = ch.wanted_mask(L, rows, h, ff, False)
    assert large == 13                                                 # q/k/v, FFN-up, FFN-down; the out-projection bit is not wanted (rows >= 32768)
    assert large & ~small == 5                                         # the growth condition: wanted bits that are not held
    # on a shared device the same batch wants FFN-down only: the call that sizes the workspace first without touching bits 1 | 4
    assert ch.wanted_mask(L, rows, h, ff, True) == 8
    assert not any(t % 1000 == 261 for t in _tiles(L, rows, h, ff, False, True))


def test_hist_w_folds_the_layernorms_alone_and_not_on_a_shared_device(clip_lib):
    L = clip_lib.lib()
    v = ch.HIST_W["v"]
    h, ff = v["h"], v["ff"]
    rows = ch.HIST_W_IMAGES * ch.HIST_W_T
    assert ch.HIST_W_T == 325 and rows == 10400
    assert ch.HIST_W_IMAGES <= ch.GRAPH_MAX_IMAGES and ch.SPLIT_ROWS_MAX_WIDE < rows < 32768 and h <= 2048
    alone, shared = _tiles(L, rows, h, ff, False, False), _tiles(L, rows, h, ff, False, True)
    assert alone == [256261, 192128, 256261, 192128]
    assert shared == [160256, 192128, 160256, 192128]
    # the form of the layer chain differs between the two settings: that is what separates their bits
    assert ch.fold_pays(L, rows, h, ff, False) and not ch.fold_pays(L, rows, h, ff, True)
    # hist_v, for comparison, keeps the un-folded form in both (its out-projection is on the 8-wave panel tile): same bits either way
    hv = ch.HIST_V["v"]
    assert not ch.fold_pays(L, ch.HIST_V_SMALL * ch.HIST_V_T, hv["h"], hv["ff"], False) and not ch.fold_pays(L, ch.HIST_V_SMALL * ch.HIST_V_T, hv["h"], hv["ff"], True)


def test_b32_text_mid_batch_would_use_a_left_over_ffn_up_panel(clip_lib):
    L = clip_lib.lib()
    h, ff, npos = ch.B32_TEXT["h"], ch.B32_TEXT["ff"], ch.B32_TEXT["npos"]
    assert (h, ff, npos) == (512, 2048, 77)
    big, mid = ch.TEXT_LARGE * npos, ch.TEXT_MID * npos
    assert big == 40656 and mid == 15862
    qkv, out, up, down = _tiles(L, big, h, ff, False, False)
    assert qkv == 320261 and up == 320261
    assert ch.wanted_mask(L, big, h, ff, False) == 13                  # panel bits 1 and 4 (and FFN-down) are built by the large batch
    assert ch.wanted_mask(L, big, h, ff, True) == 8
    # the mid batch: a fresh context wants panels of its own (so the table IS consulted), but not q/k/v or FFN-up ...
    assert ch.wanted_mask(L, mid, h, ff, False) == 10 and ch.wanted_mask(L, mid, h, ff, True) == 10
    # ... although FFN-up on fp16 weights would take the 32 x 32 x 16 kernel here: a left-over panel, if used, changes the kernel
    assert _tiles(L, mid, h, ff, False, False)[2] % 1000 == 261
    # what a fresh context runs for q/k/v and FFN-up: the fused-dequant tiles
    q_qkv, _, q_up, _ = _tiles(L, mid, h, ff, True, False)
    assert q_qkv % 1000 == 128 and q_up % 1000 == 128
    # on a shared device no left-over panel would be used either way
    assert all(t % 1000 != 261 for t in _tiles(L, mid, h, ff, False, True))
    # TEXT_MID is the smallest such count, TEXT_LARGE the smallest with both wide GEMMs on the 320 x 256 tile
    for n in (ch.TEXT_MID - 1,):
        assert not (ch.wanted_mask(L, n * npos, h, ff, False) and _tiles(L, n * npos, h, ff, False, False)[2] % 1000 == 261)
    assert ch.wanted_mask(L, (ch.TEXT_LARGE - 1) * npos, h, ff, False) & 5 != 5


def test_ctx_state_hook_checks_its_arguments_and_reads_a_context_without_a_device(clip_lib, host_only_env, fixture_cache):
    L = clip_lib.lib()
    head = (C.c_int64 * 5)(*([-7] * 5))
    panels = (C.c_uint64 * 8)(*([77] * 8))
    clip = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "q4_0"), verbosity=0)
    try:
        for args in ((None, 0, head, panels, 8),                       # no context
                     (clip.ctx, 2, head, panels, 8), (clip.ctx, -1, head, panels, 8),      # no such tower
                     (clip.ctx, 0, None, panels, 8),                   # nowhere to write the head
                     (clip.ctx, 0, head, panels, -1), (clip.ctx, 0, head, None, 8)):
            assert L.clip_amd_test_ctx_state(*args) == -3, args[1:]
            assert list(head) == [-7] * 5 and list(panels) == [77] * 8           # nothing written
        layers = fixtures.CONFIGS["tiny"]["v"]["L"]
        want_entries = 4 * layers if clip.device >= 0 else 0           # a host-only context has no tables
        for which in (0, 1):
            assert L.clip_amd_test_ctx_state(clip.ctx, which, head, None, 0) == want_entries
            assert list(head) == [0, want_entries, 0, 0, 0]            # nothing built, captured or allocated before the first encode
        st = ch.ctx_state(L, clip, 0)
        assert st["panels"] == [0] * want_entries
        # a short panels array receives the leading entries only
        assert L.clip_amd_test_ctx_state(clip.ctx, 0, head, panels, 3) == want_entries
        assert list(panels)[3:] == [77] * 5
    finally:
        clip.close()
