"""GPU tier: the bits an encode returns do not depend on what the context did before (include/clip_amd.h, at clip_amd_set_device_shared:
"what the bits of an encode depend on").  Every value assertion is bit equality between a FRESH context and a context WITH A HISTORY — same
file, same inputs, same settings; no tolerance appears anywhere.  forward.cpp keeps captured graphs, the resident-panel table, the per-layer
panel scratch, a growing workspace, the small-M statistics and sibling contexts between calls; the shapes that steer each scenario down
its branch are in tests/call_history_common.py and pinned on the CPU tier (tests/test_call_history_shapes_cpu.py).

No test here reads memory that may have been freed: where the code before the fix would have (a replay of a graph whose panels were
rebuilt), the state hook clip_amd_test_ctx_state is read and asserted on BEFORE the replay."""
import io

import numpy as np
import pytest

import call_history_common as ch
from oracle import fixtures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class Images:
    """Seeded preprocessed images on the device with an output buffer of their own: the same two pointers at every call."""

    def __init__(self, torch, B, S, proj, seed):
        self.B = B
        self.x = torch.from_numpy(fixtures.synthetic_images(B, S, seed=seed)).cuda()
        self.out = torch.empty((B, proj), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def run(self, clip, n=None):
        """encode the first n images (default: all) into the output buffer; returns the host copy"""
        n = self.B if n is None else n
        self.out.fill_(float("nan"))
        _sync_torch(self.out)
        clip.encode_images_device(self.x.data_ptr(), n, self.out.data_ptr(), True)
        clip.synchronize()
        return self.out[:n].cpu().numpy()


class Texts:
    """Token lists on the device, one output buffer."""

    def __init__(self, torch, token_lists, proj):
        self.n = len(token_lists)
        self.ids = torch.from_numpy(np.concatenate(token_lists).astype(np.int32)).cuda()
        self.offs = np.concatenate([[0], np.cumsum([len(t) for t in token_lists])]).astype(np.int32)
        self.out = torch.empty((self.n, proj), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def run(self, clip, n=None):
        n = self.n if n is None else n
        self.out.fill_(float("nan"))
        _sync_torch(self.out)
        clip.encode_texts_device(self.ids.data_ptr(), self.offs[:n + 1], self.out.data_ptr(), True)
        clip.synchronize()
        return self.out[:n].cpu().numpy()


def _sync_torch(t):
    import torch
    torch.cuda.synchronize(t.device)          # the fill ran on torch's stream, the encode runs on the context's


def _full_length_texts(n, npos, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[49406], rng.integers(0, fixtures.N_VOCAB - 2, size=npos - 2), [49407]]).astype(np.int32) for _ in range(n)]


def _ragged_texts(n, npos, seed):
    """lengths 1 ... npos: a bare BOS, BOS + EOS, the longest legal text, the rest seeded"""
    rng = np.random.default_rng(seed)
    lens = [1, 2, npos, 9, 9, npos - 1][:n] + [int(v) for v in rng.integers(2, npos + 1, size=max(0, n - 6))]
    out = []
    for ln in lens:
        if ln == 1:
            out.append(np.array([49406], np.int32))
        else:
            out.append(np.concatenate([[49406], rng.integers(0, fixtures.N_VOCAB - 2, size=ln - 2), [49407]]).astype(np.int32))
    return out


def _bits_differ(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# ---- defect 2: kernel choice of a mid batch after a large batch ------------------------------------------------------------------------

@pytest.mark.parametrize("shared", [False, True], ids=["alone", "device-shared"])
@pytest.mark.parametrize("ftype", ["q4_0", "q8_0"])
def test_mid_batch_after_large_batch_is_the_fresh_result(gpu, torch, fixture_cache, ftype, shared):
    """The text tower of ViT-B/32 (h = 512), block-quantised.  528 full-length texts (40656 rows) build resident q/k/v and FFN-up panels for
    the 32 x 32 x 16 kernel; 206 texts (15862 rows) afterwards want FFN-down and out-projection panels only and must run q/k/v and FFN-up on the
    fused-dequant kernels, as on a fresh context — not on the panels the large batch left (another kernel, other bits)."""
    L = gpu.lib()
    t = ch.B32_TEXT
    p = fixtures.cached_model(fixture_cache, "b32", ftype)
    texts = Texts(torch, _full_length_texts(ch.TEXT_LARGE, t["npos"], seed=31), t["proj"])
    fresh, hist = gpu.Clip(p, device=0), gpu.Clip(p, device=0)
    try:
        for c in (fresh, hist):
            c.set_device_shared(shared)
        want = texts.run(fresh, ch.TEXT_MID)
        assert np.all(np.isfinite(want))
        mid_mask = ch.wanted_mask(L, ch.TEXT_MID * t["npos"], t["h"], t["ff"], shared)
        big_mask = ch.wanted_mask(L, ch.TEXT_LARGE * t["npos"], t["h"], t["ff"], shared)
        assert ch.ctx_state(L, fresh, 1)["mask"] == mid_mask != 0           # the mid batch consults the table on its own account
        texts.run(hist, ch.TEXT_LARGE)
        st = ch.ctx_state(L, hist, 1)
        assert st["mask"] == big_mask and (shared or big_mask & 5 == 5)     # alone: the large batch has left q/k/v and FFN-up panels
        got = texts.run(hist, ch.TEXT_MID)
        assert ch.ctx_state(L, hist, 1)["mask"] == big_mask | mid_mask
        assert np.array_equal(got, want), "%d of %d words differ after the large batch" % (_bits_differ(got, want), want.size)
        # ... and by the same kernels (the 32 x 32 x 16 kernel on a left-over panel returns the bits of the fused kernels on this hardware, so the
        # bits alone do not tell): the profile of the mid batch lists the same launches on both contexts
        def launches(c):
            c.profile(True)
            texts.run(c, ch.TEXT_MID)
            rep = c.profile_report(reset=True)
            c.profile(False)
            return sorted((k, r["launches"]) for k, r in rep.items())
        assert launches(hist) == launches(fresh)
    finally:
        fresh.close()
        hist.close()


# ---- defect 1: a captured small-batch graph and a later batch that grows the panel mask -------------------------------------------------

def test_small_batch_graph_survives_a_mask_growing_batch(gpu, torch, fixture_cache):
    """hist_v, q4_0.  B = 32 (9280 rows) is captured with the out-projection and FFN-down panels (mask 10) in its kernel nodes; B = 128 (37120 rows)
    then wants q/k/v and FFN-up panels too.  The panels the graph points at must stay where they are.

    Step 0 is what makes the scenario reach the table at all: a batch that needs a LARGER WORKSPACE drops every captured graph on its way
    (ensure_workspace), so the workspace is sized first by the same 128 images on a "shared" device, where they want the FFN-down panel only.
    The state is asserted before the replay of step 5: with entries that moved under a live graph the test stops there."""
    L = gpu.lib()
    v = ch.HIST_V["v"]
    p = fixtures.cached_model(fixture_cache, "hist_v", "q4_0")
    big = Images(torch, ch.HIST_V_LARGE, v["S"], v["proj"], seed=41)
    small = Images(torch, ch.HIST_V_SMALL, v["S"], v["proj"], seed=42)
    mask_small = ch.wanted_mask(L, ch.HIST_V_SMALL * ch.HIST_V_T, v["h"], v["ff"], False)
    mask_large = ch.wanted_mask(L, ch.HIST_V_LARGE * ch.HIST_V_T, v["h"], v["ff"], False)
    assert (mask_small, mask_large) == (10, 13)
    fresh, hist = gpu.Clip(p, device=0), gpu.Clip(p, device=0)
    try:
        want = small.run(fresh)
        assert np.all(np.isfinite(want))
        # 0. the workspace of the large batch, without its q/k/v and FFN-up panels
        hist.set_device_shared(True)
        big.run(hist)
        hist.set_device_shared(False)
        s0 = ch.ctx_state(L, hist, 0)
        assert s0["mask"] == 8 and s0["vgraphs"] == 0
        # 1. first sighting, capture, replay
        small.run(hist)
        small.run(hist)
        kept = small.run(hist)
        # 2.
        s2 = ch.ctx_state(L, hist, 0)
        assert s2["vgraphs"] >= 1 and s2["mask"] == 10 and s2["entries"] == 4 * v["L"], s2
        assert s2["ws_bytes"] == s0["ws_bytes"]
        assert [bool(a) for a in s2["panels"]] == [False, True, False, True] * v["L"]
        # 3. the batch that grows the mask (no workspace growth: the graph survives on that account)
        big.run(hist)
        # 4. BEFORE any replay
        s4 = ch.ctx_state(L, hist, 0)
        unchanged = all(b == a for a, b in zip(s2["panels"], s4["panels"]) if a)
        assert s4["vgraphs"] == 0 or unchanged, "resident-panel table entries changed while %d vision graph(s) were still instantiated: %s -> %s" % (
            s4["vgraphs"], s2["panels"], s4["panels"])
        assert s4["mask"] & s2["mask"] == s2["mask"] and s4["mask"] == 15, s4
        assert all(s4["panels"]) and len(set(s4["panels"])) == len(s4["panels"])
        assert s4["ws_bytes"] == s2["ws_bytes"] and s4["vgraphs"] == s2["vgraphs"]          # the scenario is not vacuous: the graph is still there
        # 5. replay
        again = small.run(hist)
        assert np.array_equal(again, kept) and np.array_equal(again, want), (_bits_differ(again, kept), _bits_differ(again, want))
    finally:
        fresh.close()
        hist.close()


# ---- defect 3: the vision graph key and device_shared -----------------------------------------------------------------------------------

def test_device_shared_flip_is_the_fresh_result_of_that_setting(gpu, torch, fixture_cache):
    """hist_w, f16, B = 32 (10400 rows): alone on the device q/k/v and FFN-up run on the 32 x 32 x 16 kernel and the LayerNorms are folded into the
    GEMM epilogues; on a shared device the two GEMMs sit on the 8-wave panel tile and the LayerNorms are launched.  A graph captured under one
    setting must not be replayed under the other: the result behind a flip is that of a context that had the setting from the start, and
    the flip back returns the first bits.  The last assertion is the discrimination check: the two settings differ in at least one bit, or
    the equalities before it could not tell a replayed graph of the other setting.

    (Not hist_v: a shape at which the flag only swaps the 32 x 32 x 16 kernel for the two-per-CU kernels does not separate the settings by
    bits — measured, those kernels return identical embeddings on fp16 weights; tests/call_history_common.py has the figures.  Which graph
    runs at such a shape is asserted on the context's state in test_device_shared_flip_captures_a_graph_of_its_own.)"""
    L = gpu.lib()
    v = ch.HIST_W["v"]
    p = fixtures.cached_model(fixture_cache, "hist_w", "f16")
    imgs = Images(torch, ch.HIST_W_IMAGES, v["S"], v["proj"], seed=43)
    a, b = gpu.Clip(p, device=0), gpu.Clip(p, device=0)
    try:
        a_first = imgs.run(a)                                            # (the first workspace allocation drops the entry of this sighting)
        assert np.array_equal(imgs.run(a), a_first)                     # first sighting that stays
        assert np.array_equal(imgs.run(a), a_first)                     # captured
        assert ch.ctx_state(L, a, 0)["vgraphs"] == 1
        a.set_device_shared(True)
        a_shared = imgs.run(a)
        b.set_device_shared(True)
        b_shared = imgs.run(b)
        assert np.all(np.isfinite(a_first)) and np.all(np.isfinite(b_shared))
        assert np.array_equal(a_shared, b_shared), "%d words differ from a context that was shared from the start" % _bits_differ(a_shared, b_shared)
        a.set_device_shared(False)
        assert np.array_equal(imgs.run(a), a_first)
        # discrimination: the two settings must differ somewhere, or the shape no longer separates the two kernels
        assert _bits_differ(b_shared, a_first) > 0, ("the shared and the unshared setting return the same bits at this shape: it no longer separates the "
                                                     "two kernels (tests/test_call_history_shapes_cpu.py should have failed first)")
    finally:
        a.close()
        b.close()


def test_device_shared_flip_captures_a_graph_of_its_own(gpu, torch, fixture_cache):
    """The flip told by the context's state, on hist_v, where the two settings run different kernels and return the same bits.  Behind the flip the
    captured graph of the other setting is not looked up: the call is a first sighting, the next one captures, and the context then holds one
    instantiated graph per setting; flipping back finds the first one again.  A key without device_shared replays the one graph it has
    and never captures a second."""
    L = gpu.lib()
    v = ch.HIST_V["v"]
    p = fixtures.cached_model(fixture_cache, "hist_v", "f16")
    imgs = Images(torch, ch.HIST_V_SMALL, v["S"], v["proj"], seed=43)
    a = gpu.Clip(p, device=0)
    try:
        first = imgs.run(a)
        imgs.run(a)
        imgs.run(a)
        assert ch.ctx_state(L, a, 0)["vgraphs"] == 1
        a.set_device_shared(True)
        assert np.array_equal(imgs.run(a), first)                       # (same bits on this hardware, by other kernels)
        assert ch.ctx_state(L, a, 0)["vgraphs"] == 1                    # a first sighting, eager
        imgs.run(a)
        assert ch.ctx_state(L, a, 0)["vgraphs"] == 2, "the shared setting was served by the graph captured unshared"
        a.set_device_shared(False)
        assert np.array_equal(imgs.run(a), first)
        assert ch.ctx_state(L, a, 0)["vgraphs"] == 2                    # found again, nothing new
    finally:
        a.close()


# ---- the wide net ------------------------------------------------------------------------------------------------------------------------

def _image_files(tmp_path, S):
    from PIL import Image as PIL
    rng = np.random.default_rng(5)
    paths = []
    for i, fmt in enumerate(("PNG", "JPEG", "BMP")):
        arr = rng.integers(0, 256, size=(S + 9 + 4 * i, S + 17, 3), dtype=np.uint8)
        buf = io.BytesIO()
        PIL.fromarray(arr).save(buf, fmt)
        path = tmp_path / ("h%d.%s" % (i, fmt.lower()))
        path.write_bytes(buf.getvalue())
        paths.append(str(path))
    return paths


@pytest.mark.parametrize("handle", ["plain", "multi"])
@pytest.mark.parametrize("config,ftype", [("tiny", "q4_0"), ("tiny14", "f16"), ("tiny14", "q5_1")])
def test_history_does_not_reach_a_later_call(gpu, torch, fixture_cache, tmp_path, config, ftype, handle):
    """Fixed target calls — images at B = 1, 7, 32, 40, texts at n = 1 and a ragged 24 — on a fresh context each, and on ONE long-lived context
    behind a seeded sequence of other calls that gets longer from target to target: other batch sizes of both towers (growing the workspace,
    crossing the 64-row small-M limit both ways, splitting over the sibling), the u8, host and file entry points, a pair call, device_shared
    and profiling on and off again, and the targets themselves repeated (first sighting, capture, replay).  Two kinds of handle, because no
    context takes both: a plain one has the file entry point in its history, a one-device multi handle the pair call (both towers in one step)."""
    cfg = fixtures.CONFIGS[config]
    S, proj, npos = cfg["v"]["S"], cfg["v"]["proj"], cfg["t"]["npos"]
    T = (S // cfg["v"]["P"]) ** 2 + 1
    p = fixtures.cached_model(fixture_cache, config, ftype)
    n_split = 2500 // T                          # 2000 ... 3300 rows: a narrow tower runs such a batch as two halves on two streams
    pool = Images(torch, max(n_split, 200), S, proj, seed=51)           # history batches: prefixes of one pool
    tpool = Texts(torch, _ragged_texts(100, npos, seed=52), proj)
    one_long = Texts(torch, _full_length_texts(1, 60, seed=53), proj)   # 60 rows: the small-M path
    two_mid = Texts(torch, _full_length_texts(2, 40, seed=54), proj)    # 80 rows: just past it
    targets = [("img1", Images(torch, 1, S, proj, seed=61)), ("img7", Images(torch, 7, S, proj, seed=62)), ("img32", Images(torch, 32, S, proj, seed=63)),
               ("img40", Images(torch, 40, S, proj, seed=64)), ("txt1", Texts(torch, _full_length_texts(1, 9, seed=65), proj)),
               ("txt24", Texts(torch, _ragged_texts(24, npos, seed=66), proj))]
    u8 = [np.random.default_rng(7).integers(0, 256, size=(S + 5, S + 11, 3), dtype=np.uint8) for _ in range(3)]
    host = fixtures.synthetic_images(9, S, seed=8)
    host_texts = fixtures.synthetic_token_ids(5, seed=9, min_len=1, max_len=30)
    files = _image_files(tmp_path, S)

    def pair(c):
        oi, ot = np.zeros((12, proj), np.float32), np.zeros((tpool.n, proj), np.float32)
        c.encode_pair_device_multi([pool.x.data_ptr()], 12, [tpool.ids.data_ptr()], tpool.offs, True, oi, ot)

    def shared_round(c):
        c.set_device_shared(True)
        pool.run(c, 33)
        tpool.run(c, 10)
        c.set_device_shared(False)

    def profiled_round(c):
        c.profile(True)
        pool.run(c, 5)
        tpool.run(c, 3)
        c.profile_report(reset=True)
        c.profile(False)

    history = [lambda c: pool.run(c, 2), lambda c: pool.run(c, 3), lambda c: pool.run(c, 12), lambda c: pool.run(c, 13), lambda c: pool.run(c, 64),
               lambda c: pool.run(c, n_split), lambda c: pool.run(c, 200), lambda c: pool.run(c, 33),
               lambda c: tpool.run(c, 2), lambda c: tpool.run(c, 5), lambda c: tpool.run(c, 64), lambda c: tpool.run(c, 100),
               one_long.run, two_mid.run, one_long.run,
               lambda c: c.encode_images_u8(u8), lambda c: c.encode_images(host), lambda c: c.encode_texts(host_texts),
               pair if handle == "multi" else (lambda c: c.encode_image_files(files)), shared_round, profiled_round] + [t.run for _, t in targets]
    load = (lambda: gpu.Clip(p, n_devices=1)) if handle == "multi" else (lambda: gpu.Clip(p, device=0))

    want = {}
    for name, t in targets:                      # one fresh context per target (same kind of handle as the long-lived one)
        c = load()
        try:
            want[name] = t.run(c)
        finally:
            c.close()
        assert np.all(np.isfinite(want[name])), name

    rng = np.random.default_rng(1234)
    order = list(np.concatenate([rng.permutation(len(history)) for _ in range(4)]))     # every kind of call comes up, three times or more
    hist = load()
    try:
        for k, (name, t) in enumerate(targets):
            for _ in range(8 + 3 * k):
                history[order.pop(0)](hist)
            got = t.run(hist)
            assert np.array_equal(got, want[name]), "%s behind %d earlier rounds: %d of %d words differ" % (name, k, _bits_differ(got, want[name]), got.size)
            again = t.run(hist)                  # ... and the call straight after it (capture / replay of the target's own graph)
            assert np.array_equal(again, want[name]), "%s repeated: %d words differ" % (name, _bits_differ(again, want[name]))
    finally:
        hist.close()
