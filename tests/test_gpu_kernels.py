"""GPU tier, kernel level: the GEMMs, the small-M kernels, the LayerNorm fold and attention against the oracle / numpy on seeded inputs,
called through the C ABI test hooks (include/clip_amd.h).  The memory-bound kernels at the two ends of each tower (text embedding, im2col,
LayerNorm and its fold entry, row copies, L2 normalisation, conversions) are in test_gpu_entry_kernels.py.  All tests need a real MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

import attention_common as ac
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

TYPES = ["f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "f32"]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _h(x):
    """round through fp16 (what the GPU activations are)."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def run_gemm(L, tid, raw, N, K, X, bias=None, resid=None, epi=0, tile=0):
    M = X.shape[0]
    y = np.full((M, N), np.nan, dtype=np.float32)
    rc = L.clip_amd_test_gemm(tid, raw.ctypes.data_as(C.c_void_p), N, K, _fp(X), M,
                              _fp(bias) if bias is not None else None, _fp(resid) if resid is not None else None, _fp(y), epi, tile)
    assert rc == 0, "clip_amd_test_gemm rc=%d" % rc          # -6: a guard row behind the output changed
    _assert_written(y, "clip_amd_test_gemm")
    return y


def _assert_written(y, what):
    """the hooks poison their output buffers (include/clip_amd.h): an element no kernel wrote comes back as NaN."""
    bad = np.argwhere(~np.isfinite(y))
    assert np.all(np.isfinite(y)), "%s: %d/%d elements not finite / not written, first %s, rows %d..%d cols %d..%d" % (
        what, len(bad), y.size, bad[0].tolist(), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


def _diff_report(base, y):
    """where two outputs that should be bit-identical differ (assertion message of the bitwise tile tests)."""
    bad = np.argwhere(~((y == base) | (np.isnan(y) & np.isnan(base))))
    if not len(bad):
        return "identical"
    r, c = bad[:, 0], bad[:, 1]
    return "%d elements differ: rows %d..%d (16-row groups %s) cols %d..%d (16-col groups %s); first %s got %r want %r; nan %d" % (
        len(bad), r.min(), r.max(), sorted(set((r // 16).tolist()))[:20], c.min(), c.max(), sorted(set((c // 16).tolist()))[:20],
        bad[0].tolist(), float(y[tuple(bad[0])]), float(base[tuple(bad[0])]), int(np.isnan(y).sum()))


def gelu_tanh(x):
    x = x.astype(np.float64)
    return 0.5 * x * (1 + np.tanh(0.7978845608028654 * x * (1 + 0.044715 * x * x)))


def gelu_quick(x):
    x = x.astype(np.float64)
    return x / (1 + np.exp(-1.702 * x))


@pytest.fixture(scope="module")
def L(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib.lib()


def _weights(rng, N, K):
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    W[:, rng.integers(0, K, size=max(1, K // 128))] *= 8.0   # outlier columns
    return W


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("shape", [(50, 64, 64), (77, 96, 128), (130, 192, 256), (257, 768, 768), (16, 512, 3072)])
def test_gemm_all_weight_types_vs_dequant_reference(L, tname, shape):
    """Y = X.W^T + b for every weight format: exact up to the fp16 rounding of the dequantised weight
    (<= 2^-11 relative per product) -> rigorous elementwise bound 1e-3 * (|X|.|W|^T)."""
    M, N, K = shape
    rng = np.random.default_rng(hash((tname, shape)) % (2 ** 31))
    tid = ref.GGML_TYPES[tname]
    W = _weights(rng, N, K)
    raw = ref.quantize(tid, W)
    Wd = ref.dequantize(tid, raw, N, K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    y = run_gemm(L, tid, raw, N, K, X, bias=bias, epi=0)
    Xh = _h(X)
    want = Xh.astype(np.float64) @ Wd.astype(np.float64).T + bias
    bound = 1.0e-3 * (np.abs(Xh).astype(np.float64) @ np.abs(Wd).astype(np.float64).T) + 1e-5
    err = np.abs(y - want)
    assert np.all(np.isfinite(y))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "%d/%d bad, first %s got %g want %g; max err %g" % (
        len(bad), y.size, bad[0], y[tuple(bad[0])], want[tuple(bad[0])], err.max())
    # and close (statistically) to the ggml-numerics oracle, whose own noise is the q8 activation quantisation
    yo = ref.mul_mat(tid, raw, N, K, X, ref.MODE_FAITHFUL) + bias
    rel = np.linalg.norm(y - yo) / np.linalg.norm(yo)
    assert rel < (5e-4 if tname in ("f16", "f32") else 2e-2), rel


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (50, 768, 768), (257, 1024, 4096), (1600, 2304, 768), (333, 80, 192)])
@pytest.mark.parametrize("epi", [0, 1, 3, 4])
def test_f32_weights_are_multiplied_in_f32(L, M, N, K, epi):
    """f32 GGUF weights (round 5, k_gemm_f32.hip): f32 weights x fp16 activations (widened exactly) on v_mfma_f32_16x16x4_f32, f32
    accumulation — against the float64 product of the SAME operands the error is f32 rounding of the accumulation (~1e-6 of sum |x||w|), a
    thousand times below what an fp16-rounded weight costs (2^-11); every epilogue family, edges inside the 64 x 64 tile."""
    rng = np.random.default_rng(M + N + K + epi)
    W = _weights(rng, N, K)
    raw = ref.quantize(0, W)                                 # ggml type 0 = f32: the bytes of W
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32) if epi == 4 else None
    y = run_gemm(L, 0, raw, N, K, X, bias=bias, resid=resid, epi=epi)
    Xh = _h(X).astype(np.float64)
    lin = Xh @ W.astype(np.float64).T + bias
    mag = np.abs(Xh) @ np.abs(W.astype(np.float64)).T + np.abs(bias)
    if epi == 0:
        assert np.all(np.abs(y - lin) <= 2e-6 * mag + 1e-7), np.abs(y - lin).max()
    elif epi == 4:
        assert np.all(np.abs(y - (lin + resid)) <= 2e-6 * (mag + np.abs(resid)) + 1e-7)
    else:
        want = lin if epi == 1 else lin / (1.0 + np.exp(-1.702 * lin))
        assert np.all(np.abs(y - want) <= np.abs(want) * 2.0 ** -10 + 2e-6 * mag + 1e-6), np.abs(y - want).max()   # the output's own fp16 rounding
    assert np.array_equal(y, run_gemm(L, 0, raw, N, K, X, bias=bias, resid=resid, epi=epi))


@pytest.mark.parametrize("tile", [64064, 64128, 128064, 128128, 160128, 192128, 96256, 128256, 160256, 256256, 256259])
@pytest.mark.parametrize("tname", ["f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0"])
def test_gemm_tiles_are_bitwise_identical(L, tile, tname):
    """Every tile shape accumulates each output in the same k order -> identical bits; also exercises M/N edges."""
    rng = np.random.default_rng(42)
    M, N, K = 203, 320, 192
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    base = run_gemm(L, tid, raw, N, K, X, epi=0, tile=64064)
    y = run_gemm(L, tid, raw, N, K, X, epi=0, tile=tile)
    assert np.array_equal(base, y), _diff_report(base, y)


@pytest.mark.parametrize("ksplit,tile", [(2, 64064), (3, 64064), (5, 64128), (12, 64064), (3, 65064), (4, 65128)])
@pytest.mark.parametrize("tname,epi", [("q4_0", 4), ("f16", 1), ("q8_0", 3), ("q5_1", 0)])
def test_gemm_split_k_is_deterministic_and_matches_unsplit(L, ksplit, tile, tname, epi):
    """Small-M path: K split over `ksplit` workgroups per tile with the in-kernel ordered fix-up.  Two runs give the
    same bits (summation order does not depend on arrival order); the result differs from the unsplit one only by
    fp32 re-association."""
    rng = np.random.default_rng(100 + ksplit)
    M, N, K = 50, 320, 1536
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    code = ksplit * 1000000 + tile
    a = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=code)
    b = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=code)
    assert np.array_equal(a, b)
    base = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=1000000 + tile)
    assert np.abs(a - base).max() <= 2e-3 * max(1.0, np.abs(base).max())
    auto = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=0)     # heuristic (splits here)
    assert np.abs(auto - base).max() <= 2e-3 * max(1.0, np.abs(base).max())


RING_TILES = [65064, 65128]     # k_gemm_ring.hip: 64 activation rows x 64 / 128 weight rows, LDS ring of K-tiles


@pytest.mark.parametrize("tile", RING_TILES)
@pytest.mark.parametrize("tname", ["f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0"])
@pytest.mark.parametrize("shape,epi", [((203, 320, 192), 0), ((1600, 768, 768), 4), ((130, 2304, 768), 1), ((333, 512, 2048), 3), ((77, 80, 64), 2)])
def test_gemm_ring_kernel_is_bitwise_identical_to_the_two_buffer_kernel(L, tile, tname, shape, epi):
    """The mid-M ring kernel (raw-quant staging, dequantisation per MFMA fragment, 3-4 K-tiles in flight, counted waits) accumulates
    in the same k order from the same fp16 operand values as k_gemm.hip: identical bits for every weight type, M / N edges
    (rows and weight rows past the end are clamped reads), K-tile counts from 1 (shorter than the ring) to 48, all epilogues."""
    M, N, K = shape
    rng = np.random.default_rng(hash((shape, tname)) % (2 ** 31))
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    base = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=64064)
    y = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=tile)
    assert np.array_equal(base, y), _diff_report(base, y)


@pytest.mark.parametrize("tile", RING_TILES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448])
def test_gemm_ring_lengths_around_the_ring_depth(L, tile, K):
    """1 … 7 K-tiles: fewer tiles than ring stages (the prologue's clamped requests), exactly the ring depth, one more."""
    rng = np.random.default_rng(K + tile)
    M, N = 150, 384
    for tname in ("q4_0", "q5_1", "f16"):
        tid = ref.GGML_TYPES[tname]
        raw = ref.quantize(tid, _weights(rng, N, K))
        X = rng.standard_normal((M, K)).astype(np.float32)
        base = run_gemm(L, tid, raw, N, K, X, epi=0, tile=64064)
        y = run_gemm(L, tid, raw, N, K, X, epi=0, tile=tile)
        assert np.array_equal(base, y), (tname, _diff_report(base, y))


def test_gemm_ring_race_screen(L):
    """Many tiles, repeated: a missing wait or barrier in the ring (a stage overwritten while it is read, a tile read before it
    landed) shows up as run-to-run differences under load."""
    rng = np.random.default_rng(7)
    M, N, K = 2500, 1536, 1024
    tid = ref.GGML_TYPES["q4_0"]
    raw = ref.quantize(tid, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    base = run_gemm(L, tid, raw, N, K, X, epi=0, tile=64064)
    for tile in RING_TILES + [2000000 + 65128, 3000000 + 65064]:
        first = run_gemm(L, tid, raw, N, K, X, epi=0, tile=tile)
        if tile < 1000000:
            assert np.array_equal(base, first), (tile, _diff_report(base, first))
        else:
            assert np.abs(first - base).max() <= 2e-3 * max(1.0, np.abs(base).max())
        for _ in range(5):
            again = run_gemm(L, tid, raw, N, K, X, epi=0, tile=tile)
            assert np.array_equal(first, again), (tile, _diff_report(first, again))


@pytest.mark.parametrize("epi", [1, 2, 3, 4])
def test_gemm_epilogues(L, epi):
    rng = np.random.default_rng(7 + epi)
    M, N, K = 100, 256, 128
    tid = ref.GGML_TYPES["q4_0"]
    raw = ref.quantize(tid, _weights(rng, N, K) * 4)
    Wd = ref.dequantize(tid, raw, N, K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    y = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi)
    lin = _h(X).astype(np.float64) @ Wd.astype(np.float64).T + bias
    if epi == 1:
        want, tol = lin, 2e-3
    elif epi == 2:
        want, tol = gelu_tanh(lin), 2e-3
    elif epi == 3:
        want, tol = gelu_quick(lin), 2e-3
    else:
        want, tol = lin + resid, 1e-3
    np.testing.assert_allclose(y, want, atol=tol * max(1.0, np.abs(want).max()), rtol=2e-3)


def test_gemm_detects_transposes(L):
    """A = I style check with an ASYMMETRIC weight: catches row/col swaps of the MFMA C layout."""
    N = K = 64
    W = np.zeros((N, K), dtype=np.float32)
    for n in range(N):
        W[n, (n * 7 + 3) % K] = 1.0 + n / 64.0
    raw = ref.quantize(1, W)
    X = np.arange(64 * K, dtype=np.float32).reshape(64, K) % 13 - 6
    y = run_gemm(L, 1, raw, N, K, X, epi=0)
    want = X @ _h(W).T
    np.testing.assert_allclose(y, want, atol=1e-3)


@pytest.mark.parametrize("h", [64, 512, 768, 1024, 1280])
def test_layernorm_vs_oracle(L, h):
    rng = np.random.default_rng(h)
    rows = 37
    x = (rng.standard_normal((rows, h)) * 3 + 0.5).astype(np.float32)
    w = (1 + rng.standard_normal(h) * 0.05).astype(np.float32)
    b = (rng.standard_normal(h) * 0.05).astype(np.float32)
    y = np.empty_like(x)
    assert L.clip_amd_test_layernorm(_fp(x), _fp(w), _fp(b), 1e-5, rows, h, _fp(y), 0) == 0
    want = ref.layer_norm(x, w, b, 1e-5)
    np.testing.assert_allclose(y, want, atol=2e-5, rtol=1e-5)
    y16 = np.empty_like(x)
    assert L.clip_amd_test_layernorm(_fp(x), _fp(w), _fp(b), 1e-5, rows, h, _fp(y16), 1) == 0
    np.testing.assert_allclose(y16, _h(want), atol=4e-3, rtol=1e-3)


def attention_ref(qkv, nseq, T, h, nh, causal):
    """the float64 definition on the fp16-rounded inputs and what its element-wise fp16 bound is made of (tests/attention_common.py)"""
    return ac.attention_ref_ragged(qkv, ac.uniform_starts(nseq, T), h, nh, causal, True)


@pytest.mark.parametrize("cfg", [(3, 17, 64, 2, 0), (2, 50, 768, 12, 0), (2, 257, 1024, 16, 0), (1, 257, 1280, 16, 0),
                                 (5, 9, 512, 8, 1), (2, 77, 512, 8, 1), (1, 1, 64, 2, 1), (1, 64, 128, 2, 0), (1, 288, 128, 2, 1),
                                 (2, 577, 1024, 16, 0), (1, 300, 128, 2, 0), (1, 592, 64, 1, 1),   # 336-px ViT-L/14: T = 577
                                 (2, 257, 1408, 16, 0), (3, 50, 176, 2, 0), (2, 77, 176, 2, 1),     # d_head 88 (ViT-g/14)
                                 (1, 257, 1664, 16, 0), (3, 17, 208, 2, 0), (2, 77, 208, 2, 1), (1, 288, 104, 1, 1)])   # d_head 104 (ViT-bigG/14)
def test_attention_vs_reference(L, cfg):
    nseq, T, h, nh, causal = cfg
    rng = np.random.default_rng(sum(cfg))
    flat = (rng.standard_normal((nseq * T, 3 * h)) * 0.7).astype(np.float32)
    flat[:, :h] *= 1.0 / np.sqrt(h // nh)   # q arrives pre-scaled
    peaked = ac.make_ragged_qkv([T] * nseq, h, nh, 6, sum(cfg), guard=0)[0]      # score scale 6 and one dominant key per sequence
    for what, qkv in (("flat", flat), ("peaked", peaked)):
        out = np.full((nseq * T, h), np.nan, dtype=np.float32)
        rc = L.clip_amd_test_attention(_fp(qkv), nseq, T, h, nh, causal, _fp(out))
        assert rc == 0, rc
        defn = attention_ref(qkv, nseq, T, h, nh, causal)
        assert np.all(np.isfinite(out))
        err = np.abs(out - defn.want).max()
        assert err < 4e-3, (cfg, what, err)
        r = ac.err_over_bound(out, defn, ac.fp16_bound(defn))
        assert r <= 1.0, (cfg, what, "max err / element-wise fp16 bound", r)


def run_gemm_ex(L, tid, raw, N, K, X, bias=None, epi=0, tile=0, qcols=0, qscale=1.0, Np=0, T=0, pos=None, y=None):
    M = X.shape[0]
    if y is None:
        y = np.full((M, N), np.nan, dtype=np.float32)
    rc = L.clip_amd_test_gemm_ex(tid, raw.ctypes.data_as(C.c_void_p), N, K, _fp(X), M, _fp(bias) if bias is not None else None, None,
                                 _fp(y), epi, tile, qcols, qscale, Np, T, _fp(pos) if pos is not None else None)
    assert rc == 0, "clip_amd_test_gemm_ex rc=%d" % rc
    _assert_written(y, "clip_amd_test_gemm_ex")
    return y


# The GEMM shapes of the TEXT tower at the BASELINE workload (256 ragged texts = 10290 token rows; ViT-B/32 text: h=512, ff=2048;
# ViT-L/14 text: h=768, ff=3072) plus odd row counts: 192-row tiles, N = 512 ... 3072, K = 512 ... 3072 (reference clip.cpp:1079-1136).
TEXT_SHAPES = [(10290, 1536, 512), (10290, 2048, 512), (10290, 512, 2048), (10290, 512, 512),
               (1531, 512, 512), (769, 2048, 512), (4099, 2304, 768), (2051, 768, 3072)]


@pytest.mark.parametrize("tname", ["q4_0", "f16"])
@pytest.mark.parametrize("shape", TEXT_SHAPES)
def test_gemm_text_tower_shapes_vs_dequant_reference(L, tname, shape):
    M, N, K = shape
    rng = np.random.default_rng(hash((tname, shape, "text")) % (2 ** 31))
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    Xh = _h(X).astype(np.float64)
    want = Xh @ Wd.T + bias
    bound = 1.0e-3 * (np.abs(Xh) @ np.abs(Wd).T) + 1e-5
    base = None
    for tile in (0, 192128, 128128, 160256):               # heuristic choice, the 192-row tile, a square tile, the 8-wave large-M kernel
        y = run_gemm(L, tid, raw, N, K, X, bias=bias, epi=0, tile=tile)
        assert np.all(np.isfinite(y))
        bad = np.argwhere(np.abs(y - want) > bound)
        assert bad.size == 0, "tile %d: %d/%d bad, first %s got %g want %g" % (tile, len(bad), y.size, bad[0], y[tuple(bad[0])], want[tuple(bad[0])])
        if tile == 0:
            continue                                       # the heuristic may split K at small M: fp32 re-association, bound only
        if base is None:
            base = y
        else:
            assert np.array_equal(y, base), "tile %d differs bitwise from tile 192128" % tile
    # the residual epilogue (out-proj / FFN-down, f32 stream) at the same shape
    resid = rng.standard_normal((M, N)).astype(np.float32)
    yr = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=4)
    assert np.all(np.abs(yr - (want + resid)) <= bound + 1e-6 * np.abs(resid))


@pytest.mark.parametrize("tname", ["q4_0", "q5_1", "f16"])
@pytest.mark.parametrize("M,N,K,qcols", [(203, 384, 128, 128), (1600, 2304, 768, 768), (77, 1536, 512, 512), (130, 192, 64, 100)])
def test_gemm_f16_epilogue_q_scale_columns(L, tname, M, N, K, qcols):
    """EPI_F16 with qcols > 0: columns n < qcols carry (acc + bias) * qscale (scale AFTER the bias, reference clip.cpp:1363),
    the others acc + bias.  Elementwise bound; a wrong scale on a single column fails."""
    rng = np.random.default_rng(M * 7 + N)
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K) * 4)
    Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    qscale = 0.125 if qcols != 100 else 0.3
    Xh = _h(X).astype(np.float64)
    lin = Xh @ Wd.T + bias
    want = lin.copy()
    want[:, :qcols] *= np.float32(qscale)
    y = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=1, qcols=qcols, qscale=qscale)
    # fp16 output: half an ulp of the result + the dequant-product bound
    bound = 1.0e-3 * (np.abs(Xh) @ np.abs(Wd).T + np.abs(bias)) + np.abs(want) * 2.0 ** -10 + 1e-4
    bad = np.argwhere(np.abs(y - want) > bound)
    assert bad.size == 0, "%d bad, first %s got %g want %g" % (len(bad), bad[0], y[tuple(bad[0])], want[tuple(bad[0])])
    # the boundary column pair must differ by the scale: column qcols-1 scaled, column qcols not
    np.testing.assert_allclose(y[:, qcols - 1], want[:, qcols - 1], atol=float(bound[:, qcols - 1].max()))
    np.testing.assert_allclose(y[:, qcols], want[:, qcols], atol=float(bound[:, qcols].max()))


@pytest.mark.parametrize("B,G,h,P", [(3, 7, 768, 32), (2, 16, 1024, 14), (5, 4, 64, 8), (33, 7, 768, 32)])
def test_gemm_patch_embedding_epilogue(L, B, G, h, P):
    """EPI_PATCH_F32 (patch embedding, reference clip.cpp:1309-1331): GEMM row m = (image, patch) is scattered to token row
    image * T + 1 + patch and gets position_embd[1 + patch] added; no bias; class-token rows are not written."""
    rng = np.random.default_rng(B * 100 + G)
    Np, T, K = G * G, G * G + 1, 3 * P * P
    Wf = (rng.standard_normal((h, K)) * 0.02).astype(np.float32)
    raw = ref.quantize(1, Wf)                               # an f16 patch kernel; the f32 one: test_gpu_gemm_f32.py
    Wd = ref.dequantize(1, raw, h, K).astype(np.float64)
    X = rng.standard_normal((B * Np, K)).astype(np.float32)
    pos = (rng.standard_normal((T, h)) * 0.02).astype(np.float32)
    y = np.full((B * T, h), 777.0, dtype=np.float32)
    y = run_gemm_ex(L, 1, raw, h, K, X, epi=5, Np=Np, T=T, pos=pos, y=y)
    Xh = _h(X).astype(np.float64)
    lin = Xh @ Wd.T
    bound = 1.0e-3 * (np.abs(Xh) @ np.abs(Wd).T) + 1e-5
    y3 = y.reshape(B, T, h)
    assert np.all(y3[:, 0, :] == 777.0)                     # class rows untouched
    want = lin.reshape(B, Np, h) + pos[None, 1:, :]
    assert np.all(np.abs(y3[:, 1:, :] - want) <= bound.reshape(B, Np, h))


@pytest.mark.parametrize("tile", [96256, 128256, 160256, 256256, 256259])
@pytest.mark.parametrize("K", [64, 128, 192, 256, 448, 1024])
@pytest.mark.parametrize("tname,epi", [("f16", 0), ("q4_0", 4), ("q5_1", 1), ("q8_0", 2)])
def test_gemm8_ring_lengths_and_epilogues_match_the_4_wave_kernel_bitwise(L, tile, K, tname, epi):
    """8-wave large-M kernel (k_gemm8.hip): 1 ... 16 K-tiles through the 3-stage LDS ring (prologue / steady state / tail of the
    counted-vmcnt pipeline), M and N edges inside a tile, block-quantised weights through the dequantised fp16 panel, every
    epilogue family: bit-identical to the 64x64 tile of the 4-wave kernel (same MFMA, same k order, same dequant arithmetic)."""
    rng = np.random.default_rng(K * 13 + tile)
    M, N = 333, 576
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K) * 3)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    base = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=1000000 + 64064)   # unsplit 64x64 tiles
    y = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=tile)
    assert np.all(np.isfinite(y))
    assert np.array_equal(base, y), _diff_report(base, y)
    y2 = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=tile)
    assert np.array_equal(y, y2)


@pytest.mark.parametrize("seed", range(6))
def test_large_m_kernels_random_shapes_bitwise(L, seed):
    """Seeded random (M, N, K): edges anywhere inside a 256 x 256 tile, 1 ... 11 K-tiles, random epilogue, bias present or not — the
    8-wave and four-wave kernels against the 64 x 64 tile of the 4-wave kernel, bit for bit."""
    rng = np.random.default_rng(1000 + seed)
    for _ in range(4):
        M = int(rng.integers(1, 1400))
        N = int(rng.integers(4, 70)) * 16
        K = int(rng.integers(1, 12)) * 64
        epi = int(rng.choice([0, 1, 2, 3, 4]))
        tname = str(rng.choice(["f16", "q4_0", "q5_1", "q8_0"]))
        tid = ref.GGML_TYPES[tname]
        raw = ref.quantize(tid, _weights(rng, N, K) * 3)
        X = rng.standard_normal((M, K)).astype(np.float32)
        bias = (rng.standard_normal(N) * 0.5).astype(np.float32) if rng.integers(0, 2) else None
        resid = rng.standard_normal((M, N)).astype(np.float32) if epi == 4 else None
        base = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=1000000 + 64064)
        for tile in (160256, 256256, 256259):
            y = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=tile)
            assert np.array_equal(base, y), ((M, N, K), tname, epi, tile, _diff_report(base, y))


def test_gemm8_many_tiles_race_screen(L):
    """More workgroups than CUs, several rounds, repeated: a ring / barrier race shows up as a rare wrong tile."""
    rng = np.random.default_rng(5)
    M, N, K = 4000, 1024, 768
    raw = ref.quantize(1, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    base = run_gemm(L, 1, raw, N, K, X, epi=0, tile=128128)
    for _ in range(6):
        assert np.array_equal(run_gemm(L, 1, raw, N, K, X, epi=0, tile=160256), base)
        assert np.array_equal(run_gemm(L, 1, raw, N, K, X, epi=0, tile=256256), base)     # 2-deep ring form
        assert np.array_equal(run_gemm(L, 1, raw, N, K, X, epi=0, tile=256259), base)     # 4-wave 128 x 128 form (k_gemm4.hip)


@pytest.mark.parametrize("tname,epi", [("f16", 1), ("q4_0", 4), ("q8_0", 3), ("q5_0", 0)])
def test_gemm8_whole_rounds_split_is_bitwise_identical(L, tname, epi):
    """Tile code 256258: the tile rows that fill whole rounds of 256 workgroups go to the 256 x 256 kernel, the remaining rows to a
    second launch with the heuristic's tile.  Row-local epilogues, no K split: the same bits as one launch of any tile."""
    rng = np.random.default_rng(11)
    M, N, K = 5000, 3584, 128            # 20 x 14 = 280 tiles: 18 tile rows (4608 rows) in the first launch, 392 rows in the second
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K) * 3)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    base = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=128128)
    for tile in (256258, 256260):
        y = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi, tile=tile)
        assert np.array_equal(base, y), (tile, np.abs(base - y).max())


def run_skinny(L, tid, raw, N, K, X, bias=None, resid=None, ln=None, epi=0, qcols=0, qscale=1.0, stats=None):
    M = X.shape[0]
    y = np.full((M, N), np.nan, dtype=np.float32)
    lw, lb, eps = (ln if ln is not None else (None, None, 0.0))
    rc = L.clip_amd_test_skinny(tid, raw.ctypes.data_as(C.c_void_p), N, K, _fp(X), M, _fp(bias) if bias is not None else None,
                                _fp(resid) if resid is not None else None, _fp(lw) if lw is not None else None,
                                _fp(lb) if lb is not None else None, eps, _fp(y), epi, qcols, qscale, _fp(stats) if stats is not None else None)
    assert rc == 0, "clip_amd_test_skinny rc=%d" % rc
    _assert_written(y, "clip_amd_test_skinny")
    return y


@pytest.mark.parametrize("tname", TYPES[:6])
@pytest.mark.parametrize("M,N,K", [(50, 768, 768), (1, 512, 512), (49, 1536, 512), (64, 768, 3072), (50, 2304, 768), (64, 1024, 4096), (17, 80, 64),
                                   (100, 768, 3072), (257, 512, 512)])
def test_skinny_gemm_vs_dequant_reference_and_tiled_kernel(L, tname, M, N, K):
    """k_skinny.hip (one 16-row block per workgroup, rows split over grid.y): every weight type, both wave counts (K >= 2048 -> 8 waves),
    one to 17 row blocks incl. a ragged last one,
    f32 / residual / f16 epilogues: elementwise bound against the float64 product of the dequantised operands, and within fp32
    re-association of the tiled kernel's result."""
    rng = np.random.default_rng(M * 1000 + N + K)
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    Xh = _h(X).astype(np.float64)
    lin = Xh @ Wd.T + bias
    bound = 1.0e-3 * (np.abs(Xh) @ np.abs(Wd).T) + 1e-5
    y = run_skinny(L, tid, raw, N, K, X, bias=bias, epi=0)
    assert np.all(np.abs(y - lin) <= bound), np.abs(y - lin).max()
    tiled = run_gemm(L, tid, raw, N, K, X, bias=bias, epi=0, tile=1000000 + 64064)
    assert np.abs(y - tiled).max() <= 1e-4 * max(1.0, np.abs(tiled).max())
    assert np.array_equal(y, run_skinny(L, tid, raw, N, K, X, bias=bias, epi=0))            # deterministic
    stats = np.zeros((128, 128, 2), dtype=np.float32)          # [row][slot][sum, sum of squares]
    yr = run_skinny(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=4, stats=stats)
    assert np.all(np.abs(yr - (lin + resid)) <= bound + 1e-6 * np.abs(resid))
    # the partial statistics the residual epilogue leaves: per row, over each workgroup's 16 columns
    if (N + 15) // 16 <= 128:                                  # (the residual GEMMs of a model have N = hidden size <= 2048)
        Ms = min(M, 128)                                       # (the hook returns the statistics of the first 128 rows)
        s1 = stats[:Ms, : (N + 15) // 16, 0].sum(1)
        s2 = stats[:Ms, : (N + 15) // 16, 1].sum(1)
        np.testing.assert_allclose(s1, yr[:Ms].astype(np.float64).sum(1), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(s2, (yr[:Ms].astype(np.float64) ** 2).sum(1), rtol=1e-4)


@pytest.mark.parametrize("tname", ["q4_0", "f16", "q5_1"])
@pytest.mark.parametrize("M,N,K,epi", [(50, 2304, 768, 1), (50, 3072, 768, 3), (64, 2048, 512, 2), (33, 3072, 1024, 3), (1, 1280, 1280, 1), (150, 1536, 512, 1)])
def test_skinny_layernorm_fused_projection(L, tname, M, N, K, epi):
    """LN fused on the A operand: out = act(LayerNorm(x) . W^T + b) with LayerNorm as in the standalone kernel (output rounded to fp16
    before the product).  Reference: float64 LayerNorm -> fp16 -> float64 product; the one-pass variance and the fp16 rounding of
    values that sit on a rounding boundary allow a few ulps of the fp16 activations."""
    rng = np.random.default_rng(M + N + K + epi)
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
    X = (rng.standard_normal((M, K)) * 2.5 + 0.3).astype(np.float32)
    lw = (1 + rng.standard_normal(K) * 0.05).astype(np.float32)
    lb = (rng.standard_normal(K) * 0.05).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    xn = ref.layer_norm(X, lw, lb, 1e-5)
    xh = _h(xn).astype(np.float64)
    lin = xh @ Wd.T + bias
    want = {1: lin, 2: gelu_tanh(lin), 3: gelu_quick(lin)}[epi]
    qc, qs = ((N // 3) // 4 * 4, 0.125) if epi == 1 else (0, 1.0)       # Q-scale columns of the fused q/k/v projection
    want = want.copy()
    want[:, :qc] *= qs
    y = run_skinny(L, tid, raw, N, K, X, bias=bias, ln=(lw, lb, 1e-5), epi=epi, qcols=qc, qscale=qs)
    # LN output differs from the float64 reference by <= ~1 fp16 ulp on a few elements: bound 2^-10 * |xn| . |W|
    bound = 2.0e-3 * (np.abs(xh) @ np.abs(Wd).T) + np.abs(want) * 2.0 ** -10 + 2e-4
    bad = np.argwhere(np.abs(y - want) > bound)
    assert bad.size == 0, (len(bad), np.abs(y - want).max())
    rel = np.linalg.norm(y - want) / np.linalg.norm(want)
    assert rel < 1e-3, rel


# ---- LayerNorm folded into the GEMM epilogues (gemm_common.h: resid_fold_tail / ln_rows_load; reference clip.cpp:1350-1355,1400-1405) ----
def run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, tile1, tile2, fold, qcols=0, qscale=1.0, eps=1e-5):
    M = A.shape[0]
    x1 = np.full((M, h), np.nan, dtype=np.float32)
    y = np.full((M, N2), np.nan, dtype=np.float32)
    rc = L.clip_amd_test_lnfold(tid, raw1.ctypes.data_as(C.c_void_p), h, K1, raw2.ctypes.data_as(C.c_void_p), N2, _fp(A), M, _fp(b1), _fp(resid),
                                _fp(g), _fp(beta), eps, _fp(b2), epi2, tile1, tile2, fold, qcols, qscale, _fp(x1), _fp(y))
    assert rc == 0, "clip_amd_test_lnfold rc=%d" % rc
    _assert_written(x1, "clip_amd_test_lnfold x1")
    _assert_written(y, "clip_amd_test_lnfold y")
    return x1, y


def _lnfold_case(rng, tname, M, h, K1, N2, mean_shift=0.3, outlier=20.0):
    tid = ref.GGML_TYPES[tname]
    raw1 = ref.quantize(tid, _weights(rng, h, K1))
    W2 = _weights(rng, N2, h)
    raw2 = ref.quantize(tid, W2)
    Wd2 = ref.dequantize(tid, raw2, N2, h).astype(np.float64)
    A = rng.standard_normal((M, K1)).astype(np.float32)
    resid = rng.standard_normal((M, h)) * 2.5
    resid[:, rng.integers(0, h, size=2)] *= outlier         # outlier channels of the residual stream (about zero), then the common mode
    resid = (resid + mean_shift).astype(np.float32)
    b1 = (rng.standard_normal(h) * 0.1).astype(np.float32)
    g = (1 + rng.standard_normal(h) * 0.2).astype(np.float32)
    beta = (rng.standard_normal(h) * 0.1).astype(np.float32)
    b2 = (rng.standard_normal(N2) * 0.1).astype(np.float32)
    return tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2


def _lnfold_reference(x1, g, beta, Wd2, b2, epi2, qcols, qscale, eps=1e-5):
    """float64 LayerNorm of the GPU's own f32 residual rows -> exact product; bound = fp16 rounding of the folded operand x * gamma."""
    x = x1.astype(np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    ln = (x - mu) * rstd * g + beta
    lin = ln @ Wd2.T + b2
    want = {1: lin, 2: gelu_tanh(lin), 3: gelu_quick(lin)}[epi2].copy()
    want[:, :qcols] *= qscale
    # |sum_k W_nk e_k| <= 2^-11 sum_k |x_k gamma_k W_nk|, scaled by rstd; activations are 1.13-Lipschitz; + the output's own fp16 rounding
    pre = rstd * (2.0 ** -11) * (np.abs(x * g) @ np.abs(Wd2).T)
    bound = 1.2 * 1.05 * pre + np.abs(want) * 2.0 ** -10 + 2e-4
    return want, bound, lin


@pytest.mark.parametrize("tname", ["q4_0", "f16", "q5_1"])
@pytest.mark.parametrize("tile1,tile2,epi2", [(64064, 64064, 1), (64128, 128064, 2), (128128, 160128, 3), (160128, 192128, 1), (192128, 128128, 2),
                                              (65064, 65128, 1), (65128, 65064, 3), (3065128, 2064064, 2), (160256, 160256, 1), (256259, 256259, 3),
                                              (256256, 128256, 2), (0, 0, 1)])
@pytest.mark.parametrize("fold", [1, 2])
def test_lnfold_vs_float64_and_two_launch_form(L, tname, tile1, tile2, epi2, fold):
    """The folded form (residual epilogue emits fp16(x gamma) + partial statistics, consumer epilogue applies rstd (acc - mean c) + b')
    through every producer / consumer kernel: (a) the f32 residual rows are bit-identical to the unfolded launch, (b) the output is within
    the rigorous fp16-operand bound of the float64 LayerNorm + product, (c) folded and three-launch outputs agree to 2 fp16 ulp (99.9 % of the outputs; 3 ulp all)."""
    rng = np.random.default_rng(7 + epi2)
    M, h, K1, N2 = 203, 320, 192, 448
    tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2 = _lnfold_case(rng, tname, M, h, K1, N2)
    qc, qs = (128, 0.125) if epi2 == 1 else (0, 1.0)
    x1a, ya = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, tile1, tile2, 0, qc, qs)
    x1b, yb = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, tile1, tile2, fold, qc, qs)     # fold 2: centred operand
    if tile1 // 1000000 <= 1:     # (split-K re-associates the fp32 sums identically in both runs too: same kernel, same order)
        assert np.array_equal(x1a, x1b), _diff_report(x1a, x1b)
    want, bound, lin = _lnfold_reference(x1b, g, beta, Wd2, b2, epi2, qc, qs)
    err = np.abs(yb - want)
    bad = np.argwhere(err > bound)
    assert np.all(np.isfinite(yb))
    assert bad.size == 0, "%d/%d bad, first %s got %g want %g bound %g; max err %g" % (
        len(bad), yb.size, bad[0], yb[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])], err.max())
    # A/B: 2 fp16 ulp of max(|y|, row rms) (an output near zero keeps the absolute error of its row)
    scale = np.maximum(np.abs(ya), np.sqrt((ya.astype(np.float64) ** 2).mean(1, keepdims=True)))
    ab = np.abs(yb - ya) / (scale * 2.0 ** -10)
    # (two independently rounded fp16 operands: ~0.3 ulp of pre-rounding noise each + the output rounding; r03a observed max 2.25 over 90 k outputs)
    assert ab.max() <= 3.0 and np.quantile(ab, 0.999) <= 2.0, "A/B max %.2f ulp at %s, p99.9 %.2f" % (ab.max(), np.unravel_index(ab.argmax(), ab.shape), np.quantile(ab, 0.999))
    rel = np.linalg.norm(yb - want) / np.linalg.norm(want)
    rel0 = np.linalg.norm(ya - want) / np.linalg.norm(want)
    assert rel < 1.5 * rel0 + 1e-4, (rel, rel0)          # not noisier than the LayerNorm-kernel form


@pytest.mark.parametrize("tname", ["q4_0", "f16"])
def test_lnfold_is_bitwise_independent_of_the_producer_and_consumer_kernels(L, tname):
    """Statistics slots are 64 columns wide out of the wide kernels and 32 out of the ring / BN = 64 tiles; the consumer merges the
    32-column pairs first, which reproduces the 64-column slot exactly -> the folded output does not depend on tile shapes."""
    rng = np.random.default_rng(11)
    M, h, K1, N2 = 150, 384, 128, 320
    tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2 = _lnfold_case(rng, tname, M, h, K1, N2)
    for fold in (1, 2):            # 2: the centred operand (per-row offsets): the same invariance
        base = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, 2, 64128, 64128, fold)[1]
        for t1, t2 in [(64064, 64128), (65064, 64128), (65128, 128128), (160128, 65064), (192128, 65128), (160256, 160128), (256259, 256256), (128064, 128064), (160128, 256259), (65064, 256260)]:     # 256259 / 256260 as consumer: k_gemm4.hip (consumer half of the fold, round 5)
            y = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, 2, t1, t2, fold)[1]
            assert np.array_equal(base, y), "fold %d tiles (%d, %d): %s" % (fold, t1, t2, _diff_report(base, y))


@pytest.mark.parametrize("tname,M,h,K1,N2,epi2", [("q4_0", 1600, 768, 768, 2304, 1), ("q4_0", 1600, 768, 3072, 3072, 3), ("f16", 1300, 1024, 1024, 3072, 1),
                                                  ("q8_0", 2500, 512, 2048, 2048, 2), ("q5_1", 771, 1280, 1280, 1280, 2)])
def test_lnfold_model_shapes_heuristic_tiles(L, tname, M, h, K1, N2, epi2):
    """Model widths through the tiles the heuristic picks (ring kernel, 160 x 128, split-K), row mean up to 2 sigma away from zero:
    the fold rounds x gamma to fp16 BEFORE the mean is removed, so its error bound grows with |mean| / sigma — still inside the rigorous bound."""
    rng = np.random.default_rng(M + h)
    tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2 = _lnfold_case(rng, tname, M, h, K1, N2, mean_shift=5.0)
    qc, qs = (h, 0.125) if epi2 == 1 else (0, 1.0)
    x1b, yb = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, 0, 0, 1, qc, qs)
    want, bound, lin = _lnfold_reference(x1b, g, beta, Wd2, b2, epi2, qc, qs)
    err = np.abs(yb - want)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "%d/%d bad, max err %g" % (len(bad), yb.size, err.max())
    rel = np.linalg.norm(yb - want) / np.linalg.norm(want)
    assert rel < 2e-3, rel


@pytest.mark.parametrize("tname,M,h,K1,N2,epi2", [("q4_0", 1600, 768, 768, 2304, 1), ("f16", 1300, 1024, 1024, 4096, 3), ("q4_0", 50, 768, 3072, 3072, 3)])
def test_lnfold_centred_operand_under_large_row_means(L, tname, M, h, K1, N2, epi2):
    """VERDICT r3 item 3 / ADVICE r3: rows of the residual stream whose mean is k sigma away from zero, and outlier channels.  The r03 fold
    multiplied fp16(x gamma): its operand rounding error grows ~k-fold against the reference's normalise-first order (clip.cpp:1350-1355).
    The centred fold (fold = 2: fp16((x - mu) gamma), mu = the row's mean at the previous LayerNorm) must stay within 2x the error of the
    three-launch form everywhere in the sweep; the table goes to gpurun_out/ (DESIGN.md section 3 carries it)."""
    lines = []
    skinny = M <= 64
    t1 = -1 if skinny else 0
    for outlier in (20.0, 100.0):
        for k in (0, 2, 5, 10, 30):
            rng = np.random.default_rng(1000 + k + int(outlier))
            tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2 = _lnfold_case(rng, tname, M, h, K1, N2, mean_shift=2.5 * k, outlier=outlier)
            qc, qs = (h, 0.125) if epi2 == 1 else (0, 1.0)
            rel = {}
            for fold in (0, 1, 2):
                x1, y = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, t1, 0, fold, qc, qs)
                want, bound, lin = _lnfold_reference(x1, g, beta, Wd2, b2, epi2, qc, qs)
                assert np.all(np.isfinite(y))
                rel[fold] = float(np.linalg.norm(y - want) / np.linalg.norm(want))
                if fold == 2:
                    x64 = x1.astype(np.float64)
                    ratio = float(np.median(np.abs(x64.mean(1)) / x64.std(1)))
            lines.append("%-5s M=%-5d h=%-5d outlier x%-4g mean shift %2d sigma (median |mean|/std of the rows %.2f): rel. L2 error vs float64  three-launch %.3e  fold r03 %.3e (x%.1f)  fold centred %.3e (x%.2f)" % (
                tname, M, h, outlier, k, ratio, rel[0], rel[1], rel[1] / rel[0], rel[2], rel[2] / rel[0]))
            assert rel[2] <= 2.0 * rel[0] + 2e-5, lines[-1]
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "r04_lnfold_centre_sweep.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


# ---- the large-M kernels against float64 AT the sizes they run at (so far bit-identity to the 64 x 64 tile at
# M <= 5000 and self-consistency at real size) ----
@pytest.mark.parametrize("tname", ["f16", "q5_1"])
@pytest.mark.parametrize("M,N,K", [(33410, 1024, 1024), (65792, 1024, 1024), (65792, 4096, 1024)])
def test_large_m_kernels_vs_float64_at_model_size(L, tname, M, N, K):
    """ViT-L/14 at batch 130 / 256 (33410 / 65792 token rows; reference clip.cpp:1360-1422): the heuristic's choice there — 256 x 256
    four-wave tiles on the whole rounds + a second launch for the remaining rows (k_gemm4.hip), block-quantised weights through the
    fp16 panel — and the 8-wave 160 x 256 kernel, against the float64 product of the fp16-rounded activations with the dequantised
    weights, elementwise (bound = fp16 rounding of the dequantised weight), every row of the batch."""
    assert L.clip_amd_test_gemm_tile_ex(M, N, K, int(tname != "f16"), 1) % 1000 in (259, 260)      # the regime under test (f32 output: never k_gemm32.hip)
    rng = np.random.default_rng(M + N + K)
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K))
    Wd = ref.dequantize(tid, raw, N, K)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    Xh = _h(X)
    ys = {tile: run_gemm(L, tid, raw, N, K, X, bias=bias, epi=0, tile=tile) for tile in (0, 160256)}
    Wt64, Wabs = Wd.astype(np.float64).T.copy(), np.abs(Wd).T.copy()
    for r0 in range(0, M, 8192):                              # float64 reference in row chunks (2 GB for the largest shape otherwise)
        r1 = min(M, r0 + 8192)
        want = Xh[r0:r1].astype(np.float64) @ Wt64 + bias
        bound = 1.0e-3 * (np.abs(Xh[r0:r1]) @ Wabs).astype(np.float64) + 1e-5
        for tile, y in ys.items():
            err = np.abs(y[r0:r1] - want)
            bad = np.argwhere(err > bound)
            assert bad.size == 0, "tile %d rows %d..%d: %d bad, first %s got %g want %g" % (
                tile, r0, r1, len(bad), bad[0], y[r0 + bad[0][0], bad[0][1]], want[tuple(bad[0])])
    assert np.array_equal(ys[0], ys[160256]), _diff_report(ys[160256], ys[0])      # and the two kernels agree bit for bit
    if N == K:       # the residual epilogue of the same kernels (out-projection shape), in place as the layers run it
        resid = rng.standard_normal((M, N)).astype(np.float32)
        yr = run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=4)
        assert np.array_equal(yr, resid + ys[0]) or np.max(np.abs(yr - (resid + ys[0]))) <= 1e-6 * np.max(np.abs(resid))


@pytest.mark.parametrize("tname", ["q4_0", "f16", "q5_1", "q8_0"])
@pytest.mark.parametrize("M,h,K1,N2,epi2", [(50, 768, 768, 2304, 1), (50, 768, 3072, 3072, 3), (13, 512, 2048, 2048, 2), (64, 1024, 1024, 3072, 1), (1, 1280, 1280, 5120, 2), (77, 512, 512, 1536, 1)])
def test_lnfold_small_m_kernels(L, tname, M, h, K1, N2, epi2):
    """The folded LayerNorm on the small-M path (one image, one text): skinny residual epilogue -> fp16(x gamma) + 16-column statistics ->
    skinny consumer.  Rigorous bound against float64, agreement with the LayerNorm-fused-on-the-operand form of the same kernels, and
    the f32 residual rows bit-identical between the two forms."""
    rng = np.random.default_rng(M * 3 + h + epi2)
    tid, raw1, raw2, Wd2, A, resid, b1, g, beta, b2 = _lnfold_case(rng, tname, M, h, K1, N2)
    qc, qs = (h, 0.125) if epi2 == 1 else (0, 1.0)
    x1a, ya = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, -1, 0, 0, qc, qs)
    x1b, yb = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, -1, 0, 1, qc, qs)
    assert np.array_equal(x1a, x1b), _diff_report(x1a, x1b)
    want, bound, lin = _lnfold_reference(x1b, g, beta, Wd2, b2, epi2, qc, qs)
    err = np.abs(yb - want)
    bad = np.argwhere(err > bound)
    assert np.all(np.isfinite(yb)) and bad.size == 0, "%d/%d bad, max err %g" % (len(bad), yb.size, err.max())
    scale = np.maximum(np.abs(ya), np.sqrt((ya.astype(np.float64) ** 2).mean(1, keepdims=True)))
    ab = np.abs(yb - ya) / (scale * 2.0 ** -10)
    assert ab.max() <= 3.0 and np.quantile(ab, 0.999) <= 2.0, "A/B max %.2f ulp, p99.9 %.2f" % (ab.max(), np.quantile(ab, 0.999))
    # and against the tiled kernels' fold on the same inputs: same operand fp16(x gamma), statistics from other partial sums
    x1c, yc = run_lnfold(L, tid, raw1, h, K1, raw2, N2, A, b1, resid, g, beta, b2, epi2, 64128, 64128, 1, qc, qs)
    ab2 = np.abs(yb - yc) / (scale * 2.0 ** -10)
    assert ab2.max() <= 2.0, ab2.max()


# ---- run-to-run bit stability of the activation epilogues (round 6) ----
STABLE_TILES = [0, 64064, 64128, 65064, 65128, 128064, 128128, 160128, 192128, 160256, 256256, 256259, 256261, 320261]


@pytest.mark.parametrize("tname", ["f16", "q4_0"])
@pytest.mark.parametrize("epi", [2, 3, 1])
def test_activation_epilogues_are_bit_stable_run_to_run(L, tname, epi):
    """Round 6 regression.  A first version of the two-FMA epilogue let hipcc's SLP vectoriser pack the GELU chain (v_pk_fma_f32 -> v_exp /
    v_rcp -> v_pk_mul_f32 on the reciprocals); on gfx950 that code returned wrong quarter-waves (16 rows x 1 column) a few dozen times per
    2 M outputs, DIFFERENTLY from run to run — first seen on the text tower's FFN-up (1027 x 2048 x 512, ring kernel), invisible to every
    accuracy bound (gemm_common.h GELU_SCALAR_FENCE).  Every kernel family: 6 runs of the same product, bit for bit, at that shape and at
    one that reaches the large tiles; and inside the float64 bound."""
    tid = ref.GGML_TYPES[tname]
    for (M, N, K) in [(1027, 2048, 512), (4099, 3072, 768)]:
        rng = np.random.default_rng(M + N + epi)
        raw = ref.quantize(tid, _weights(rng, N, K))
        Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
        X = rng.standard_normal((M, K)).astype(np.float32)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        qc, qs = (N // 4, 0.125) if epi == 1 else (0, 1.0)
        lin = _h(X).astype(np.float64) @ Wd.T + bias
        want = {1: lin, 2: gelu_tanh(lin), 3: gelu_quick(lin)}[epi].copy()
        want[:, :qc] *= qs
        bound = 1.2e-3 * (np.abs(_h(X)).astype(np.float64) @ np.abs(Wd).T) + np.abs(want) * 2.0 ** -10 + 1e-4
        for tile in STABLE_TILES:
            if tile % 1000 == 261 and not (N >= 2 * K):
                continue
            base = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=epi, tile=tile, qcols=qc, qscale=qs)
            assert np.all(np.abs(base - want) <= bound), (tile, M, N, K, float(np.abs(base - want).max()))
            for _ in range(5):
                y = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=epi, tile=tile, qcols=qc, qscale=qs)
                assert np.array_equal(base, y), "tile %d (%d x %d x %d): %s" % (tile, M, N, K, _diff_report(base, y))
