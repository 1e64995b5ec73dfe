"""Shared by test_weight_side_cpu.py and test_gpu_weight_side.py: the numpy side of the weight-side kernel tests and the calls of the three hooks
(include/clip_amd.h: clip_amd_test_dequant_panels, clip_amd_test_gemm_panel, clip_amd_test_fold_vectors).

panel_want      the fp16 panel launch_dequant must leave (k_gemm8.hip dequant_kernel): dequant_fp16 in the top-left [N][K] of [Npad][Kpad], zero elsewhere.
compare_panel   value for value, no tolerance: a zero may carry either sign, a weight that is itself subnormal in fp16 may arrive exact or as zero
                (the rule of test_gpu_gemm_exact.py::test_operand_readback).
fold_exact      gamma, beta multiples of 2^-8, bias and weights multiples of 2^-6: c and b' of k_fold.hip known as integers in units of 2^-14.
fold_bound      the derived bound of the realistic fold case.
"""
import ctypes as C
import functools

import numpy as np

import gemm_exact_common as ge
from oracle import ref
from test_gpu_gemm_exact import seed, table  # noqa: F401  (table: raw_table blocks, optionally with every block scale subnormal; cached there)
from test_gpu_kernels import _weights

POISON16 = 0x7e00
F16_MIN_NORMAL = 2.0 ** -14
GUNIT = 256                    # fold_exact: gamma and beta are multiples of 2^-8 ...
FUNIT = GUNIT * ge.UNIT        # ... so every product gamma w and beta w is a multiple of 2^-14

SINGLE_SHAPES = [(80, 64), (320, 192), (128, 96)]                          # (N, K); (128, 96): an odd number of 32-blocks, the last k-block pair half padding
LAYER_SHAPES = [(576, 192), (192, 192), (768, 192), (192, 768)]            # h = 192, ff = 768: q/k/v, out, FFN-up, FFN-down
# "runs and cuts": 8 distinct shapes — the 7 above and (576, 448), the second GEMM shape of this suite, as the eighth
CUT_SHAPES = [(80, 64), (320, 192), (128, 96), (576, 192), (192, 192), (768, 192), (192, 768), (576, 448)]
CUT_TYPES = ["q4_0", "q4_0", "q4_0", "q4_0", "q4_0", "q8_0", "q5_1", "q5_1"]
GEMM_SHAPES = [(203, 320, 192), (333, 576, 448)]                           # (M, N, K)
SPLIT_SHAPE = (50, 320, 1536)
FOLD_SHAPES = [(80, 64), (320, 192), (300, 448)]
FOLD_F16_ONLY = (80, 100)                                                  # K % 8 != 0, Kpad 128


def pad_shape(N, K):
    return (N + 127) // 128 * 128, (K + 63) // 64 * 64


def panel_want(tname, raw, N, K):
    """-> float16 [Npad][Kpad]"""
    Np, Kp = pad_shape(N, K)
    want = np.zeros((Np, Kp), dtype=np.float16)
    want[:N, :K] = ge.dequant_fp16(tname, raw, N, K)
    return want


def compare_panel(got_bits, want, what):
    """got_bits uint16 [Npad][Kpad] as the hook returned it -> (subnormal weights that arrived exact, ... as zero)"""
    assert got_bits.dtype == np.uint16 and got_bits.shape == want.shape, (what, got_bits.shape, want.shape)
    n_poison = int((got_bits == POISON16).sum())
    assert n_poison == 0, "%s: %d/%d halfs of the panel still hold the poison (never written)" % (what, n_poison, got_bits.size)
    got = got_bits.view(np.float16).astype(np.float32)
    w = want.astype(np.float32)
    tiny = (w != 0) & (np.abs(w) < F16_MIN_NORMAL)
    flushed = tiny & (got == 0)
    bad = np.argwhere(np.where(flushed, w, got) != w)                      # (NaN != anything; +0 == -0)
    assert bad.size == 0, "%s: %d/%d differ, rows %d..%d cols %d..%d, first %s got %r (0x%04x) want %r" % (
        what, len(bad), got.size, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), bad[0].tolist(),
        float(got[tuple(bad[0])]), int(got_bits[tuple(bad[0])]), float(w[tuple(bad[0])]))
    return int((tiny & ~flushed).sum()), int(flushed.sum())


# --------------------------------------------------------------------------------------------------------------------------------
# the hooks
# --------------------------------------------------------------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def call_dequant_panels(L, jobs, n=None):
    """jobs: [(tname, raw, N, K)] -> (rc, guard_ok, [uint16 [Npad][Kpad]]); the panels are pre-filled with 0xffff: what the hook did not deliver stays"""
    cnt = len(jobs) if n is None else n
    m = max(len(jobs), 1)
    raws = [np.ascontiguousarray(j[1], dtype=np.uint8) for j in jobs]
    outs = [np.full(pad_shape(max(j[2], 1), max(j[3], 1)), 0xffff, dtype=np.uint16) for j in jobs]
    types = (C.c_int * m)(*[ref.GGML_TYPES.get(j[0], -1) if isinstance(j[0], str) else j[0] for j in jobs])
    Ns, Ks = (C.c_int64 * m)(*[j[2] for j in jobs]), (C.c_int64 * m)(*[j[3] for j in jobs])
    w = (C.c_void_p * m)(*[r.ctypes.data for r in raws])
    o = (C.c_void_p * m)(*[a.ctypes.data for a in outs])
    ok = C.c_int(-1)
    rc = L.clip_amd_test_dequant_panels(cnt, types, w, Ns, Ks, o, C.byref(ok))
    return rc, ok.value, outs


def run_dequant_panels(L, jobs, what=""):
    rc, ok, outs = call_dequant_panels(L, jobs)
    assert rc == 0 and ok == 1, (what, "clip_amd_test_dequant_panels rc=%d guard_ok=%d" % (rc, ok))       # -6: a half outside the panels changed
    return outs


def call_gemm_panel(L, tid, raw, raw2, N, K, X, bias=None, resid=None, epi=0, tile=0, qcols=0, qscale=1.0, panel_mode=1, lead=0):
    X = np.ascontiguousarray(X, dtype=np.float32)
    M = X.shape[0]
    y = np.full((M, N), np.nan, dtype=np.float32)
    rc = L.clip_amd_test_gemm_panel(tid, _vp(raw), _vp(raw2), N, K, _fp(X), M, _fp(bias), _fp(resid), _fp(y), epi, tile, qcols, qscale, panel_mode, lead)
    return rc, y


def run_gemm_panel(L, *a, what="", **kw):
    """rc == 0 (no guard row changed) and every element written"""
    rc, y = call_gemm_panel(L, *a, **kw)
    assert rc == 0, (what, "clip_amd_test_gemm_panel rc=%d" % rc)
    bad = np.argwhere(~np.isfinite(y))
    assert bad.size == 0, "%s: %d/%d elements not finite / not written, first %s" % (what, len(bad), y.size, bad[0].tolist())
    return y


def call_fold(L, tid, raw, N, K, gamma, beta, bias):
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    gamma, beta, bias = f(gamma), f(beta), f(bias)
    c, b = np.full(N, np.nan, dtype=np.float32), np.full(N, np.nan, dtype=np.float32)
    rc = L.clip_amd_test_fold_vectors(tid, _vp(raw), N, K, _fp(gamma), _fp(beta), _fp(bias), _fp(c), _fp(b))
    return rc, c, b


def run_fold(L, *a, what=""):
    rc, c, b = call_fold(L, *a)
    assert rc == 0, (what, "clip_amd_test_fold_vectors rc=%d" % rc)          # -6: one of the 64 floats behind c or b' changed
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(b)), (what, "an element of c or b' was not written")
    return c, b


# --------------------------------------------------------------------------------------------------------------------------------
# pre-built panel: two exact_case weights of one type and shape
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def panel_case(tname, M, N, K):
    """-> (c, raw2, W2): an exact_case and a second weight from another seed (raw bytes, float64 values), within the same budget"""
    xmax = min(16, ge.xmax_for(tname, K))
    c = ge.exact_case(np.random.default_rng(seed("panel", tname, M, N, K)), tname, M, N, K, xmax)
    c2 = ge.exact_case(np.random.default_rng(seed("planes", tname, M, N, K)), tname, 1, N, K, xmax)
    for a in (c.raw, c.W, c.X, c.bias, c.resid, c.acc, c2.raw, c2.W):
        a.setflags(write=False)
    return c, c2.raw, c2.W


def other_want(c, W2, epi, qcols=0):
    """what a launch that multiplied the planes of the second weight would return"""
    o = ge.ExactCase(**dict(c.__dict__))
    o.acc = np.rint(c.X.astype(np.float64)).astype(np.int64) @ np.rint(W2 * ge.UNIT).astype(np.int64).T
    return o.want(epi, qcols=qcols)


# --------------------------------------------------------------------------------------------------------------------------------
# fold vectors
# --------------------------------------------------------------------------------------------------------------------------------
class FoldExact:
    """raw, W float64 [N][K]; gamma, beta f32 [K], bias f32 [N]; c_i, b_i, bias_i: int64 in units of 2^-14"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def want(self, with_bias):
        """(c, b') as the f32 the kernel must store: one rounding of the exact sum"""
        b = self.b_i + (self.bias_i if with_bias else 0)
        for v in (self.c_i, b):
            assert np.abs(v).max() < 2 ** 53                               # float64 holds the integer; the division by 2^14 is exact
        return (self.c_i.astype(np.float64) / FUNIT).astype(np.float32), (b.astype(np.float64) / FUNIT).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fold_exact(tname, N, K, gmax=2 * GUNIT):
    """weights from exact_case (K % 32 != 0, f16 only: drawn by the same rule, multiples of 2^-6 with |w| <= 4); gamma, beta = i / 256 with
    |i| <= gmax (default 512: |.| <= 2), bias multiples of 2^-6 with |.| <= 4"""
    rng = np.random.default_rng(seed("fold", tname, N, K, gmax))
    if K % 32 == 0:
        c = ge.exact_case(rng, tname, 1, N, K, 1)
        raw, W = c.raw, c.W
    else:
        assert tname == "f16"
        raw = (rng.integers(-4 * ge.UNIT, 4 * ge.UNIT + 1, size=(N, K)) / ge.UNIT).astype(np.float16).view(np.uint8).reshape(N, -1)
        W = ge.dequant_exact(tname, raw, N, K)
    Wi = np.rint(W * ge.UNIT).astype(np.int64)
    assert np.array_equal(Wi, W * ge.UNIT)
    g_i, be_i = rng.integers(-gmax, gmax + 1, size=K), rng.integers(-gmax, gmax + 1, size=K)
    bias_u = rng.integers(-4 * ge.UNIT, 4 * ge.UNIT + 1, size=N)
    f = FoldExact(tname=tname, tid=ref.GGML_TYPES[tname], N=N, K=K, raw=np.ascontiguousarray(raw), W=W, gamma=(g_i / GUNIT).astype(np.float32),
                  beta=(be_i / GUNIT).astype(np.float32), bias=(bias_u / ge.UNIT).astype(np.float32), c_i=Wi @ g_i, b_i=Wi @ be_i, bias_i=bias_u * GUNIT)
    assert np.array_equal(f.gamma.astype(np.float64) * GUNIT, g_i) and np.array_equal(f.beta.astype(np.float64) * GUNIT, be_i)
    assert np.array_equal(f.bias.astype(np.float64) * ge.UNIT, bias_u)
    for a in (f.raw, f.W, f.gamma, f.beta, f.bias, f.c_i, f.b_i, f.bias_i):
        a.setflags(write=False)
    return f


def fold_partial_sums_exact(f):
    """in units of 2^-14 every product gamma w, beta w and the bias are integers, and the sum of their magnitudes over a row stays below 2^53: every
    partial sum, in any order, is an integer that float64 holds — the kernel's double accumulator never rounds"""
    Wi = np.rint(np.abs(f.W) * ge.UNIT).astype(np.int64)
    g_i, be_i = np.rint(np.abs(f.gamma).astype(np.float64) * GUNIT).astype(np.int64), np.rint(np.abs(f.beta).astype(np.float64) * GUNIT).astype(np.int64)
    worst = max((Wi @ g_i).max(), (Wi @ be_i + np.abs(f.bias_i)).max())
    return int(worst) < 2 ** 53


class FoldReal:
    """quantised _weights, gamma = 1 + 0.2 N(0, 1), beta = 0.1 N(0, 1) (as _lnfold_case draws them), bias 0.1 N(0, 1); float64 references and bounds"""

    def __init__(self, tname, N, K):
        rng = np.random.default_rng(seed("foldreal", tname, N, K))
        self.tid = ref.GGML_TYPES[tname]
        Wf = _weights(rng, N, K)
        self.raw = Wf.astype(np.float16).view(np.uint8).reshape(N, -1) if tname == "f16" else ref.quantize(self.tid, Wf).reshape(N, -1)
        self.raw = np.ascontiguousarray(self.raw)
        self.W = ge.dequant_fp16(tname, self.raw, N, K).astype(np.float64)        # the kernel's weight: the exact value rounded once to fp16
        self.gamma = (1 + rng.standard_normal(K) * 0.2).astype(np.float32)
        self.beta = (rng.standard_normal(K) * 0.1).astype(np.float32)
        self.bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        g, be, bi = self.gamma.astype(np.float64), self.beta.astype(np.float64), self.bias.astype(np.float64)
        self.c64, self.mag_c = self.W @ g, np.abs(self.W) @ np.abs(g)
        self.b64 = {False: self.W @ be, True: self.W @ be + bi}
        self.mag_b = {False: np.abs(self.W) @ np.abs(be), True: np.abs(self.W) @ np.abs(be) + np.abs(bi)}
        self.K = K


@functools.lru_cache(maxsize=None)
def fold_real(tname, N, K):
    return FoldReal(tname, N, K)


def fold_bound(want64, mag, K):
    """|c - c64| <= 2^-24 |c64| + 2^-149 (one rounding to f32, gradual underflow) + K 2^-51 sum_k |gamma_k w_nk| (sequential double summation in the
    kernel against numpy's pairwise / blocked one: (K - 1) 2^-53 of the magnitude each, to first order; K 2^-51 is four times their sum)"""
    return 2.0 ** -24 * np.abs(want64) + 2.0 ** -149 + K * 2.0 ** -51 * mag
