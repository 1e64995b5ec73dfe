"""Shared by test_gemm_exact_cpu.py and test_gpu_gemm_exact.py: what the fp16-activation GEMM kernels multiply, known exactly.

dequant_fp16   the weight operand of every kernel (gemm_common.h dequant_wpair): (q - zero) d or fma(q, d, m) in packed fp16, ONE rounding — the exact
               value, then one astype(float16).  float16(that) == float16(ggml's f32 weight) bit for bit (test_gemm_exact_cpu.py).
exact_case     operands for which every f32 partial sum of X W^T (+ bias, + resid) is exact in ANY order: the expectation is integer arithmetic and
               a kernel is held to it without a tolerance, whatever its MFMA shape, K split or summation order.
act_bound      the bound on an activation epilogue's fp16 output for an f32 argument x that numpy knows exactly.
"""
import numpy as np

from oracle import ref
from test_gpu_entry_kernels import BLOCK_BYTES, np_dequant, raw_table
from test_gpu_gemm_f32 import ACT_C

QTYPES = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
WTYPES = ["f16"] + QTYPES
UNIT = 64                      # exact_case: every weight, bias and residual value is a multiple of 2^-6
QSCALE = 0.125                 # ... and the Q scale a power of two: the scaled columns are multiples of 2^-9
BUDGET = 2 ** 23               # |any partial sum| in units of 2^-6 (2^-9 on the scaled columns)
# the largest |weight| exact_case can produce: |q - zero| 2^-3, or q 2^-3 + 2 with an offset; f16: 4
W_MAX = {"f16": 4.0, "q4_0": 1.0, "q4_1": 15 / 8 + 2, "q5_0": 2.0, "q5_1": 31 / 8 + 2, "q8_0": 16.0}


def _has_m(tname):
    return tname in ("q4_1", "q5_1")


def _blocks(tname, raw, N, K):
    return np.ascontiguousarray(raw, dtype=np.uint8).reshape(N, K // 32, BLOCK_BYTES[tname])


def _f16_field(blk, o):
    return np.ascontiguousarray(blk[:, :, o:o + 2]).view(np.float16).astype(np.float64)            # [N][nb][1]


def dequant_exact(tname, raw, N, K):
    """the real number the kernel rounds: float64 holds it exactly (an 8-bit code times an 11-bit scale, plus an 11-bit offset, all within 2^-24 .. 2^16).
    The codes come from np_dequant on the same blocks with d = 1 and m = 0 (small integers: exact in its f32), so the block layout is stated once."""
    if tname == "f16":
        return np.ascontiguousarray(raw, dtype=np.uint8).view(np.float16).reshape(N, K).astype(np.float64)
    blk = _blocks(tname, raw, N, K)
    unit = blk.copy()
    unit[:, :, 0:2] = np.array([1.0], dtype=np.float16).view(np.uint8)
    if _has_m(tname):
        unit[:, :, 2:4] = 0
    q = np_dequant(tname, unit.reshape(N, -1), N, K).astype(np.float64).reshape(N, K // 32, 32)      # q - zero, or q
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 128
    w = q * _f16_field(blk, 0)
    if _has_m(tname):
        w = w + _f16_field(blk, 2)
    return w.reshape(N, K)


def dequant_fp16(tname, raw, N, K):
    """-> float16 [N][K]: the kernel's weight operand."""
    with np.errstate(over="ignore"):
        return dequant_exact(tname, raw, N, K).astype(np.float16)


def xmax_for(tname, K):
    """the largest |x| the budget of exact_case admits at this K"""
    return int(BUDGET // (K * UNIT * W_MAX[tname]))


class ExactCase:
    """raw: the weight in its ggml layout; W float64 [N][K], X f32 integers [M][K], bias f32 [N], resid f32 [M][N];
    acc, bias_i, resid_i: int64 in units of 2^-6."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def want(self, epi, bias=True, qcols=0):
        """the exact result as the f32 the hook returns: epilogue 0 acc + bias, 4 resid + (acc + bias), 1 float16((acc + bias) q)"""
        lin = self.acc + (self.bias_i if bias else 0)
        if epi == 4:
            lin = lin + self.resid_i
        assert np.abs(lin).max() < 2 ** 24
        out = lin.astype(np.float64) / UNIT
        if epi == 1:
            out[:, :qcols] *= QSCALE
            with np.errstate(over="ignore"):
                return out.astype(np.float16).astype(np.float32)
        assert epi in (0, 4)
        return out.astype(np.float32)


def exact_case(rng, tname, M, N, K, xmax):
    """Block scales d = +-2^-e, e in 3 .. 6 per block, offsets m multiples of 2^-6 with |m| <= 2, every code and qh bit from random bytes; f16 weights
    multiples of 2^-6 with |w| <= 4; X integers in [-xmax, xmax]; bias, resid multiples of 2^-6 with |.| <= 4.  Every product and every sum of them is
    a multiple of 2^-6 below 2^23 2^-6 in magnitude: an f32 holds each partial sum exactly, in any order, and so it does the sums with bias and resid."""
    assert K % 32 == 0 and xmax >= 1
    assert K * xmax * W_MAX[tname] * UNIT <= BUDGET, "budget: K xmax max|w| 2^6 = %g > 2^23" % (K * xmax * W_MAX[tname] * UNIT)
    assert (K * xmax * W_MAX[tname] + 4) * QSCALE * (8 * UNIT) < 2 * BUDGET, "budget of the scaled columns, bias included, in units of 2^-9"
    assert (K * xmax * W_MAX[tname] + 8) * UNIT < 2 * BUDGET, "with bias and resid (|.| <= 4 each) every sum stays below 2^24 units"
    if tname == "f16":
        raw = (rng.integers(-4 * UNIT, 4 * UNIT + 1, size=(N, K)) / UNIT).astype(np.float16).view(np.uint8).reshape(N, -1)
    else:
        raw = raw_table(rng, tname, N, K)
        blk = _blocks(tname, raw, N, K)
        nb = K // 32
        d = (rng.choice([-1.0, 1.0], size=(N, nb)) * 2.0 ** -rng.integers(3, 7, size=(N, nb))).astype(np.float16)
        blk[:, :, 0:2] = d.view(np.uint8).reshape(N, nb, 2)
        if _has_m(tname):
            m = (rng.integers(-2 * UNIT, 2 * UNIT + 1, size=(N, nb)) / UNIT).astype(np.float16)
            blk[:, :, 2:4] = m.view(np.uint8).reshape(N, nb, 2)
        raw = blk.reshape(N, -1)
    W = dequant_exact(tname, raw, N, K)
    assert np.array_equal(dequant_fp16(tname, raw, N, K).astype(np.float64), W), "every weight is an fp16 number"
    Wi = np.rint(W * UNIT).astype(np.int64)
    assert np.array_equal(Wi, W * UNIT) and np.abs(W).max() <= W_MAX[tname]
    Xi = rng.integers(-xmax, xmax + 1, size=(M, K)).astype(np.int64)
    bias_i = rng.integers(-4 * UNIT, 4 * UNIT + 1, size=N).astype(np.int64)
    resid_i = rng.integers(-4 * UNIT, 4 * UNIT + 1, size=(M, N)).astype(np.int64)
    acc = Xi @ Wi.T
    return ExactCase(tname=tname, tid=ref.GGML_TYPES[tname], M=M, N=N, K=K, raw=np.ascontiguousarray(raw), W=W, X=Xi.astype(np.float32),
                     bias=(bias_i / UNIT).astype(np.float32), resid=(resid_i / UNIT).astype(np.float32), acc=acc, bias_i=bias_i, resid_i=resid_i)


def act_bound(g, x):
    """|y - g| for y = the fp16 output of an activation epilogue, g = its float64 value at the f32 argument x: the f32 evaluation stays within
    delta = ACT_C 2^-23 |x| + 2^-126 of g (test_gpu_gemm_f32.py derives ACT_C from gemm_common.h's gelu_tanh / gelu_quick), and y is that value rounded
    to nearest fp16 with gradual underflow: half an ulp <= 2^-11 of its magnitude, and 2^-25 below the normal range."""
    g, x = np.abs(np.asarray(g, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64))
    delta = ACT_C * 2.0 ** -23 * x + 2.0 ** -126
    return np.maximum(2.0 ** -11 * (g + delta), 2.0 ** -25) + delta
