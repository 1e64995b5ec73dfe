"""GPU tier, kernel level: the weight GEMM of an f32 GGUF file (k_gemm_f32.hip) in the form the layers run it since round 6 —
gemm_f32_kernel<EPI, AF32 = true>: f32 activation rows behind the half_t pointer, epilogue_f32_out (f32 stores) in place of the three
fp16-output epilogues — through clip_amd_test_gemm_f32, next to the fp16-activation form (AF32 = false) on the same operands.

Shapes: the tile is 64 weight rows x 64 activation rows, a wave covers 16 weight rows, a K step is 16 wide with the next step prefetched.
M in {1, 63, 64, 65, 130} (row clamp to M - 1, a second row tile), N in {64, 68, 80, 192} (68: a wave whose first column group is valid and the
rest is not; 80: a wave wholly past N), K in {64, 80, 128, 192, 588} (4 .. 40 steps; 80 and 588 with zero weight padding), and one K = 4096.
Every call carries two guard rows behind the output, filled with a sentinel like the rest of y: run_gemm_f32 asserts they come back bit for bit.

Measured on an MI355X (printed by the cases, -s shows them):
    epilogues 0 / 1 / 4 and the f32 patch embedding, max |y - want| / (2e-6 mag + 1e-7):          0.19 (K = 4096: 0.10)
    epilogues 2 / 3, c = max (|y - want| - 1.13 (2e-6 mag + 1e-7)) / (2^-23 |lin|):                -19.1 (negative everywhere: GELU_C below)
    epilogues 2 / 3, the activation alone, max |y - gelu64(y of epilogue 0)| / (2^-23 |y0|):      0.91 tanh form, 1.06 quick form (ACT_C below)
    one layer, max over rows of |gpu - f64|_inf / |np32 - f64|_inf:                                1.90 full, 1.77 causal (LAYER_R below)
    fp16(f32 form) against the fp16 form: equal except at fp16 ties of the f32 value, about one output in 16 000 (fp16_of_f32_form_matches)

That the cases bite was checked once with mutations of k_gemm_f32.hip (never committed), of the 79 cases here:
    the Q scale withheld from the last group of 4 Q columns (`n < qcols - 4`)          14 fail (q-scale, bitwise, both layer cases)
    both GELUs returning 0 for negative arguments                                      24 fail
    the AF32 prefetch re-reading step nk - 2 in place of nk - 1                        39 fail: every K that is a multiple of 64; at K = 80 and 588 the last
                                                                                       step is zero padding on both operands and the re-read cannot show
A store one column group past N was not run on a GPU: it writes into the next row and, from the last row, into the guard rows, which every call checks.
"""
import functools
import itertools

import numpy as np
import pytest

import attention_common as ac
import gemm_f32_common as gc
from test_gpu_kernels import L, _weights, gelu_quick, gelu_tanh  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

MS = [1, 63, 64, 65, 130]
NS = [64, 68, 80, 192]
KS = [64, 80, 128, 192, 588]
LONG = (65, 64, 4096)
MN = list(itertools.product(MS, NS))
TAILS = np.array([-12.0, -8.0, -5.0, -3.0, -1.5, 3.0, 8.0], dtype=np.float32)     # added to the bias of 7 columns: lin from about -12 to +8
GELU = {2: gelu_tanh, 3: gelu_quick}
# epilogues 2 / 3: tolerance 1.13 (2e-6 mag + 1e-7) + GELU_C 2^-23 |lin|.  The measured value (module docstring) is NEGATIVE: mag >= |lin|, so the first
# term alone is >= 19 x 2^-23 |lin| while the kernel's whole error stays below a tenth of it; twice a negative value rounded up gives no positive
# integer, so the second term is 0 and what holds the activation's own f32 evaluation is ACT_C below.
GELU_C = 0
# The activation alone: y against the float64 GELU of the f32 value it was applied to (y of epilogue 0: the same acc + bias, bit for bit), in
# units of 2^-23 |x|.  From the code (gemm_common.h), u = 2^-24, e = exp2(arg), t = 1 / (e + 1), result x - x t (tanh form) or x t (quick form):
#   arg: the folded constants carry <= 5 u (three float factors and two products), x^2, the FMA and the product one u each: <= 8 u |arg|
#        (quick form: constant 3 u, product u: 4 u |arg|); v_exp_f32 adds 1 ulp <= 2 u: rel(e) <= 8 u ln2 |arg| + 2 u
#   dt = t (1 - t) rel(e), and t (1 - t) |log2 e| <= 0.323 (at e = 2^2.2), t (1 - t) <= 1/4:  <= (1.8 + 0.5) u;  e + 1: u t;  v_rcp_f32 1 ulp: 2 u t
#   the last FMA / product: u |result| <= u |x|.   Sum <= 6.3 u |x| = 3.2 x 2^-23 |x| (quick form 5.4 u)  ->  4, plus one subnormal for a flushed e.
ACT_C = 4.0
LAYER_R = 3.9             # one layer: |gpu - f64| <= LAYER_R |np32 - f64| + 1e-6 per row: twice the measured 1.90 (an interface error costs >= 100)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class Case:
    """One (M, N, K): f32 operands and their float64 product, computed once and shared read-only by every test."""

    def __init__(self, M, N, K):
        rng = np.random.default_rng(M * 1000003 + N * 1009 + K)
        W = _weights(rng, N, K)
        X = rng.standard_normal((M, K)).astype(np.float32)          # not fp16-representable
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        bias[np.linspace(0, N - 1, len(TAILS)).astype(int)] += TAILS     # first and last column included
        resid = rng.standard_normal((M, N)).astype(np.float32)
        self.M, self.N, self.K = M, N, K
        self.W, self.X, self.bias, self.resid = _frozen(W, X, bias, resid)
        W64, X64 = W.astype(np.float64), X.astype(np.float64)
        self.dot, self.absdot = _frozen(X64 @ W64.T, np.abs(X64) @ np.abs(W64).T)
        self.lin, self.mag = _frozen(self.dot + bias, self.absdot + np.abs(bias))
        self.what = "M=%d N=%d K=%d" % (M, N, K)


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    return Case(M, N, K)


def shapes(K):
    return [LONG[:2]] if K == LONG[2] else MN


def lin_bound(mag):
    """the project's bound on this kernel's f32 accumulation (test_f32_weights_are_multiplied_in_f32): no fp16 term"""
    return 2e-6 * mag + 1e-7


def assert_within(y, want, bound, what):
    assert np.all(np.isfinite(y)), (what, "not finite / not written", int((~np.isfinite(y)).sum()))
    ratio = np.abs(y - want) / bound
    bad = np.argwhere(ratio > 1.0)
    assert bad.size == 0, "%s: %d/%d outside, first %s got %r want %r; max err / bound %g" % (
        what, len(bad), y.size, bad[0].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])]), ratio.max())
    return float(ratio.max())


def bits(y):
    return np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------------------
# 1. against float64
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS + [LONG[2]])
@pytest.mark.parametrize("epi", [0, 4])
def test_f32_activations_vs_float64_f32_epilogues(L, epi, K):
    """epilogue 0 (plain) and 4 (residual, in place): |y - want| <= 2e-6 mag + 1e-7 with |resid| inside mag for 4."""
    worst = 0.0
    for M, N in shapes(K):
        c = case(M, N, K)
        y = gc.run_gemm_f32(L, c.W, c.X, c.what, bias=c.bias, resid=c.resid if epi == 4 else None, epi=epi)
        want, mag = (c.lin + c.resid, c.mag + np.abs(c.resid)) if epi == 4 else (c.lin, c.mag)
        worst = max(worst, assert_within(y, want, lin_bound(mag), "epilogue %d %s" % (epi, c.what)))
    print("gemm_f32 act_f32 epilogue %d K %4d: max err / (2e-6 mag + 1e-7) = %.4f" % (epi, K, worst))


@pytest.mark.parametrize("K", KS + [LONG[2]])
def test_f32_activations_vs_float64_q_scale(L, K):
    """epilogue 1: (acc + bias) qscale on the columns below qcols — the scale AFTER the bias — stored as f32.  qcols in {0, 64, 100}: 64 of N = 192 is
    the q/k/v layout, 64 of N = 68 / 80 leaves the last column group(s) unscaled, 100 splits a wave's 16 columns between two groups of 4.  want and
    the bound are scaled on the Q columns; the columns on both sides of the boundary are asserted on their own."""
    worst = 0.0
    for M, N in shapes(K):
        c = case(M, N, K)
        for qcols, qscale in ((0, 1.0), (64, 0.125), (100, 0.3)):
            if qcols > N:
                continue
            what = "epilogue 1 qcols %d %s" % (qcols, c.what)
            y = gc.run_gemm_f32(L, c.W, c.X, what, bias=c.bias, epi=1, qcols=qcols, qscale=qscale)
            scale = np.ones(N)
            scale[:qcols] = np.float32(qscale)
            want, bound = c.lin * scale, lin_bound(c.mag) * scale
            worst = max(worst, assert_within(y, want, bound, what))
            for col in (qcols - 1, qcols):
                if 0 <= col < N and qcols:
                    assert_within(y[:, col], want[:, col], bound[:, col], what + " column %d" % col)
    print("gemm_f32 act_f32 epilogue 1 K %4d: max err / (2e-6 mag + 1e-7) = %.4f" % (K, worst))


def test_f32_activations_without_bias(L):
    """the projection has no bias: epilogue 0 and 1 with bias = NULL"""
    for M, N, K in ((65, 68, 80), (130, 192, 588)):
        c = case(M, N, K)
        for epi in (0, 1):
            y = gc.run_gemm_f32(L, c.W, c.X, c.what, bias=None, epi=epi)
            assert_within(y, c.dot, lin_bound(c.absdot), "epilogue %d without bias %s" % (epi, c.what))


@pytest.mark.parametrize("K", KS + [LONG[2]])
@pytest.mark.parametrize("epi", [2, 3])
def test_f32_activations_vs_float64_gelu(L, epi, K):
    """epilogues 2 (tanh GELU) and 3 (quick GELU) stored as f32, against the float64 GELU of the float64 lin: the GEMM error through a 1.13-Lipschitz
    function plus GELU_C 2^-23 |lin|; and the activation alone against the float64 GELU of the very f32 value it was applied to, within
    ACT_C 2^-23 |x| (both constants: top of the module).  The bias puts lin between about -12 and +8 on 7 columns: the negative tail, where
    x - x t cancels, and the flushed exponentials are inside."""
    worst_c, worst_act = -np.inf, 0.0
    for M, N in shapes(K):
        c = case(M, N, K)
        what = "epilogue %d %s" % (epi, c.what)
        y = gc.run_gemm_f32(L, c.W, c.X, what, bias=c.bias, epi=epi)
        want = GELU[epi](c.lin)
        first, unit = 1.13 * lin_bound(c.mag), 2.0 ** -23 * np.abs(c.lin)
        assert c.lin.min() < -9.0 and c.lin.max() > 5.0, what
        worst_c = max(worst_c, float(((np.abs(y - want) - first) / unit).max()))
        assert_within(y, want, first + GELU_C * unit, what)
        y0 = gc.run_gemm_f32(L, c.W, c.X, what, bias=c.bias, epi=0)
        worst_act = max(worst_act, assert_within(y, GELU[epi](y0), ACT_C * 2.0 ** -23 * np.abs(y0.astype(np.float64)) + 2.0 ** -126, what + " activation alone"))
    print("gemm_f32 act_f32 epilogue %d K %4d: c = %.3f; activation alone %.3f x 2^-23 |x|" % (epi, K, worst_c, worst_act * ACT_C))


# --------------------------------------------------------------------------------------------------------------------------------
# 2. the two instantiations
# --------------------------------------------------------------------------------------------------------------------------------
def fp16_of_f32_form_matches(y32, y16):
    """-> (mask of elements where the fp16 form's output is NOT what the f32 form's value allows, number of ties taken the other way).
    The fp16 form of epilogue 1 rounds ONCE: hipcc fuses the epilogue's last FMA and the conversion into v_fma_mixlo_f16 (gemm_common.h, at
    gelu_tanh, describes the same fusion), so y16 = fp16(acc q + bias q) while the f32 form stores f32(acc q + bias q).  Rounding a real number to
    f32 and then to fp16 differs from rounding it to fp16 at once only where the f32 value is exactly the midpoint of two fp16 neighbours (else
    both lie on the same side of every midpoint): there either neighbour is right, everywhere else y16 must be fp16(y32) to the bit.  No tolerance."""
    y32 = np.asarray(y32, dtype=np.float32)
    near = y32.astype(np.float16)                                             # round to nearest even
    d = y32.astype(np.float64) - near.astype(np.float64)
    other = np.nextafter(near, np.where(d > 0, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    tie = (d != 0) & (2 * np.abs(d) == np.abs(other.astype(np.float64) - near.astype(np.float64)))
    got = np.asarray(y16, dtype=np.float32).astype(np.float16).view(np.uint16)
    same, away = got == near.view(np.uint16), tie & (got == other.view(np.uint16))
    return ~(same | away), int(away.sum())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_f32_and_fp16_activation_forms_agree_bitwise(L, epi, K):
    """X holds fp16 values: widening them is exact and both forms run the same MFMA sequence, so AF32 = true (f32 rows, f4 loads) and AF32 = false
    (fp16 rows, 8-byte loads) must give the same accumulators — an offset, stride or clamp error in either set of loads breaks it.  Epilogues 0 and 4
    store those f32 values: equal bits.  Epilogues 2 and 3: the f32 form stores the value the fp16 form rounds, fp16(y_f32) has the bits of y_f16.
    Epilogue 1: the same except at fp16 ties of the f32 value, where the fp16 form, which rounds once, may take either neighbour
    (fp16_of_f32_form_matches; found by this test: 1 to 5 outputs per K).  The Q scale here is a power of two: then (acc + bias) q of epilogue_f32_out
    (two operations, as the reference scales) and fma(acc, q, bias q) of gemm_epilogue round the same real number; for any other scale see
    test_q_scale_forms_differ_by_their_roundings_only."""
    ties = 0
    for M, N in MN:
        c = case(M, N, K)
        Xh = c.X.astype(np.float16).astype(np.float32)
        kw = dict(bias=c.bias, resid=c.resid if epi == 4 else None, epi=epi, qcols=64 if epi == 1 else 0, qscale=0.125 if epi == 1 else 1.0)
        what = "epilogue %d %s" % (epi, c.what)
        y32 = gc.run_gemm_f32(L, c.W, Xh, what, act_f32=1, **kw)
        y16 = gc.run_gemm_f32(L, c.W, Xh, what, act_f32=0, **kw)
        assert np.all(np.isfinite(y32)) and np.all(np.isfinite(y16)), what
        if epi in (0, 4):
            diff = bits(y32) != bits(y16)
        elif epi == 1:
            diff, away = fp16_of_f32_form_matches(y32, y16)
            ties += away
        else:
            diff = y32.astype(np.float16).view(np.uint16) != y16.astype(np.float16).view(np.uint16)
        assert not diff.any(), "%s: %d elements differ, first %s: f32 activations %r, fp16 activations %r" % (
            what, int(diff.sum()), np.argwhere(diff)[0].tolist(), float(y32[tuple(np.argwhere(diff)[0])]), float(y16[tuple(np.argwhere(diff)[0])]))
    if epi == 1:
        print("gemm_f32 epilogue 1 K %4d: %d fp16 ties of the f32 value rounded the other way by the fp16 form" % (K, ties))


def test_q_scale_forms_differ_by_their_roundings_only(L):
    """A Q scale that is no power of two (1 / sqrt(32): head size 32): epilogue_f32_out computes round(round(acc + bias) q) as the reference does
    (ggml_scale after the add, clip.cpp:1363), gemm_epilogue fma(acc, q, round(bias q)).  Both are within 2^-24 (|result| + |acc| q + |bias| q) of
    (acc + bias) q, so the fp16 the second one stores is within half an fp16 ulp of itself (2^-11 |y16|, 2^-25 below the normal range) plus
    2^-22 mag q of the f32 the first one stores; the unscaled columns agree as above."""
    q = float(np.float32(1.0 / np.sqrt(32.0)))
    for M, N, K in ((65, 192, 80), (130, 68, 588)):
        c = case(M, N, K)
        Xh = c.X.astype(np.float16).astype(np.float32)
        kw = dict(bias=c.bias, epi=1, qcols=64, qscale=q)
        y32 = gc.run_gemm_f32(L, c.W, Xh, c.what, act_f32=1, **kw)
        y16 = gc.run_gemm_f32(L, c.W, Xh, c.what, act_f32=0, **kw)
        mag = np.abs(Xh).astype(np.float64) @ np.abs(c.W).astype(np.float64).T + np.abs(c.bias)
        assert_within(y16[:, :64], y32[:, :64].astype(np.float64), 2.0 ** -11 * np.abs(y16[:, :64]) + 2.0 ** -25 + 2.0 ** -22 * mag[:, :64] * q, "Q columns " + c.what)
        assert not fp16_of_f32_form_matches(y32[:, 64:], y16[:, 64:])[0].any(), c.what


# --------------------------------------------------------------------------------------------------------------------------------
# 3. exact selection
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 80, 192])
def test_one_hot_operands_select_exactly(L, K):
    """A one-hot operand turns the product into a copy: every other term is an exact zero, so the f32 result equals the selected element of the
    other operand bit for bit.  X one-hot (row m has 1.0 at k = m, M = K): y[m][n] == W[n][m]; W one-hot (row n has 1.0 at k = n mod K): y[m][n] ==
    X[m][n mod K].  Every k of every 16-wide step is selected once — the last step, which the prefetch clamp re-reads, and the steps next to the
    zero padding (K = 80 -> Kpad 128) included; a step read twice, skipped, or taken from the neighbouring row shows as a wrong or doubled value."""
    rng = np.random.default_rng(K)
    for N in (68, 192):
        W = _weights(rng, N, K)
        y = gc.run_gemm_f32(L, W, np.eye(K, dtype=np.float32), "X one-hot N=%d K=%d" % (N, K), epi=0)
        bad = np.argwhere(bits(y) != bits(W.T))
        assert bad.size == 0, "X one-hot N=%d K=%d: %d elements differ, first (m, n) = %s" % (N, K, len(bad), bad[0].tolist())
    for M in (65, 130):
        N = 192
        X = rng.standard_normal((M, K)).astype(np.float32)
        W = np.zeros((N, K), dtype=np.float32)
        W[np.arange(N), np.arange(N) % K] = 1.0
        y = gc.run_gemm_f32(L, W, X, "W one-hot M=%d K=%d" % (M, K), epi=0)
        bad = np.argwhere(bits(y) != bits(X[:, np.arange(N) % K]))
        assert bad.size == 0, "W one-hot M=%d K=%d: %d elements differ, first (m, n) = %s" % (M, K, len(bad), bad[0].tolist())


# --------------------------------------------------------------------------------------------------------------------------------
# 4. stores stay inside
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_f32", [1, 0])
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_stores_stay_inside_the_output(L, epi, act_f32):
    """Two guard rows behind y, sentinel-filled like y itself: for every epilogue and every (M, N) the rows >= M keep the sentinel (run_gemm_f32
    asserts it — a store one row or one column group too far lands there or in the next row's first columns) and all of [0, M) x [0, N) was
    written with finite values, none of them the fill."""
    K = 80
    for M, N in MN:
        c = case(M, N, K)
        what = "epilogue %d act_f32 %d %s" % (epi, act_f32, c.what)
        y = gc.run_gemm_f32(L, c.W, c.X, what, bias=c.bias, resid=c.resid if epi == 4 else None, epi=epi, qcols=64 if epi == 1 else 0, qscale=0.125,
                            act_f32=act_f32)
        assert y.shape == (M, N) and np.all(np.isfinite(y)), what
        assert not np.any(bits(y) == gc.SENTINEL_BITS), (what, "an element of y was not written")


# --------------------------------------------------------------------------------------------------------------------------------
# 5. f32 patch embedding
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,G,h,P", [(3, 7, 64, 14), (2, 4, 192, 8)])
def test_f32_patch_embedding(L, B, G, h, P):
    """The loader admits an f32 v.patch_embd.weight: W_F32, gemm_f32_kernel<EPI_PATCH_F32, false> on the fp16 im2col rows at K = 3 P^2
    (P = 14: K = 588 -> Kpad 640).  GEMM row m = (image, patch) lands in token row image T + 1 + patch with position_embd[1 + patch] added, no
    bias; the class-token rows and the guard rows keep the fill; the rest is within 2e-6 mag + 1e-7 of fp16(X) W^T + pos in float64."""
    rng = np.random.default_rng(B * 100 + G)
    Np, T, K = G * G, G * G + 1, 3 * P * P
    W = (rng.standard_normal((h, K)) * 0.02).astype(np.float32)
    X = rng.standard_normal((B * Np, K)).astype(np.float32)
    pos = (rng.standard_normal((T, h)) * 0.02).astype(np.float32)
    what = "patch embedding B=%d G=%d h=%d P=%d" % (B, G, h, P)
    y = gc.run_gemm_f32(L, W, X, what, epi=5, Np=Np, T=T, pos=pos, act_f32=0)
    y3 = y.reshape(B, T, h)
    assert np.all(bits(y3[:, 0, :]) == gc.SENTINEL_BITS), (what, "class rows written")
    Xh = X.astype(np.float16).astype(np.float64)
    W64 = W.astype(np.float64)
    want = (Xh @ W64.T).reshape(B, Np, h) + pos[None, 1:, :]
    mag = (np.abs(Xh) @ np.abs(W64).T).reshape(B, Np, h) + np.abs(pos[None, 1:, :])
    r = assert_within(y3[:, 1:, :], want, lin_bound(mag), what)
    print("gemm_f32 %s: max err / (2e-6 mag + 1e-7) = %.4f" % (what, r))
    rc, again = gc.call_gemm_f32(L, W, X, epi=5, Np=Np, T=T, pos=pos, act_f32=0)
    assert rc == 0 and np.array_equal(bits(again[:B * T]), bits(y)), (what, "second run differs")


# --------------------------------------------------------------------------------------------------------------------------------
# 6. determinism
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_f32_activations_same_bits_run_to_run(L, epi):
    c = case(130, 192, 588)
    kw = dict(bias=c.bias, resid=c.resid if epi == 4 else None, epi=epi, qcols=64 if epi == 1 else 0, qscale=0.3)
    first = gc.run_gemm_f32(L, c.W, c.X, c.what, **kw)
    for _ in range(3):
        assert np.array_equal(bits(gc.run_gemm_f32(L, c.W, c.X, c.what, **kw)), bits(first)), "epilogue %d %s: a second run differs" % (epi, c.what)


# --------------------------------------------------------------------------------------------------------------------------------
# One f32 layer composed from the hooks
# --------------------------------------------------------------------------------------------------------------------------------
H, HEADS, FF, EPS = 64, 2, 128, 1e-5
LENS = (1, 5, 17, 33)


def _layer_params():
    rng = np.random.default_rng(20)
    n = lambda *s: rng.standard_normal(s)
    P = dict(ln1_w=1 + 0.1 * n(H), ln1_b=0.1 * n(H), wqkv=n(3 * H, H) / np.sqrt(H), bqkv=0.1 * n(3 * H), wo=n(H, H) / np.sqrt(H), bo=0.1 * n(H),
             ln2_w=1 + 0.1 * n(H), ln2_b=0.1 * n(H), w1=n(FF, H) / np.sqrt(H), b1=0.1 * n(FF), w2=n(H, FF) / np.sqrt(FF), b2=0.1 * n(H),
             x=n(sum(LENS), H))
    return {k: v.astype(np.float32) for k, v in P.items()}


def _matmul(a, w):
    """a w^T one k at a time in the operands' type: for float32 a fixed summation order, independent of any BLAS"""
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=a.dtype)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * w[None, :, k]
    return acc


def _layer_numpy(dt, P, starts, causal):
    """the layer of reference clip.cpp:1342-1423 (quick-GELU form) in numpy, every operand and intermediate of type dt"""
    p = {k: v.astype(dt) for k, v in P.items()}
    dh = H // HEADS

    def ln(x, w, b):
        d = x - x.mean(-1, keepdims=True, dtype=dt)
        return d / np.sqrt((d * d).mean(-1, keepdims=True, dtype=dt) + dt(EPS)) * w + b

    x = p["x"]
    qkv = _matmul(ln(x, p["ln1_w"], p["ln1_b"]), p["wqkv"]) + p["bqkv"]
    qkv[:, :H] *= dt(np.float32(1.0 / np.sqrt(dh)))                        # the scale after the bias, the f32 constant the kernel gets
    a = np.zeros_like(x)
    for r0, r1 in zip(starts[:-1], starts[1:]):
        for hd in range(HEADS):
            q, k, v = (qkv[r0:r1, j * H + hd * dh:j * H + (hd + 1) * dh] for j in range(3))
            s = _matmul(q, k)
            if causal:
                s = np.where(np.tril(np.ones(s.shape, dtype=bool)), s, dt(-np.inf))
            e = np.exp(s - s.max(-1, keepdims=True))
            a[r0:r1, hd * dh:(hd + 1) * dh] = _matmul(e / e.sum(-1, keepdims=True, dtype=dt), v.T)
    x1 = x + (_matmul(a, p["wo"]) + p["bo"])
    f = _matmul(ln(x1, p["ln2_w"], p["ln2_b"]), p["w1"]) + p["b1"]
    f = f / (dt(1) + np.exp(dt(-1.702) * f))
    out = x1 + (_matmul(f, p["w2"]) + p["b2"])
    assert out.dtype == dt and qkv.dtype == dt and a.dtype == dt and f.dtype == dt
    return out


def _layer_gpu(L, P, starts, causal):
    """the same layer from the kernels' hooks, f32 handed from one to the next as the layer chain of an f32 file does (forward.cpp)"""
    import ctypes as C
    rows = P["x"].shape[0]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def ln(x, w, b):
        out = np.empty((rows, H), np.float32)
        rc = L.clip_amd_test_layernorm_ex(fp(x), rows, H, None, 1, fp(w), fp(b), EPS, rows, H, None, 0, fp(out), H)
        assert rc == 0, "clip_amd_test_layernorm_ex rc=%d" % rc
        return out

    x = np.ascontiguousarray(P["x"])
    qkv = gc.run_gemm_f32(L, P["wqkv"], ln(x, P["ln1_w"], P["ln1_b"]), "q/k/v", bias=P["bqkv"], epi=1, qcols=H, qscale=float(np.float32(1.0 / np.sqrt(H // HEADS))))
    assert qkv.shape == (rows, 3 * H)
    rc, a = ac.run_ragged(L, qkv, starts, max(LENS), H, HEADS, causal, 3)
    assert rc == 0, "clip_amd_test_attention_ragged rc=%d" % rc
    x1 = gc.run_gemm_f32(L, P["wo"], a, "out-projection", bias=P["bo"], resid=x, epi=4)
    f = gc.run_gemm_f32(L, P["w1"], ln(x1, P["ln2_w"], P["ln2_b"]), "FFN-up", bias=P["b1"], epi=3)
    return gc.run_gemm_f32(L, P["w2"], f, "FFN-down", bias=P["b2"], resid=x1, epi=4)


@pytest.fixture(scope="module")
def layer_refs():
    P = _layer_params()
    starts = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    return P, starts, {causal: (_layer_numpy(np.float64, P, starts, causal), _layer_numpy(np.float32, P, starts, causal)) for causal in (0, 1)}


@pytest.mark.parametrize("causal", [0, 1])
def test_one_f32_layer_from_the_hooks(L, layer_refs, causal):
    """LayerNorm (out32) -> q/k/v GEMM (epilogue 1, 1 / sqrt(d_head) on the first h columns) -> f32 attention on ragged lengths (1, 5, 17, 33) ->
    out-projection (epilogue 4) -> LayerNorm -> FFN-up (epilogue 3) -> FFN-down (epilogue 4) at h = 64, 2 heads, ff = 128: the contract the layer
    chain of an f32 file assumes when it reads its half_t workspaces as float — [rows][3h] with q | k | v, the scale after the bias, f32 handed on
    unrounded.  Reference: the layer in float64 numpy from the same f32 parameters; yardstick: the same numpy chain in float32 (a fixed summation
    order, no BLAS).  Per output row |gpu - f64|_inf <= LAYER_R |np32 - f64|_inf + 1e-6.  An fp16 step anywhere costs ~1e-3 against ~1e-6."""
    P, starts, refs = layer_refs
    f64, np32 = refs[causal]
    gpu = _layer_gpu(L, P, starts, causal)
    assert gpu.shape == f64.shape and np.all(np.isfinite(gpu))
    e_gpu, e_np = np.abs(gpu - f64).max(1), np.abs(np32 - f64).max(1)
    print("f32 layer %s: max over rows |gpu - f64| / |np32 - f64| = %.3f (|gpu - f64| max %.3g, |np32 - f64| max %.3g, min %.3g)" % (
        "causal" if causal else "full", float((e_gpu / e_np).max()), e_gpu.max(), e_np.max(), e_np.min()))
    assert np.all(e_gpu <= LAYER_R * e_np + 1e-6), (int(np.argmax(e_gpu / e_np)), float((e_gpu / e_np).max()))
