"""GPU tier, kernel level: the weight side of the quantised models — the panel dequantisation (k_gemm8.hip launch_dequant / dequant_kernel) with the job
lists dequant_layer of forward.cpp hands it, a caller-supplied panel through launch_gemm (GemmParams::w16_pre, and the fallback when no panel can be
had), and the LayerNorm-fold vectors of k_fold.hip — each through a hook of its own (include/clip_amd.h) that poisons what the kernel stores to and
keeps guards around it.  tests/weight_side_common.py has the numpy side (checked on its own in test_weight_side_cpu.py).

1. panels            clip_amd_test_dequant_panels: every half of every [Npad][Kpad] panel equal to panel_want (dequant_fp16 top-left, zero padding; a zero
                     may carry either sign, a weight that is itself subnormal in fp16 may arrive exact or as zero), guards before the first and behind the
                     last panel intact.  Single weights (one shape with an odd number of 32-blocks), one layer's four weights in one call and its prefixes
                     of 2 and 3, eight weights in three runs (five of a type: a cut after four; a type change; a run of two), an f16 entry that must stay
                     poison, and the layer twice bit for bit.
2. pre-built panel   clip_amd_test_gemm_panel on exact_case operands (integer expectation, no tolerance): the DevWeight handed to launch_gemm holds
                     a SECOND weight, the panel the first — the result must be the product with the first, from every kernel family, with the panel
                     built as the only job and as the last of four.  Without any panel the panel tile codes must fall back to the fused kernel.
3. fold vectors      clip_amd_test_fold_vectors, every weight type, with and without bias: bit for bit the exact sums on exact inputs; within the
                     derived bound 2^-24 |c64| + 2^-149 + K 2^-51 sum |gamma w| of a float64 reference at realistic scales; c equal to the f32
                     accumulator row of the GEMM on X = gamma (the cancellation k_fold.hip relies on).

Measured on an MI355X (printed by the cases, -s shows them):
    1. every half of every panel equal to panel_want, padding rows and columns zero, guards intact, (128, 96) included: no kernel or repack change was
       needed.  Weights that are themselves subnormal in fp16, single-weight cases: q4_0 2384, q4_1 10, q5_0 1176, q5_1 4, q8_0 157 — all arrived
       exact, none as zero.  The two calls of the layer case agree bit for bit.
    2. no element of any case differed, with the panel as the only job and as the last of four; without a panel rc 0, every element written, exact.
    3. exact: no element differed.  Realistic: max err / bound f16 0.990, q4_0 0.975, q4_1 0.987, q5_0 0.976, q5_1 0.975, q8_0 0.986 (nearly all of
       the bound is the one rounding to f32; numpy's own sequential sum reaches 0.93 .. 0.97 in test_weight_side_cpu.py).  c equals the GEMM's row bit for bit.
    The 90 cases take 5.6 s together, the slowest 0.18 s.

That the cases bite was checked once with mutations that were never committed (values and host routing only, no address or bound), of the
90 cases here:
    sb + bias -> sb in fold_kernel                       12 fail (the 6 exact and the 6 realistic fold cases, on b' with a bias)
    gamma and beta exchanged in launch_fold_vectors      18 fail (every case of 3.)
    launch_gemm ignores w16_pre                          40 fail (every case of test_prebuilt_panel_is_what_every_kernel_multiplies)
    jobs.out[jobs.n] = outs[i ? i - 1 : 0]               run on the lists of equal-sized panels only (the single-weight, pre-built-panel and no-panel
                                                         cases, 50): 40 fail (every pre-built-panel case, at lead = 3: the panel that feeds the GEMM keeps its poison)
"""
import numpy as np
import pytest

import gemm_exact_common as ge
import weight_side_common as ws
from oracle import ref
from test_gpu_gemm_exact import assert_same
from test_gpu_kernels import L, run_gemm  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

PANEL_CODES = {
    "4-wave": (128128, ws.GEMM_SHAPES, (0, 4, 1)),
    "ring": (65064, ws.GEMM_SHAPES, (0, 4, 1)),
    "8-wave 96": (96256, ws.GEMM_SHAPES, (0, 4, 1)),
    "8-wave 256": (256256, ws.GEMM_SHAPES, (0, 4, 1)),
    "gemm4": (256259, ws.GEMM_SHAPES, (0, 4, 1)),
    "gemm32": (256261, ws.GEMM_SHAPES, (1,)),                  # fp16-output epilogues only; N % 64 == 0 and K >= 128: both shapes qualify
    "split-k": (2064064, [ws.SPLIT_SHAPE], (0, 4, 1)),
    "heuristic": (0, ws.GEMM_SHAPES, (0, 4, 1)),
}
NO_PANEL_CODES = [160256, 256259, 256261]
QCOLS = 64


# --------------------------------------------------------------------------------------------------------------------------------
# 1. panels
# --------------------------------------------------------------------------------------------------------------------------------
def job(tname, N, K, sub=False):
    return (tname, ws.table(tname, N, K, sub)[0], N, K)


def check_panels(L, jobs, what):
    """one call; every quantised panel equal to panel_want, an f16 entry all poison -> (panels, subnormal weights exact, as zero)"""
    outs = ws.run_dequant_panels(L, jobs, what)
    exact = zero = 0
    for i, ((tname, raw, N, K), got) in enumerate(zip(jobs, outs)):
        w = "%s: panel %d of %d (%s N=%d K=%d)" % (what, i, len(jobs), tname, N, K)
        if tname == "f16":
            assert np.all(got == ws.POISON16), w + ": launch_dequant must skip an f16 weight, %d halfs were written" % int((got != ws.POISON16).sum())
            continue
        e, z = ws.compare_panel(got, ws.panel_want(tname, raw, N, K), w)
        exact, zero = exact + e, zero + z
    return outs, exact, zero


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_single_weight_panels(L, tname):
    """n = 1, what every other hook and launch_gemm itself pass: three shapes — (128, 96) has three 32-blocks, so the last k-block pair of the panel is half
    padding — and once with every block scale subnormal in fp16"""
    exact = zero = 0
    for (N, K) in ws.SINGLE_SHAPES:
        for sub in ((False, True) if (N, K) == ws.SINGLE_SHAPES[0] else (False,)):
            _, e, z = check_panels(L, [job(tname, N, K, sub)], "single%s" % (" subnormal d" if sub else ""))
            exact, zero = exact + e, zero + z
    print("panels single %-4s subnormal weights: %d exact, %d as zero" % (tname, exact, zero))


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("tname", ge.QTYPES)
def test_one_layer_in_one_launch(L, tname, n):
    """q/k/v, out, FFN-up, FFN-down of h = 192, ff = 768 as dequant_layer lists them, and the first 2 and 3 of them: every blk_end boundary is the last one once"""
    check_panels(L, [job(tname, N, K) for (N, K) in ws.LAYER_SHAPES[:n]], "layer n=%d" % n)


def test_runs_and_cuts(L):
    """five weights of one type (a second launch after four), a type change, a run of two — eight distinct shapes in one call"""
    check_panels(L, [job(t, N, K) for t, (N, K) in zip(ws.CUT_TYPES, ws.CUT_SHAPES)], "runs and cuts")


def test_an_f16_entry_is_skipped(L):
    (N, K) = ws.SINGLE_SHAPES[1]
    f16 = ("f16", np.ascontiguousarray(ws.table("f16", N, K, False)[0]), N, K)
    check_panels(L, [job("q4_1", *ws.SINGLE_SHAPES[0]), f16, job("q4_1", *ws.LAYER_SHAPES[1])], "q4_1, f16, q4_1")


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_layer_panels_are_deterministic(L, tname):
    jobs = [job(tname, N, K) for (N, K) in ws.LAYER_SHAPES]
    a = ws.run_dequant_panels(L, jobs, "first")
    b = ws.run_dequant_panels(L, jobs, "second")
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "panel %d: %d halfs differ between two calls" % (i, int((x != y).sum()))


# --------------------------------------------------------------------------------------------------------------------------------
# 2. pre-built panel
# --------------------------------------------------------------------------------------------------------------------------------
def gemm_args(c, epi):
    return dict(bias=c.bias, resid=c.resid if epi == 4 else None, epi=epi, qcols=QCOLS if epi == 1 else 0, qscale=ge.QSCALE if epi == 1 else 1.0)


@pytest.mark.parametrize("family,tname", [(f, t) for f in PANEL_CODES for t in ge.QTYPES])
def test_prebuilt_panel_is_what_every_kernel_multiplies(L, family, tname):
    """panel_mode 1: w16_pre holds the panel of w_raw, the DevWeight the planes of another weight; lead = 0 (the only job) and lead = 3 (the last of four)"""
    code, shapes, epis = PANEL_CODES[family]
    for (M, N, K) in shapes:
        c, raw2, W2 = ws.panel_case(tname, M, N, K)
        for epi in epis:
            want, other = c.want(epi, qcols=QCOLS), ws.other_want(c, W2, epi, qcols=QCOLS)
            assert (want != other).mean() > 0.9, "a launch that ignored the panel must not pass"
            for lead in (0, 3):
                what = "%s tile %d M=%d N=%d K=%d epilogue %d lead %d" % (tname, code, M, N, K, epi, lead)
                y = ws.run_gemm_panel(L, c.tid, c.raw, raw2, N, K, c.X, what=what, tile=code, panel_mode=1, lead=lead, **gemm_args(c, epi))
                assert_same(y, want, what)


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_panel_tiles_without_any_panel_fall_back_to_the_fused_kernel(L, tname):
    """panel_mode 0: neither w16_pre nor w16_scratch — rc 0, every element written, guard rows intact (run_gemm_panel), and the exact product"""
    for (M, N, K) in ws.GEMM_SHAPES:
        c, _, _ = ws.panel_case(tname, M, N, K)
        for code in NO_PANEL_CODES:
            for epi in (0, 1):
                what = "%s tile %d M=%d N=%d K=%d epilogue %d without a panel" % (tname, code, M, N, K, epi)
                y = ws.run_gemm_panel(L, c.tid, c.raw, None, N, K, c.X, what=what, tile=code, panel_mode=0, **gemm_args(c, epi))
                assert_same(y, c.want(epi, qcols=QCOLS), what)


# --------------------------------------------------------------------------------------------------------------------------------
# 3. fold vectors
# --------------------------------------------------------------------------------------------------------------------------------
def fold_shapes(tname):
    return ws.FOLD_SHAPES + ([ws.FOLD_F16_ONLY] if tname == "f16" else [])


def assert_vec(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d/%d differ, n %d..%d, first n=%d got %r want %r" % (
        what, len(bad), got.size, bad.min(), bad.max(), bad[0], float(got[bad[0]]), float(want[bad[0]]))


@pytest.mark.parametrize("tname", ge.WTYPES)
def test_fold_vectors_exact(L, tname):
    """every product and partial sum is exact in the kernel's double accumulator: c = float32(sum gamma w), b' = float32(sum beta w + bias), to the bit"""
    for (N, K) in fold_shapes(tname):
        f = ws.fold_exact(tname, N, K)
        assert ws.fold_partial_sums_exact(f)
        for with_bias in (True, False):
            what = "%s N=%d K=%d %s" % (tname, N, K, "with bias" if with_bias else "bias = NULL")
            c, b = ws.run_fold(L, f.tid, f.raw, N, K, f.gamma, f.beta, f.bias if with_bias else None, what=what)
            want_c, want_b = f.want(with_bias)
            assert_vec(c, want_c, what + ": c")
            assert_vec(b, want_b, what + ": b'")


@pytest.mark.parametrize("tname", ge.WTYPES)
def test_fold_vectors_realistic_scales(L, tname):
    worst = 0.0
    for (N, K) in fold_shapes(tname):
        r = ws.fold_real(tname, N, K)
        for with_bias in (True, False):
            what = "%s N=%d K=%d %s" % (tname, N, K, "with bias" if with_bias else "bias = NULL")
            c, b = ws.run_fold(L, r.tid, r.raw, N, K, r.gamma, r.beta, r.bias if with_bias else None, what=what)
            for name, got, want, mag in (("c", c, r.c64, r.mag_c), ("b'", b, r.b64[with_bias], r.mag_b[with_bias])):
                ratio = np.abs(got.astype(np.float64) - want) / ws.fold_bound(want, mag, K)
                bad = np.flatnonzero(ratio > 1.0)
                assert bad.size == 0, "%s: %s: %d/%d outside the bound, first n=%d got %r want %r; max err / bound %g" % (
                    what, name, len(bad), N, bad[0], float(got[bad[0]]), float(want[bad[0]]), ratio.max())
                worst = max(worst, float(ratio.max()))
    print("fold realistic %-4s max err / bound %.3f" % (tname, worst))


@pytest.mark.parametrize("tname", ge.WTYPES)
def test_fold_c_equals_the_gemm_accumulator_on_gamma(L, tname):
    """X = gamma as one fp16-exact row through the unsplit 64 x 64 tile, epilogue 0, no bias: the f32 accumulator of the MFMA path IS c — with exact inputs
    both are the exact sum, so mean * c_n cancels against what the GEMM accumulated to the last bit"""
    N, K = ws.FOLD_SHAPES[1]
    gmax = min(2 * ws.GUNIT, ge.BUDGET // int(K * ge.UNIT * ge.W_MAX[tname]))            # every f32 partial sum below 2^24 units of 2^-14
    f = ws.fold_exact(tname, N, K, gmax)
    assert np.array_equal(f.gamma.astype(np.float16).astype(np.float32), f.gamma) and np.abs(f.c_i).max() < 2 ** 24
    c, _ = ws.run_fold(L, f.tid, f.raw, N, K, f.gamma, f.beta, None, what=tname)
    y = run_gemm(L, f.tid, f.raw, N, K, np.ascontiguousarray(f.gamma[None, :]), epi=0, tile=1064064)
    assert_vec(c, y[0], "%s: c of launch_fold_vectors against the GEMM's accumulator row" % tname)
    assert_vec(c, f.want(False)[0], "%s: c" % tname)
