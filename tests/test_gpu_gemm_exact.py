"""GPU tier, kernel level: the fp16-activation GEMM kernels (k_gemm.hip, k_gemm_ring.hip, k_gemm8.hip, k_gemm4.hip, k_gemm32.hip, k_skinny.hip, epilogues
in gemm_common.h) held to what they multiply, not to a reference that rounds more than they do.  tests/gemm_exact_common.py has the numpy side
(checked on its own in test_gemm_exact_cpu.py); the hooks poison every output and keep guard rows behind it (include/clip_amd.h), and run_gemm /
run_gemm_ex / run_skinny assert rc == 0 and a finite y, so every call below also says "every element was written, nothing behind row M - 1 was".

Kernel families by tile code (FAMILIES): the heuristic, the 4-wave tiles, the ring kernel, the 8-wave panel kernel, k_gemm4, k_gemm32 (epilogues 1-3, N % 64 == 0
and K >= 128 only: other calls fall back inside launch_gemm and would test another kernel under its name), explicit split-K, and the skinny kernel
(epilogues 0 and 4: the others need a LayerNorm).  Shapes: (77, 80, 64) one K-tile and a wave wholly past N; (203, 320, 192) the project's edge shape;
(333, 576, 448) 7 K-tiles, more than the ring depth; (50, 320, 1536) for the split-K codes; skinny (1, 64, 64), (17, 80, 64), (50, 768, 2048) (8 waves).

1. operand readback    X = identity rows: y[m][n] must BE dequant_fp16(...)[n][m] (value for value; a zero may carry either sign), blocks from raw_table,
                       and once with every block scale subnormal in fp16.  A weight that is itself subnormal may arrive exact or as zero.
2. exact operands      exact_case: epilogues 0, 4 (in place), 1 (qcols 0 / 64 / N), 5 (f16) equal integer arithmetic, no tolerance.
3. activations         epilogues 2 / 3 on exact pre-activations over -16 .. 16 and beyond: |y - gelu64(x)| <= act_bound; the 16 x 16 x 32 families agree bit for bit.
4. realistic scales    quantised _weights, normal X: |y - Xh Wh^T| <= 2 (K + 2) 2^-24 mag against the kernel's OWN operands (no fp16 weight term, no absolute term).
5. poison and guards   M one past a tile edge, N = 80; the rows epilogue 5 must not write keep the caller's fill bit for bit.

Measured on an MI355X (printed by the cases, -s shows them):
    1. readback: every weight of every type, family and shape equal to dequant_fp16, the runs with subnormal block scales included.  Weights that are
       themselves subnormal in fp16 (e.g. 453 254 of q4_0 in the split-K family, 45 .. 270 of the f16 tables): all arrived exact, none as zero — the
       packed fp16 dequantisation, the panel and the matrix unit keep fp16 subnormals.
    2. no element of any exact case differed.
    3. max |y - gelu64(x)| / act_bound: tanh form 0.919, quick form 0.906 (what the f32 emulation of test_gemm_exact_cpu.py gives: the kernels evaluate
       the two expressions as written); 0.98 .. 0.999 with q8_0 weights, whose larger |x| reach x = 32 + 2^-6, where gelu(x) = x lies half an fp16 ulp
       from both neighbours (the bound is the rounding itself there).  6 000 (split-K) to 110 000 results per case are subnormal in fp16 and inside the bound: the
       conversion does not flush, no allowance is made.  Every 16 x 16 x 32 family gave the bits of tile 1064064.
    4. max err / (2 (K + 2) 2^-24 mag): heuristic, 4-wave, ring, 8-wave, k_gemm4 0.011 .. 0.017 (the same figure per type in all five: the same sums);
       skinny 0.009 .. 0.012; split-K (K = 1536) 0.0003 .. 0.0004; k_gemm32 0.84 .. 0.87 of a bound that is almost all output rounding (epilogue 1).
       Up to 3779 operands per case are subnormal in fp16 (f16 and q4_1 / q5_1 weights near zero, |x| < 2^-14).
    5. every family: rc 0, finite, the two rows epilogue 5 must not write bit for bit the fill.

That the cases bite was checked once with mutations of gemm_common.h (never committed; values only, no address or loop bound), of the 194 cases here and
the 855 cases of test_gpu_kernels.py, test_gpu_gemm32.py, test_gpu_gemm_f32.py and test_gpu_parity.py that existed before:
    0.044715f -> 0.04f in gelu_tanh                      42 of the new cases fail (every case of 3.);  37 of the old (LayerNorm-fold and f32-file cases;
                                                         test_gemm_epilogues passes)
    the fifth-bit word withheld from pair s = 3          62 fail (every q5_0 / q5_1 case of 1. to 4.);  98 of the old
    bias[r] * q -> bias[r] in ln_apply                   36 fail (2. of every family that uses ln_apply: k_gemm32 and k_skinny restate it);  137 of the old
    one column strip of gemm_epilogue never stored      129 fail, the helpers' own "not finite / not written" among them (3248 of 64960 elements, columns
                                                         16 .. 31, at the edge shape);  all 66 cases of test_gemm_tiles_are_bitwise_identical, which compare two
                                                         calls at one shape, fail on that assertion
"""
import functools
import zlib

import numpy as np
import pytest

import gemm_exact_common as ge
from oracle import ref
from test_gpu_entry_kernels import BLOCK_BYTES, raw_table
from test_gpu_kernels import L, _weights, gelu_quick, gelu_tanh, run_gemm, run_gemm_ex, run_skinny  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

SKINNY = -1
BASE = 1000000 + 64064            # the unsplit 64 x 64 tile of the 4-wave kernel: what the 16 x 16 x 32 families are compared with
FAMILIES = {
    "heuristic": [0],
    "4-wave": [64064, 64128, 128064, 128128, 160128, 192128],
    "ring": [65064, 65128],
    "8-wave": [96256, 128256, 160256, 256256],
    "gemm4": [256259],
    "gemm32": [256261, 320261],
    "split-k": [2064064, 3065128],
    "skinny": [SKINNY],
}
SHAPES = [(77, 80, 64), (203, 320, 192), (333, 576, 448)]
SPLIT_SHAPE = (50, 320, 1536)
SKINNY_SHAPES = [(1, 64, 64), (17, 80, 64), (50, 768, 2048)]
PATCH_NP = {77: 7, 203: 29, 333: 37, 50: 25}           # epilogue 5: M = B Np, T = Np + 1 (test_gemm_patch_embedding_epilogue)
FILL = 777.0
GELU = {2: gelu_tanh, 3: gelu_quick}
F16_MIN_NORMAL = 2.0 ** -14

family_type = pytest.mark.parametrize("family,tname", [(f, t) for f in FAMILIES for t in ge.WTYPES])


def shapes_of(family):
    if family == "skinny":
        return SKINNY_SHAPES
    if family == "split-k":
        return [SPLIT_SHAPE]
    if family == "heuristic":
        return SHAPES + [SPLIT_SHAPE]
    if family == "gemm32":
        return [s for s in SHAPES if s[1] % 64 == 0 and s[2] >= 128]
    return SHAPES


def seed(*key):
    return zlib.crc32(repr(key).encode())


def call(L, code, tid, raw, N, K, X, bias=None, resid=None, epi=0, qcols=0, **kw):
    X = np.ascontiguousarray(X, dtype=np.float32)
    if code == SKINNY:
        return run_skinny(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=epi)
    if epi == 4:
        return run_gemm(L, tid, raw, N, K, X, bias=bias, resid=resid, epi=4, tile=code)
    return run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=epi, tile=code, qcols=qcols, qscale=ge.QSCALE if qcols else 1.0, **kw)


def assert_same(y, want, what):
    """value for value (+0 == -0), no tolerance; y is finite already (run_gemm & co)"""
    bad = np.argwhere(y != want)
    assert bad.size == 0, "%s: %d/%d differ, rows %d..%d cols %d..%d, first %s got %r want %r" % (
        what, len(bad), y.size, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), bad[0].tolist(),
        float(y[tuple(bad[0])]), float(want[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def case(tname, M, N, K):
    c = ge.exact_case(np.random.default_rng(seed("exact", tname, M, N, K)), tname, M, N, K, min(16, ge.xmax_for(tname, K)))
    for a in (c.raw, c.W, c.X, c.bias, c.resid, c.acc):
        a.setflags(write=False)
    return c


# --------------------------------------------------------------------------------------------------------------------------------
# 1. operand readback
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(tname, N, K, subnormal_d):
    """-> (raw [N][row bytes], dequant_fp16 of it); subnormal_d: every block scale d = +-2^-e, e in 15 .. 17"""
    rng = np.random.default_rng(seed("table", tname, N, K, subnormal_d))
    raw = raw_table(rng, tname, N, K)
    if subnormal_d:
        blk = raw.reshape(N, K // 32, BLOCK_BYTES[tname])
        d = (rng.choice([-1.0, 1.0], size=(N, K // 32)) * 2.0 ** -rng.integers(15, 18, size=(N, K // 32))).astype(np.float16)
        assert np.all(d != 0) and np.all(np.abs(d) < F16_MIN_NORMAL)
        blk[:, :, 0:2] = d.view(np.uint8).reshape(N, K // 32, 2)
    raw = np.ascontiguousarray(raw)
    w = ge.dequant_fp16(tname, raw, N, K)
    raw.setflags(write=False)
    w.setflags(write=False)
    return raw, w


def readback(L, code, tname, raw, N, K, epi):
    """W as the kernel multiplies it: row k of the identity against every weight row, M = K (the skinny kernel: at most 256 rows a call)"""
    rows = min(K, 256) if code == SKINNY else K
    out = np.empty((K, N), dtype=np.float32)
    for k0 in range(0, K, rows):
        X = np.zeros((rows, K), dtype=np.float32)
        X[np.arange(rows), k0 + np.arange(rows)] = 1.0
        out[k0:k0 + rows] = call(L, code, ref.GGML_TYPES[tname], raw, N, K, X, epi=epi)
    return out.T


@family_type
def test_operand_readback(L, family, tname):
    """y = I W^T is the weight operand itself: dequant_fp16 to the bit for every normal (or zero) weight — one wrong code, fifth bit, scale or a second
    rounding shows.  Epilogue 0 returns the f32 accumulator; k_gemm32 has fp16 outputs only (epilogue 1, no bias, no scale: fp16 of an fp16 number)."""
    epi = 1 if family == "gemm32" else 0
    exact = zero = 0
    for (_, N, K) in shapes_of(family):
        for sub in ((False,) if tname == "f16" else (False, True)):
            if sub and (N, K) != shapes_of(family)[0][1:]:
                continue                                                    # the subnormal scales once per family and type
            raw, w = table(tname, N, K, sub)
            want = w.astype(np.float32)
            tiny = (want != 0) & (np.abs(want) < F16_MIN_NORMAL)
            assert sub or tname == "f16" or tiny.mean() < 0.01
            for code in FAMILIES[family]:
                got = readback(L, code, tname, raw, N, K, epi)
                what = "readback %s tile %d N=%d K=%d%s" % (tname, code, N, K, " subnormal d" if sub else "")
                assert_same(np.where(tiny, want, got), want, what)
                flushed = tiny & (got == 0)
                assert_same(np.where(flushed, want, got), want, what + " (subnormal weights: exact or zero)")
                exact, zero = exact + int((tiny & ~flushed).sum()), zero + int(flushed.sum())
    print("readback %-9s %-4s subnormal weights: %d exact, %d as zero" % (family, tname, exact, zero))


# --------------------------------------------------------------------------------------------------------------------------------
# 2. exact operands
# --------------------------------------------------------------------------------------------------------------------------------
@family_type
def test_exact_operands_every_epilogue(L, family, tname):
    """exact_case: every partial sum is an f32 number in any order, so acc + bias, resid + (acc + bias) in place, float16((acc + bias) q) with the scale
    after the bias on qcols in {0, 64, N}, and the patch embedding's scatter + position rows (f16 weight) equal the integer expectation exactly."""
    calls = 0
    for i, (M, N, K) in enumerate(shapes_of(family)):
        c = case(tname, M, N, K)
        for code in FAMILIES[family]:
            what = "%s tile %d M=%d N=%d K=%d" % (tname, code, M, N, K)
            if family != "gemm32":
                assert_same(call(L, code, c.tid, c.raw, N, K, c.X, bias=c.bias, epi=0), c.want(0), what + " epilogue 0")
                assert_same(call(L, code, c.tid, c.raw, N, K, c.X, bias=c.bias, resid=c.resid, epi=4), c.want(4), what + " epilogue 4")
                calls += 2
                if i == 0:
                    assert_same(call(L, code, c.tid, c.raw, N, K, c.X, bias=None, epi=0), c.want(0, bias=False), what + " epilogue 0 without bias")
            if family != "skinny":
                for qcols in (0, 64, N):
                    want = c.want(1, qcols=qcols)
                    assert np.all(np.isfinite(want))
                    assert_same(call(L, code, c.tid, c.raw, N, K, c.X, bias=c.bias, epi=1, qcols=qcols), want, what + " epilogue 1 qcols %d" % qcols)
                    calls += 1
            if family not in ("gemm32", "skinny") and tname == "f16":
                Np = PATCH_NP[M]
                B, T = M // Np, Np + 1
                pos_i = np.random.default_rng(seed("pos", M, N)).integers(-4 * ge.UNIT, 4 * ge.UNIT + 1, size=(T, N))
                y = np.full((B * T, N), FILL, dtype=np.float32)
                y = call(L, code, c.tid, c.raw, N, K, c.X, epi=5, Np=Np, T=T, pos=(pos_i / ge.UNIT).astype(np.float32), y=y).reshape(B, T, N)
                want = ((c.acc.reshape(B, Np, N) + pos_i[None, 1:, :]) / ge.UNIT).astype(np.float32)
                assert np.all(y[:, 0, :].view(np.uint32) == np.float32(FILL).view(np.uint32)), what + " epilogue 5: class rows written"
                assert_same(y[:, 1:, :].reshape(M, N), want.reshape(M, N), what + " epilogue 5")
                calls += 1
    assert calls > 0


# --------------------------------------------------------------------------------------------------------------------------------
# 3. activations over their range
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def act_case(tname, M, N, K):
    """rows of X with two or three +-1 entries, a bias per column from -12 to 10 and three columns at 200: x = X W^T + bias is a short sum of
    multiples of 2^-6, exact in f32 in any order -> (X, bias, x as float64)"""
    c = case(tname, M, N, K)
    rng = np.random.default_rng(seed("act", tname, M, N, K))
    Xi = np.zeros((M, K), dtype=np.int64)
    for m in range(M):
        cols = rng.choice(K, size=int(rng.integers(2, 4)), replace=False)
        Xi[m, cols] = rng.choice([-1, 1], size=len(cols))
    bias_i = np.rint(np.linspace(-12.0, 10.0, N) * ge.UNIT).astype(np.int64)
    bias_i[[3, N // 2, N - 1]] = 200 * ge.UNIT
    x_i = Xi @ np.rint(c.W * ge.UNIT).astype(np.int64).T + bias_i
    assert np.abs(x_i).max() < 2 ** 24
    out = (Xi.astype(np.float32), (bias_i / ge.UNIT).astype(np.float32), x_i / ge.UNIT)
    for a in out:
        a.setflags(write=False)
    return out


_act_base = {}


def act_base(L, tname, shape, epi):
    key = (tname, shape, epi)
    if key not in _act_base:
        M, N, K = shape
        c = case(tname, M, N, K)
        X, bias, _ = act_case(tname, M, N, K)
        _act_base[key] = call(L, BASE, c.tid, c.raw, N, K, X, bias=bias, epi=epi)
    return _act_base[key]


@pytest.mark.parametrize("family,tname", [(f, t) for f in FAMILIES if f != "skinny" for t in ge.WTYPES])
def test_activations_over_their_range(L, family, tname):
    """tanh GELU (2) and quick GELU (3) at arguments numpy knows exactly: near zero, the negative tail where x - x t cancels and the results pass
    through the fp16 subnormals, and x > 100 where exp2 overflows — within act_bound of the float64 function, and the same bits from every
    16 x 16 x 32 kernel (k_gemm32 restates the epilogue on other fragments: held to the bound)."""
    xs = np.concatenate([act_case(tname, *s)[2].ravel() for s in shapes_of(family)])
    distinct = np.unique(xs)
    assert (np.abs(distinct) <= 16).sum() >= 1000 and ((distinct >= -8) & (distinct <= -3)).sum() >= 100 and (xs > 100).any()
    worst = {2: 0.0, 3: 0.0}
    tiny = 0
    for shape in shapes_of(family):
        M, N, K = shape
        c = case(tname, M, N, K)
        X, bias, x = act_case(tname, M, N, K)
        for epi in (2, 3):
            g = GELU[epi](x)
            bound = ge.act_bound(g, x)
            tiny += int(((g != 0) & (np.abs(g) < F16_MIN_NORMAL)).sum())
            for code in FAMILIES[family]:
                y = call(L, code, c.tid, c.raw, N, K, X, bias=bias, epi=epi)
                ratio = np.abs(y - g) / bound
                what = "%s tile %d M=%d N=%d K=%d epilogue %d" % (tname, code, M, N, K, epi)
                bad = np.argwhere(ratio > 1.0)
                assert bad.size == 0, "%s: %d/%d outside act_bound, first %s x %r got %r want %r; max err / bound %g" % (
                    what, len(bad), y.size, bad[0].tolist(), float(x[tuple(bad[0])]), float(y[tuple(bad[0])]), float(g[tuple(bad[0])]), ratio.max())
                worst[epi] = max(worst[epi], float(ratio.max()))
                if family != "gemm32":
                    assert_same(y, act_base(L, tname, shape, epi), what + " against tile %d" % BASE)
    print("activations %-9s %-4s max err / act_bound: tanh %.3f quick %.3f; %d results subnormal in fp16" % (family, tname, worst[2], worst[3], tiny))


# --------------------------------------------------------------------------------------------------------------------------------
# 4. realistic scales against the kernel's own operands
# --------------------------------------------------------------------------------------------------------------------------------
class Real:
    """quantised _weights and a standard normal X: the float64 product of the operands the kernel multiplies (fp16(X), dequant_fp16) and its magnitude"""

    def __init__(self, tname, M, N, K):
        rng = np.random.default_rng(seed("real", tname, M, N, K))
        self.tid = ref.GGML_TYPES[tname]
        self.raw = ref.quantize(self.tid, _weights(rng, N, K))
        Wh = ge.dequant_fp16(tname, self.raw.reshape(N, -1), N, K).astype(np.float64)
        self.X = rng.standard_normal((M, K)).astype(np.float32)
        Xh = self.X.astype(np.float16).astype(np.float64)
        self.bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        self.resid = rng.standard_normal((M, N)).astype(np.float32)
        aX, aW = np.abs(Xh), np.abs(Wh)
        self.lin = Xh @ Wh.T + self.bias
        self.mag = aX @ aW.T + np.abs(self.bias)
        # products with an operand that is subnormal in fp16 (the matrix unit may take it as zero): their whole magnitude
        sX, sW = aX * ((aX > 0) & (aX < F16_MIN_NORMAL)), aW * ((aW > 0) & (aW < F16_MIN_NORMAL))
        self.sub = sX @ aW.T + aX @ sW.T
        self.n_sub = int((sX > 0).sum() + (sW > 0).sum())
        self.K = K


@functools.lru_cache(maxsize=None)
def real(tname, M, N, K):
    return Real(tname, M, N, K)


@family_type
def test_realistic_scales_against_the_kernels_own_operands(L, family, tname):
    """bound 2 (K + 2) 2^-24 mag, mag = |Xh| |Wh|^T + |bias| (+ |resid|): rigorous if each of the K accumulation steps (and the two epilogue additions) errs by
    at most one f32 ulp of a partial sum <= mag — which covers a truncating adder.  k_gemm32: epilogue 1, plus the fp16 rounding of the output."""
    worst, n_sub = 0.0, 0
    for (M, N, K) in shapes_of(family):
        r = real(tname, M, N, K)
        n_sub += r.n_sub
        for code in FAMILIES[family]:
            for epi in ((1,) if family == "gemm32" else (0, 4)):
                want = r.lin + r.resid if epi == 4 else r.lin
                bound = 2 * (K + 2) * 2.0 ** -24 * (r.mag + np.abs(r.resid) if epi == 4 else r.mag) + r.sub
                if epi == 1:
                    bound = bound + np.maximum(2.0 ** -11 * (np.abs(want) + bound), 2.0 ** -25)
                y = call(L, code, r.tid, r.raw, N, K, r.X, bias=r.bias, resid=r.resid if epi == 4 else None, epi=epi)
                ratio = np.abs(y - want) / bound
                bad = np.argwhere(ratio > 1.0)
                assert bad.size == 0, "%s tile %d M=%d N=%d K=%d epilogue %d: %d/%d outside, first %s got %r want %r; max err / bound %g" % (
                    tname, code, M, N, K, epi, len(bad), y.size, bad[0].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])]), ratio.max())
                worst = max(worst, float(ratio.max()))
    print("realistic %-9s %-4s max err / bound %.4f (%d operands subnormal in fp16)" % (family, tname, worst, n_sub))


# --------------------------------------------------------------------------------------------------------------------------------
# 5. poison and guards
# --------------------------------------------------------------------------------------------------------------------------------
def rows_of(code):
    """activation rows of the tile behind a code (the heuristic and the skinny kernel: 64 / 16)"""
    if code == SKINNY:
        return 16
    bm = (code % 1000000) // 1000
    return 64 if bm in (0, 65) else bm


@pytest.mark.parametrize("family", list(FAMILIES))
def test_poisoned_outputs_and_guard_rows(L, family):
    """M one past a tile edge (a last tile with ONE valid row) and N = 80 (a wave wholly past N; k_gemm32: N = 128, K = 128, what it accepts): the hook returns
    0 (no guard row behind row M - 1 changed) and y is finite (no element kept its poison) — asserted by the helpers, and again here.  Epilogue 5 with
    T = Np + 2: the class row and the row past the last patch keep the caller's fill bit for bit."""
    N, K = (128, 128) if family == "gemm32" else (80, 64)
    for code in FAMILIES[family]:
        M = rows_of(code) + 1
        c = case("f16", M, N, K)
        what = "tile %d M=%d N=%d K=%d" % (code, M, N, K)
        if family == "gemm32":
            y = call(L, code, c.tid, c.raw, N, K, c.X, bias=c.bias, epi=1)
            assert np.all(np.isfinite(y))
            assert_same(y, c.want(1), what)
            continue
        for epi in (0, 4):
            y = call(L, code, c.tid, c.raw, N, K, c.X, bias=c.bias, resid=c.resid, epi=epi)
            assert np.all(np.isfinite(y))
            assert_same(y, c.want(epi), what + " epilogue %d" % epi)
        if family == "skinny":
            continue
        T = M + 2
        pos_i = np.random.default_rng(seed("pos5", M)).integers(-4 * ge.UNIT, 4 * ge.UNIT + 1, size=(T, N))
        y = call(L, code, c.tid, c.raw, N, K, c.X, epi=5, Np=M, T=T, pos=(pos_i / ge.UNIT).astype(np.float32), y=np.full((T, N), FILL, dtype=np.float32))
        assert np.all(y[[0, T - 1]].view(np.uint32) == np.float32(FILL).view(np.uint32)), what + " epilogue 5: a row that is not a patch row was written"
        assert_same(y[1:T - 1], ((c.acc + pos_i[1:T - 1]) / ge.UNIT).astype(np.float32), what + " epilogue 5")
