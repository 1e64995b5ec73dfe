"""CPU tier: the numpy side of test_gpu_gemm_exact.py (tests/gemm_exact_common.py) is itself checked — the model of the kernels' weight operand against
the oracle's dequantisation, the exactness of exact_case under f32 accumulation in any order, and act_bound against an f32 emulation of the two GELU
expressions of gemm_common.h: the emulation inside it, a tanh-GELU with the cubic constant 0.04 in place of 0.044715 outside it."""
import numpy as np
import pytest

import gemm_exact_common as ge
from oracle import ref
from test_gpu_entry_kernels import BLOCK_BYTES, raw_table
from test_gpu_kernels import gelu_quick, gelu_tanh


def _subnormal_d(rng, tname, raw, N, K):
    """the same blocks with every second scale d subnormal in fp16 (2^-24 .. 2^-15, both signs)"""
    blk = raw.reshape(N, K // 32, BLOCK_BYTES[tname]).copy()
    bits = rng.integers(1, 0x400, size=(N, K // 32), dtype=np.uint16) | (rng.integers(0, 2, size=(N, K // 32), dtype=np.uint16) << 15)
    bits[:, 1::2] = np.ascontiguousarray(blk[:, 1::2, 0:2]).view(np.uint16)[:, :, 0]
    blk[:, :, 0:2] = bits.view(np.uint8).reshape(N, K // 32, 2)
    return blk.reshape(N, -1)


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_operand_model_equals_fp16_of_the_oracle_weight(tname):
    """dequant_fp16 (exact value, one rounding) against ref.dequantize (ggml's f32 arithmetic) on random raw blocks: float16(oracle) bit for bit, and
    within 2^-11 relative of the f32 value (half an fp16 ulp; 2^-25 absolute below the normal range)."""
    rng = np.random.default_rng(ge.QTYPES.index(tname))
    N, K = 96, 256
    tid = ref.GGML_TYPES[tname]
    raw = raw_table(rng, tname, N, K)
    for what, r in (("scales as raw_table", raw), ("subnormal d", _subnormal_d(rng, tname, raw, N, K))):
        got = ge.dequant_fp16(tname, r, N, K)
        oracle = ref.dequantize(tid, r.reshape(-1), N, K)
        assert np.all(np.isfinite(oracle)), what
        assert np.array_equal(got.view(np.uint16), oracle.astype(np.float16).view(np.uint16)), (tname, what)
        err = np.abs(got.astype(np.float64) - oracle.astype(np.float64))
        assert np.all(err <= np.maximum(2.0 ** -11 * np.abs(oracle), 2.0 ** -25)), (tname, what, err.max())
        if what == "subnormal d":
            d = np.ascontiguousarray(r.reshape(N, K // 32, -1)[:, :, 0:2]).view(np.float16)
            assert (np.abs(d) < 2.0 ** -14).sum() >= N * K // 64 and np.all(d != 0)


@pytest.mark.parametrize("tname", ge.WTYPES)
@pytest.mark.parametrize("K", [2048, 4096])
def test_exact_case_is_exact_under_f32_accumulation_in_any_order(tname, K):
    """the int64 expectation equals f32 accumulation of the f32 products in three random chunk orders (chunks of random length, summed in random
    order, then the chunk sums in random order), at the largest xmax the budget admits; one step past the budget the helper refuses."""
    rng = np.random.default_rng(K + ge.WTYPES.index(tname))
    xmax = ge.xmax_for(tname, K)
    if tname == "q8_0":
        assert (K, xmax) in ((2048, 4), (4096, 2))
    M, N = 5, 64
    c = ge.exact_case(rng, tname, M, N, K, xmax)
    assert np.array_equal(c.X, np.rint(c.X)) and np.abs(c.X).max() == xmax
    want = c.acc.astype(np.float64) / ge.UNIT
    prod = c.X[:, None, :] * c.W.astype(np.float32)[None, :, :]                        # [M][N][K] f32 products, each exact
    assert np.array_equal(prod.astype(np.float64), c.X.astype(np.float64)[:, None, :] * c.W[None, :, :])
    for _ in range(3):
        order = rng.permutation(K)
        cuts = np.sort(rng.choice(np.arange(1, K), size=int(rng.integers(3, 40)), replace=False))
        sums = []
        for chunk in np.split(order, cuts):
            s = np.zeros((M, N), dtype=np.float32)
            for k in chunk:
                s = s + prod[:, :, k]
            sums.append(s)
        total = np.zeros((M, N), dtype=np.float32)
        for i in rng.permutation(len(sums)):
            total = total + sums[i]
        assert total.dtype == np.float32 and np.array_equal(total.astype(np.float64), want)
    assert np.array_equal(c.want(0), (want + c.bias).astype(np.float32))
    assert np.array_equal(c.want(4), (want + c.bias + c.resid).astype(np.float32))
    with pytest.raises(AssertionError, match="budget"):
        ge.exact_case(rng, tname, M, N, 2 * K, xmax)


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def emulate_gelu_tanh(x, cubic=0.044715):
    """gemm_common.h gelu_tanh in f32: e = exp2(x fma(x x, C2, C1)), t = 1 / (e + 1), r = fma(-x, t, x); each FMA computed in float64 and rounded once"""
    x = _f32(x)
    c1 = _f32(_f32(_f32(2.0) * _f32(0.79788456080286535587989211986876)) * _f32(1.44269504088896340736))
    c2 = _f32(c1 * _f32(cubic))
    with np.errstate(over="ignore"):
        inner = _f32(_f32(x * x).astype(np.float64) * np.float64(c2) + np.float64(c1))
        e = np.exp2(_f32(x * inner))
        t = _f32(_f32(1.0) / _f32(e + _f32(1.0)))
    return _f32(-x.astype(np.float64) * t.astype(np.float64) + x.astype(np.float64))


def emulate_gelu_quick(x):
    """gemm_common.h gelu_quick in f32: x / (1 + exp2(x (-1.702 log2 e)))"""
    x = _f32(x)
    k = _f32(_f32(-1.702) * _f32(1.44269504088896340736))
    with np.errstate(over="ignore"):
        t = _f32(_f32(1.0) / _f32(_f32(1.0) + np.exp2(_f32(x * k))))
    return _f32(x * t)


def test_act_bound_holds_for_the_kernel_expressions_and_rejects_a_wrong_cubic_constant():
    x = np.arange(-1024, 1025, dtype=np.float64) / 64                                   # the grid x = i / 64, |x| <= 16
    for name, emu, g in (("tanh", emulate_gelu_tanh, gelu_tanh(x)), ("quick", emulate_gelu_quick, gelu_quick(x))):
        y = emu(x).astype(np.float16).astype(np.float64)
        ratio = np.abs(y - g) / ge.act_bound(g, x)
        print("act_bound %s form: max err / bound %.3f" % (name, ratio.max()))
        assert ratio.max() <= 1.0, (name, ratio.max(), x[ratio.argmax()])
    g = gelu_tanh(x)
    mutant = emulate_gelu_tanh(x, cubic=0.04).astype(np.float16).astype(np.float64)
    outside = int((np.abs(mutant - g) > ge.act_bound(g, x)).sum())
    print("act_bound: the 0.04 mutant is outside on %d of %d points" % (outside, x.size))
    assert outside >= 300
    # ... which the tolerance of test_gpu_kernels.py::test_gemm_epilogues (2e-3 absolute and relative) lets through on all of |x| <= 4
    near = np.abs(x) <= 4
    assert np.all(np.abs(mutant - g)[near] <= 2e-3 * max(1.0, np.abs(g[near]).max()) + 2e-3 * np.abs(g[near]))
