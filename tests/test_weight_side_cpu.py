"""CPU tier: the numpy side of test_gpu_weight_side.py (tests/weight_side_common.py) is itself checked — panel_want against the oracle's
dequantisation, the comparison rule on made-up panels, the exactness of the exact fold inputs in float64, the derived bound of the realistic fold
case against numpy's own sequential sum, and that the two expectations of the pre-built-panel cases differ — and the three hooks refuse bad arguments
with -3 before they look for a device (needs the library, no device)."""
import numpy as np
import pytest

import gemm_exact_common as ge
import weight_side_common as ws
from oracle import ref

ALL_PANEL_SHAPES = sorted(set(ws.SINGLE_SHAPES + ws.LAYER_SHAPES + ws.CUT_SHAPES))


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_panel_want_is_fp16_of_the_oracle_weight_zero_padded(tname):
    for (N, K) in ALL_PANEL_SHAPES:
        for sub in ((False, True) if (N, K) == ws.SINGLE_SHAPES[0] else (False,)):
            raw, w = ws.table(tname, N, K, sub)
            want = ws.panel_want(tname, raw, N, K)
            Np, Kp = (N + 127) // 128 * 128, (K + 63) // 64 * 64
            assert want.dtype == np.float16 and want.shape == (Np, Kp) and Np % 128 == 0 and Kp % 64 == 0 and 0 <= Np - N < 128 and 0 <= Kp - K < 64
            oracle = ref.dequantize(ref.GGML_TYPES[tname], raw.reshape(-1), N, K)
            assert np.array_equal(want[:N, :K].view(np.uint16), oracle.astype(np.float16).view(np.uint16)), (tname, N, K, sub)
            assert np.array_equal(want[:N, :K], w)
            assert not want[N:].view(np.uint16).any() and not want[:, K:].view(np.uint16).any()
            if sub:
                d = np.ascontiguousarray(raw.reshape(N, K // 32, -1)[:, :, 0:2]).view(np.float16)
                assert np.all(d != 0) and np.all(np.abs(d.astype(np.float32)) < ws.F16_MIN_NORMAL), "every block scale is subnormal in fp16"
    assert ws.pad_shape(128, 96) == (128, 128) and ws.pad_shape(80, 64) == (128, 64) and ws.pad_shape(192, 768) == (256, 768)


def test_compare_panel_admits_signed_zeros_and_flushed_subnormals_only():
    want = np.zeros((128, 64), dtype=np.float16)
    want[0, :4] = [1.5, -2.0 ** -15, 2.0 ** -24, -0.25]
    good = want.view(np.uint16).copy()
    assert ws.compare_panel(good, want, "same") == (2, 0)
    v = good.copy()
    v[5, 5] = 0x8000                                                       # -0 for +0
    v[0, 1] = 0x8000                                                       # a subnormal weight as (signed) zero
    assert ws.compare_panel(v, want, "zeros") == (1, 1)
    for what, (r, c, bits) in {"poison": (100, 63, ws.POISON16), "normal weight as zero": (0, 0, 0), "subnormal weight off by one": (0, 2, 2),
                               "padding written": (127, 63, 0x0001), "last bit": (0, 3, np.float16(-0.25).view(np.uint16) + 1)}.items():
        v = good.copy()
        v[r, c] = bits
        with pytest.raises(AssertionError):
            ws.compare_panel(v, want, what)


@pytest.mark.parametrize("tname", ge.WTYPES)
def test_exact_fold_inputs_are_exact_in_float64(tname):
    """the int64 expectation equals float64 accumulation of the float64 products, sequentially as the kernel runs and in a random order, to the bit;
    gamma, beta and the bias are what the test says they are"""
    rng = np.random.default_rng(ge.WTYPES.index(tname))
    for (N, K) in ws.FOLD_SHAPES + ([ws.FOLD_F16_ONLY] if tname == "f16" else []):
        f = ws.fold_exact(tname, N, K)
        assert ws.fold_partial_sums_exact(f)
        assert np.abs(f.gamma).max() <= 2 and np.abs(f.beta).max() <= 2 and np.abs(f.gamma).max() > 1.5
        assert np.array_equal(f.gamma * 256, np.rint(f.gamma * 256)) and np.array_equal(f.bias * 64, np.rint(f.bias * 64))
        assert np.array_equal(ge.dequant_fp16(tname, f.raw, N, K).astype(np.float64), f.W), "every weight is an fp16 number"
        for order in (np.arange(K), rng.permutation(K)):
            sc, sb = np.zeros(N), np.zeros(N)
            for k in order:
                sc = sc + np.float64(f.gamma[k]) * f.W[:, k]
                sb = sb + np.float64(f.beta[k]) * f.W[:, k]
            assert np.array_equal(sc * ws.FUNIT, f.c_i) and np.array_equal(sb * ws.FUNIT, f.b_i)
            for with_bias in (False, True):
                c, b = f.want(with_bias)
                assert c.dtype == np.float32 and np.array_equal(c, sc.astype(np.float32))
                assert np.array_equal(b, (sb + f.bias.astype(np.float64)).astype(np.float32) if with_bias else sb.astype(np.float32))


@pytest.mark.parametrize("K", [64, 448, 3072])
def test_realistic_fold_bound_admits_a_sequential_double_sum(K):
    """numpy's sequential float64 sum, rounded once to f32 (what fold_kernel computes), against the pairwise / blocked float64 reference: inside the bound"""
    worst = 0.0
    for tname in ("f16", "q4_0", "q5_1"):
        r = ws.fold_real(tname, 80, K)
        sc, sb = np.zeros(80), np.zeros(80)
        for k in range(K):
            sc = sc + np.float64(r.gamma[k]) * r.W[:, k]
            sb = sb + np.float64(r.beta[k]) * r.W[:, k]
        sbb = sb + r.bias.astype(np.float64)
        for got, want, mag in ((sc, r.c64, r.mag_c), (sb, r.b64[False], r.mag_b[False]), (sbb, r.b64[True], r.mag_b[True])):
            ratio = np.abs(got.astype(np.float32).astype(np.float64) - want) / ws.fold_bound(want, mag, K)
            worst = max(worst, float(ratio.max()))
    print("fold bound K=%d: sequential double sum, max err / bound %.3f" % (K, worst))
    assert worst <= 1.0
    # ... and a float32 accumulator (the error the bound is there to catch) is far outside it
    r = ws.fold_real("q4_0", 80, K)
    s32 = np.zeros(80, dtype=np.float32)
    for k in range(K):
        s32 = s32 + r.gamma[k] * r.W[:, k].astype(np.float32)
    assert (np.abs(s32.astype(np.float64) - r.c64) / ws.fold_bound(r.c64, r.mag_c, K)).max() > 1.0


@pytest.mark.parametrize("tname", ge.QTYPES)
def test_the_two_expectations_of_the_pre_built_panel_cases_differ(tname):
    for (M, N, K) in ws.GEMM_SHAPES + [ws.SPLIT_SHAPE]:
        c, raw2, W2 = ws.panel_case(tname, M, N, K)
        assert raw2.shape == c.raw.shape and not np.array_equal(raw2, c.raw)
        for epi, qcols in ((0, 0), (4, 0), (1, 64)):
            a, b = c.want(epi, qcols=qcols), ws.other_want(c, W2, epi, qcols=qcols)
            assert a.shape == b.shape == (M, N) and (a != b).mean() > 0.9, (tname, M, N, K, epi, (a != b).mean())


def test_hooks_refuse_bad_arguments_before_they_look_for_a_device(clip_lib):
    L = clip_lib.lib()
    N, K, M = 128, 64, 4
    raw = {t: ws.table(t, N, K, False)[0] for t in ge.QTYPES}
    f16 = np.zeros((N, K), dtype=np.float16).view(np.uint8)
    X = np.zeros((M, K), dtype=np.float32)
    q = ("q4_0", raw["q4_0"], N, K)
    # clip_amd_test_dequant_panels
    for what, jobs, n in (("n = 0", [q], 0), ("n = 9", [q] * 9, 9), ("n < 0", [q], -1), ("f32 entry", [q, (0, raw["q4_0"], N, K)], None),
                          ("unknown type", [(5, raw["q4_0"], N, K)], None), ("N = 0", [("q4_0", raw["q4_0"], 0, K)], None),
                          ("K < 0", [q, ("q8_0", raw["q8_0"], N, -64)], None)):
        rc, ok, outs = ws.call_dequant_panels(L, jobs, n=n)
        assert rc == -3 and ok == -1, (what, rc, ok)
        assert all(np.all(o == 0xffff) for o in outs), (what, "a panel was written")
    assert L.clip_amd_test_dequant_panels(1, None, None, None, None, None, None) == -3
    # clip_amd_test_gemm_panel
    tid = ref.GGML_TYPES["q4_0"]
    base = dict(epi=0, tile=128128, panel_mode=1, lead=0)
    for what, kw in (("lead = 4", dict(lead=4)), ("lead < 0", dict(lead=-1)), ("panel_mode = 2", dict(panel_mode=2)), ("panel_mode < 0", dict(panel_mode=-1)),
                     ("epilogue 5", dict(epi=5)), ("epilogue -1", dict(epi=-1)), ("epilogue 4 without resid", dict(epi=4)),
                     ("qcols > N", dict(epi=1, qcols=N + 1)), ("qcols < 0", dict(epi=1, qcols=-1)), ("tile < 0", dict(tile=-1)),
                     ("lead with panel_mode 0", dict(panel_mode=0, lead=1))):
        rc, y = ws.call_gemm_panel(L, tid, raw["q4_0"], None, N, K, X, **dict(base, **kw))
        assert rc == -3 and np.all(np.isnan(y)), (what, rc)
    for what, t, w in (("f16 with a pre-built panel", ref.GGML_TYPES["f16"], f16), ("f32", 0, np.zeros((N, K), dtype=np.float32))):
        assert ws.call_gemm_panel(L, t, w, None, N, K, X, **base)[0] == -3, what
    assert ws.call_gemm_panel(L, tid, raw["q4_0"], raw["q4_0"], N, K, X, epi=0, tile=160256, panel_mode=0)[0] == -3, "second weight with panel_mode 0"
    assert ws.call_gemm_panel(L, tid, None, None, N, K, X, **base)[0] == -3, "w_raw = NULL"
    assert ws.call_gemm_panel(L, tid, raw["q4_0"], None, 0, K, X, **base)[0] == -3, "N = 0"
    # clip_amd_test_fold_vectors
    g = np.ones(K, dtype=np.float32)
    for what, a in (("f32", (0, raw["q4_0"], N, K, g, g, None)), ("unknown type", (4, raw["q4_0"], N, K, g, g, None)), ("N = 0", (tid, raw["q4_0"], 0, K, g, g, None)),
                    ("K < 0", (tid, raw["q4_0"], N, -K, g, g, None)), ("no gamma", (tid, raw["q4_0"], N, K, None, g, None)),
                    ("no beta", (tid, raw["q4_0"], N, K, g, None, None)), ("no weight", (tid, None, N, K, g, g, None))):
        rc, c, b = ws.call_fold(L, *a)
        assert rc == -3 and np.all(np.isnan(c)) and np.all(np.isnan(b)), (what, rc)
    assert L.clip_amd_test_fold_vectors(tid, raw["q4_0"].ctypes.data, N, K, ws._fp(g), ws._fp(g), None, None, None) == -3
    for name in ("clip_amd_test_dequant_panels", "clip_amd_test_gemm_panel", "clip_amd_test_fold_vectors"):
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
