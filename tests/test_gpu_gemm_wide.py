"""GPU tier, kernel level: the 256-column tiles of the fused-dequant GEMM (csrc/gemm_wide.h, tile codes 128257 / 160257: one LDS image of W rotated by
k-slice, two workgroups per CU) through clip_amd_test_gemm_ex and clip_amd_test_fold_consumer.

Every launch is compared BITWISE with tile 160128 on the same buffers (same MFMA, k order, dequantisation and epilogue expressions), and against the
float64 product of the operands with the bounds the existing GEMM tests use:
    epilogue 1     |y - want| <= 1e-3 (|Xh| |Wd|^T + |bias|) + |want| 2^-10 + 1e-4          (test_gpu_kernels.test_gemm_f16_epilogue_q_scale_columns)
    epilogue 2, 3  |y - act(lin)| <= 1.13 (1e-3 (|Xh| |Wd|^T + |bias|) + 1e-4) + |act(lin)| 2^-10: the same bound on the pre-activation through the
                   1.13-Lipschitz activations (lnfold_parts_common.consumer_expect), plus the output's fp16 rounding
The hooks poison the outputs and keep guard rows behind row M - 1 (rc -6 when one changes); the output rows are N wide, so a store past column N
lands in the next row and breaks the bitwise comparison.

Shapes: M in {1, 127, 128, 129, 159, 160, 161, 321} (one row, both tile heights +- 1, three row tiles), N in {256, 264, 512, 768} (264: a second column
tile with 8 valid columns, weight rows clamped past the padded plane), K in {64, 128, 512, 768} (1, 2, 8, 12 K-steps: the first, second and steady-state
rotations of the W image).  16 (M, N, K) per weight type and tile height cover every M twice and every (N, K) pair once; the epilogue rotates with them.
"""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import gemm_exact_common as ge
import lnfold_parts_common as lp
from oracle import ref
from test_gpu_kernels import L, _diff_report, _h, _weights, gelu_quick, gelu_tanh, run_gemm_ex  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = {128: 128257, 160: 160257}
BASE = 160128
MS = [1, 127, 128, 129, 159, 160, 161, 321]
NS = [256, 264, 512, 768]
KS = [64, 128, 512, 768]
SHAPES = [(MS[(3 * j) % 8], NS[j % 4], KS[j // 4]) for j in range(16)]
ACT = {2: gelu_tanh, 3: gelu_quick}


def test_shape_plan_covers_the_edges():
    assert {(s[1], s[2]) for s in SHAPES} == {(n, k) for n in NS for k in KS}
    assert all(sum(1 for s in SHAPES if s[0] == m) == 2 for m in MS)
    for t in range(len(ge.QTYPES)):          # every epilogue at every K-step count, for every weight type
        assert {(1 + (j + t) % 3, SHAPES[j][2]) for j in range(16)} == {(e, k) for e in (1, 2, 3) for k in KS}


@functools.lru_cache(maxsize=None)
def real_case(tname, M, N, K):
    """quantised weights (x 4: pre-activations across the GELU knee), normal X, a bias; the float64 product of the operands the kernel multiplies"""
    rng = np.random.default_rng(zlib.crc32(repr(("wide", tname, M, N, K)).encode()))
    tid = ref.GGML_TYPES[tname]
    raw = ref.quantize(tid, _weights(rng, N, K) * 4)
    Wd = ref.dequantize(tid, raw, N, K).astype(np.float64)
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    Xh = _h(X).astype(np.float64)
    lin = Xh @ Wd.T + bias
    blin = 1.0e-3 * (np.abs(Xh) @ np.abs(Wd).T + np.abs(bias)) + 1e-4
    for a in (raw, X, bias, lin, blin):
        a.setflags(write=False)
    return tid, raw, X, bias, lin, blin


def check_against_float64(y, lin, blin, epi, qcols, qscale, what):
    if epi == 1:
        want = lin.copy()
        want[:, :qcols] *= np.float32(qscale)
        bound = blin + np.abs(want) * 2.0 ** -10
    else:
        want = ACT[epi](lin)
        bound = 1.13 * blin + np.abs(want) * 2.0 ** -10
    err = np.abs(y - want)
    bad = np.argwhere(err > bound)
    print("%s: max err / bound %.4f" % (what, float((err / bound).max())))
    assert bad.size == 0, "%s: %d/%d outside, first %s got %r want %r" % (what, len(bad), y.size, bad[0].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])]))


@pytest.mark.parametrize("bm", [128, 160])
@pytest.mark.parametrize("tname", ge.QTYPES)
def test_wide_tile_edges_bitwise_and_float64(L, tname, bm):
    t = ge.QTYPES.index(tname)
    for j, (M, N, K) in enumerate(SHAPES):
        epi = 1 + (j + t) % 3
        tid, raw, X, bias, lin, blin = real_case(tname, M, N, K)
        what = "%s tile %d M=%d N=%d K=%d epilogue %d" % (tname, WIDE[bm], M, N, K, epi)
        base = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=epi, tile=BASE)
        y = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=epi, tile=WIDE[bm])
        assert np.array_equal(base, y), (what, _diff_report(base, y))
        check_against_float64(y, lin, blin, epi, 0, 1.0, what)


@pytest.mark.parametrize("bm", [128, 160])
@pytest.mark.parametrize("tname", ["q4_0", "q5_1", "q8_0"])
def test_wide_tile_q_scale_columns(L, tname, bm):
    """EPI_F16 with the Q scale on columns n < qcols: 128 (a wave's first half), 100 / 332 (a boundary inside a 64-column half, in the first and in the
    second column tile's range of waves) and 256 (the whole first tile), with and without a bias"""
    M, N, K = 161, 512, 128
    tid, raw, X, bias, lin, blin = real_case(tname, M, N, K)
    for qcols, qscale in ((128, 0.125), (100, 0.3), (332, 0.3), (256, 0.125)):
        what = "%s tile %d qcols %d" % (tname, WIDE[bm], qcols)
        base = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=1, tile=BASE, qcols=qcols, qscale=qscale)
        y = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=1, tile=WIDE[bm], qcols=qcols, qscale=qscale)
        assert np.array_equal(base, y), (what, _diff_report(base, y))
        check_against_float64(y, lin, blin, 1, qcols, qscale, what)
    nb = run_gemm_ex(L, tid, raw, N, K, X, bias=None, epi=1, tile=WIDE[bm], qcols=128, qscale=0.125)
    assert np.array_equal(nb, run_gemm_ex(L, tid, raw, N, K, X, bias=None, epi=1, tile=BASE, qcols=128, qscale=0.125))


@pytest.mark.parametrize("bm", [128, 160])
@pytest.mark.parametrize("tname", lp.TYPES[1:])
def test_wide_tile_fold_consumer(L, tname, bm):
    """The consumer half of the LayerNorm fold on planted statistics with a (mean, rstd) of its own in every row, c and b' non-trivial, with and without
    the centring offsets: bit for bit the 160 x 128 tile (outputs and the row means left for the next producer), and inside the windows of
    lnfold_parts_common (exact statistics: integer arithmetic; general ones: the derived delta).  N2 = 264: the direct-store form beside the staged one."""
    specs = [(161, 264, 128, 64, True, 1), (321, 512, 320, 64, False, 2), (129, 256, 1024, 32, False, 3), (160, 768, 64, 64, True, 1)]
    for (M, N2, h, slotw, exact, epi) in specs:
        cs = lp.consumer_case(tname, M, N2, h, slotw, exact)
        qc, qs = (lp.QCOLS, lp.QSCALE) if epi == 1 else (0, 1.0)
        for with_mu in (True, False):
            what = "%s tile %d M=%d N2=%d h=%d slotw=%d exact=%d epilogue %d mu %d" % (tname, WIDE[bm], M, N2, h, slotw, exact, epi, with_mu)
            out = []
            for tile in (BASE, WIDE[bm]):
                rc, y, mu_out = lp.call_consumer(L, cs.tid, cs.raw, N2, h, cs.xg, cs.st, slotw, cs.mu if with_mu else None, cs.c, cs.bf, cs.eps, epi, qc, qs, tile)
                assert rc == 0, (what, tile, rc)
                assert not np.any(np.isnan(y)), (what, tile, "%d outputs NaN / not written" % np.isnan(y).sum())
                out.append((y, mu_out))
            assert np.array_equal(out[0][0], out[1][0]), (what, _diff_report(out[0][0], out[1][0]))
            assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32)), (what, "mu_out")
            y = out[1][0]
            _, lo, hi, exc = lp.consumer_expect(cs, epi, with_mu)
            bad = np.argwhere((y < lo) | (y > hi))
            assert len(bad) == 0, (what, "%d / %d outside their windows, first %s" % (len(bad), y.size, bad[0].tolist()))


@pytest.mark.parametrize("bm", [128, 160])
def test_wide_tile_many_tiles_race_screen(L, bm):
    """More workgroups than one resident round would need per XCD, twelve K-steps, six launches: a W slice written before its last reader passed the
    barrier, or read before its writer did, shows as a wrong tile or as run-to-run differences."""
    rng = np.random.default_rng(5)
    M, N, K = 1600, 1024, 768
    tid = ref.GGML_TYPES["q4_0"]
    raw = ref.quantize(tid, _weights(rng, N, K))
    X = rng.standard_normal((M, K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    base = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=1, tile=BASE)
    for i in range(6):
        y = run_gemm_ex(L, tid, raw, N, K, X, bias=bias, epi=1, tile=WIDE[bm])
        assert np.array_equal(base, y), (i, _diff_report(base, y))


def test_other_launches_with_a_wide_code_run_the_narrow_tile(L):
    """f16 weights and the f32 / residual epilogues are not carried by the wide tile: launch_gemm runs them on 160 x 128, same bits"""
    rng = np.random.default_rng(9)
    M, N, K = 203, 320, 192
    X = rng.standard_normal((M, K)).astype(np.float32)
    for tname, epi in (("f16", 1), ("q4_0", 0), ("f16", 0)):
        tid = ref.GGML_TYPES[tname]
        raw = ref.quantize(tid, _weights(rng, N, K))
        for code in WIDE.values():
            assert np.array_equal(run_gemm_ex(L, tid, raw, N, K, X, epi=epi, tile=code), run_gemm_ex(L, tid, raw, N, K, X, epi=epi, tile=BASE)), (tname, epi, code)


_CHILD = r"""
import os, sys
import numpy as np
from clip_cpp_amd import synth
n_img, n_txt, cache, out, forced = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5] == "1"
texts = synth.token_ids(n_txt, seed=23, min_len=8, max_len=75)
Mt, Mv = sum(len(t) for t in texts), n_img * 50
shapes = [(Mv, 2304, 768, 160257), (Mv, 3072, 768, 160257), (Mt, 1536, 512, 128257), (Mt, 2048, 512, 160257)]
if forced:
    os.environ["CLIP_AMD_TILE_OVERRIDE"] = ";".join("%d,%d,%d,%d" % s for s in shapes)
else:
    os.environ.pop("CLIP_AMD_TILE_OVERRIDE", None)
import clip_cpp_amd
L = clip_cpp_amd.lib()
path = synth.cached_model(cache, "b32", "q4_0", text=True, vision=True, seed=1234)
c = clip_cpp_amd.Clip(path, device=0)
tiles = [L.clip_amd_test_gemm_tile_ex(m, n, k, 1, 0) for (m, n, k, _) in shapes]
imgs = np.random.default_rng(3).standard_normal((n_img, 224, 224, 3), dtype=np.float32)
ei = np.asarray(c.encode_images(imgs))
et = np.asarray(c.encode_texts(texts))
c.profile(True)
c.encode_texts(texts)
fams = sorted({k.split("/")[0] for k in c.profile_report()})
np.savez(out, ei=ei, et=et, tiles=np.array(tiles), want=np.array([s[3] for s in shapes]), wide=np.array([f for f in fams if ",256," in f and f.startswith("gemm_dma_kernel")]))
"""


def test_end_to_end_forced_rule_equals_unforced(L, fixture_cache, tmp_path):
    """ViT-B/32 q4_0, 170 images and 128 texts: with CLIP_AMD_TILE_OVERRIDE putting the q/k/v and FFN-up GEMMs of both towers on the wide tiles the
    embeddings are bit for bit those of the unforced context.  The override is read once per process, so each side is a process of its own."""
    res = {}
    for forced in ("1", "0"):
        out = str(tmp_path / ("e2e_%s.npz" % forced))
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", _CHILD, "170", "128", fixture_cache, out, forced], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[forced] = np.load(out)
    f, u = res["1"], res["0"]
    assert np.array_equal(f["tiles"], f["want"]), (f["tiles"], "the override did not reach the heuristic")
    assert len(f["wide"]) >= 1, "no 256-column fused kernel in the forced context's profile"
    assert np.all(np.isfinite(f["ei"])) and np.all(np.isfinite(f["et"])) and f["ei"].shape[0] == 170 and f["et"].shape[0] == 128
    assert np.array_equal(f["ei"].view(np.uint32), u["ei"].view(np.uint32)), "image embeddings differ: %d elements" % int((f["ei"] != u["ei"]).sum())
    assert np.array_equal(f["et"].view(np.uint32), u["et"].view(np.uint32)), "text embeddings differ: %d elements" % int((f["et"] != u["et"]).sum())
