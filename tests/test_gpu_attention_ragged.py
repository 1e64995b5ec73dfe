"""GPU tier, kernel level: the three attention kernels (k_attn.hip whole-row, k_attn_long.hip streaming, k_attn_f32.hip) on RAGGED batches
through clip_amd_test_attention_ragged: seq_start on the device, sequences shorter than the launch's max_len (dead key tiles, workgroups that
leave at q0 >= len), the query split over gridDim.y, query-block pairs on short sequences, the 128-query form of the streaming kernel.

Every case asserts: rc == 0; every row inside a sequence is finite and within the ELEMENT-WISE bound of tests/attention_common.py against a
float64 softmax(Q K^T) V (fp16 kernels: the fp16 bound on fp16-rounded inputs; f32 kernel: the f32 bound on the inputs as they are, and at
least 8 times below the fp16 bound of the same data); every guard row (NaN in qkv before seq_start[0] and after seq_start[nseq]) still holds
the sentinel bit for bit; a second run gives identical bits.  Inputs: a flat softmax (scale 1) and a peaked one (scale 6), each with one
query row per sequence whose probability sits on a single key while the others underflow fp16.  The bounds themselves are checked without a
GPU in test_attention_reference_cpu.py (emulated kernel arithmetic inside, planted masking / indexing errors outside).

Observed max err / bound on an MI355X (printed by every case; -s shows them), flat / peaked inputs:
    whole-row kernel   0.66 / 0.64      (fp16 bound; the numpy emulation of the same arithmetic: 0.59 / 0.75)
    streaming kernel   0.63 / 0.62      (fp16 bound)
    f32 kernel         0.028 / 0.034    (f32 bound: a worst-case bound, loose by design; masking and indexing errors are >= 1e-2 against 1e-5 .. 1e-4)
    whole-row against streaming: at most 1.125 fp16 ulps at the row's scale (asserted: 2)

That the cases bite was checked once with masking mutations of the kernels (never committed): k_attn.hip `key < kmax` fails 63 of the 122
cases, `kfull = (len + 15) >> 4` 27 (the non-causal whole-row ones), k_attn_long.hip with raw scores for keys past len 23, k_attn_f32.hip's
`vis` without `key < len` 12.  Dropping the blockIdx.x rotation of the odd last block's wave fails none, and cannot: one slot of [0, nslot)
still takes that block with the same arithmetic; the rotation only balances the SIMDs.
"""
import numpy as np
import pytest

import attention_common as ac

pytestmark = pytest.mark.gpu

AUTO, WHOLE, STREAM, F32 = 0, 1, 2, 3
KNAME = {AUTO: "auto", WHOLE: "whole-row", STREAM: "streaming", F32: "f32"}
SENTINEL_BITS = np.float32(ac.SENTINEL).view(np.uint32)


@pytest.fixture(scope="module")
def L(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib.lib()


def check(L, name, dh, scale, causal, kernel, max_len, uniform=False):
    """One batch through one kernel, every assertion of the module docstring; returns the output."""
    qkv, ss, h, nh = ac.batch(name, dh, scale)
    what = (KNAME[kernel], name, dh, scale, "causal" if causal else "full", max_len)
    run = lambda: ac.run_ragged(L, qkv, None if uniform else ss, max_len, h, nh, causal, kernel, nseq=len(ss) - 1)
    rc, out = run()
    assert rc == 0, (what, rc)
    ref = ac.reference(name, dh, scale, causal, kernel != F32)
    bound = ac.f32_bound(ref) if kernel == F32 else ac.fp16_bound(ref)
    r = ac.err_over_bound(out, ref, bound)
    print("attention err/bound %-9s %-9s d_head %3d scale %d %-6s max_len %4d: %.4f" % (what + (r,)))
    assert r <= 1.0, (what, r)
    if kernel == F32:       # an fp16 step anywhere in this path (inputs, probabilities, output) is an error of the order of the fp16 bound
        r16 = ac.err_over_bound(out, ref, ac.fp16_bound(ref) / 8)
        assert r16 <= 1.0, (what, r16)
    guard = out[~ref.inside]
    assert np.all(guard.view(np.uint32) == SENTINEL_BITS), (what, "guard rows written", int((guard.view(np.uint32) != SENTINEL_BITS).sum()))
    rc2, again = run()
    assert rc2 == 0 and np.array_equal(out.view(np.uint32), again.view(np.uint32)), (what, "second run differs")
    return out


@pytest.mark.parametrize("max_len", [77, 80, 112])      # NT = 5, 5 and 7 (query-block pairs, two dead key tiles)
@pytest.mark.parametrize("kernel", [AUTO, WHOLE])
def test_text_shape_whole_row(L, kernel, max_len):
    for scale in ac.SCALES:
        check(L, "text", 64, scale, 1, kernel, max_len)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", ac.HEAD_SIZES)
@pytest.mark.parametrize("name", ["heads", "heads4"])   # 18 workgroups: queries split over gridDim.y; 72 workgroups: no split
def test_every_head_size_whole_row(L, name, dh, causal):
    for scale in ac.SCALES:
        check(L, name, dh, scale, causal, AUTO, 288)


@pytest.mark.parametrize("causal", [0, 1])
def test_nt37_whole_row(L, causal):
    for scale in ac.SCALES:
        check(L, "nt37", 64, scale, causal, WHOLE, 592)


@pytest.mark.parametrize("max_len", [80, 112])
def test_text_shape_streaming(L, max_len):
    for scale in ac.SCALES:
        check(L, "text", 64, scale, 1, STREAM, max_len)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", ac.HEAD_SIZES)
def test_every_head_size_streaming(L, dh, causal):
    for scale in ac.SCALES:
        check(L, "heads", dh, scale, causal, STREAM, 288)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", [64, 104])
def test_long_ragged_streaming(L, dh, causal):
    for scale in ac.SCALES:
        for kernel in (AUTO, STREAM):
            check(L, "long", dh, scale, causal, kernel, 1025)


@pytest.mark.parametrize("causal", [0, 1])
def test_wide_batch_streaming_128_query_workgroups(L, causal):
    """44 sequences x 2 heads x 3 blocks of 128 queries: most workgroups of the short sequences leave at q0 >= len"""
    for scale in ac.SCALES:
        check(L, "wide", 64, scale, causal, STREAM, 300)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", ac.HEAD_SIZES)
def test_f32_kernel(L, dh, causal):
    for scale in ac.SCALES:
        check(L, "f32", dh, scale, causal, F32, 130)
        check(L, "uniform65", dh, scale, causal, F32, 65, uniform=True)       # seq_start == NULL


WHOLE_AND_STREAM = [("text", 64, 1, 80), ("text", 64, 1, 112), ("nt37", 64, 0, 592), ("nt37", 64, 1, 592), ("wide", 64, 0, 300), ("wide", 64, 1, 300)]
WHOLE_AND_STREAM += [("heads", dh, c, 288) for dh in ac.HEAD_SIZES for c in (0, 1)]


@pytest.mark.parametrize("cfg", WHOLE_AND_STREAM, ids=lambda c: "%s-d%d-%s-%d" % (c[0], c[1], "causal" if c[2] else "full", c[3]))
def test_whole_row_against_streaming(L, cfg):
    name, dh, causal, max_len = cfg
    for scale in ac.SCALES:
        qkv, ss, h, nh = ac.batch(name, dh, scale)
        rc_w, whole = ac.run_ragged(L, qkv, ss, max_len, h, nh, causal, WHOLE)
        rc_s, stream = ac.run_ragged(L, qkv, ss, max_len, h, nh, causal, STREAM)
        assert rc_w == 0 and rc_s == 0, (cfg, rc_w, rc_s)
        inside = ac.reference(name, dh, scale, causal, True).inside
        assert np.all(np.isfinite(whole[inside])) and np.all(np.isfinite(stream[inside]))
        u = ac.ulps_at_row_scale(whole[inside], stream[inside], h, nh)
        print("attention whole-row vs streaming %-6s d_head %3d scale %d %-6s max_len %4d: %.3f fp16 ulps at row scale" % (
            name, dh, scale, "causal" if causal else "full", max_len, u))
        assert u <= 2.0, (cfg, scale, u)


def _alone(L, name, dh, scale, causal, kernel, max_len, batched):
    """every sequence of the batch run alone (nseq = 1, same max_len, another seq_start[0]) reproduces its rows of the batched run"""
    qkv, ss, h, nh = ac.batch(name, dh, scale)
    for i in range(len(ss) - 1):
        r0, r1 = int(ss[i]), int(ss[i + 1])
        before = ac.GUARD + 1 + i
        one = np.full((before + (r1 - r0) + ac.GUARD, 3 * h), np.nan, dtype=np.float32)
        one[before:before + r1 - r0] = qkv[r0:r1]
        rc, out = ac.run_ragged(L, one, [before, before + r1 - r0], max_len, h, nh, causal, kernel)
        assert rc == 0, (KNAME[kernel], name, dh, i, rc)
        same = np.array_equal(out[before:before + r1 - r0].view(np.uint32), batched[r0:r1].view(np.uint32))
        assert same, (KNAME[kernel], name, dh, "causal" if causal else "full", "sequence %d (len %d) alone differs from the batched run" % (i, r1 - r0),
                      float(np.abs(out[before:before + r1 - r0] - batched[r0:r1]).max()))
        rest = np.concatenate([out[:before], out[before + r1 - r0:]])
        assert np.all(rest.view(np.uint32) == SENTINEL_BITS)


@pytest.mark.parametrize("kernel", [WHOLE, STREAM, F32])
def test_text_sequences_do_not_depend_on_the_batch(L, kernel):
    _alone(L, "text", 64, 6, 1, kernel, 80, check(L, "text", 64, 6, 1, kernel, 80))


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", ac.HEAD_SIZES)
@pytest.mark.parametrize("kernel", [WHOLE, STREAM, F32])
def test_sequences_do_not_depend_on_the_batch(L, kernel, dh, causal):
    """The per-query order of operations depends only on the instantiation (NT / the chunk size) and the query's own length; chunks past a
    causal query contribute exact zeros.  The query split, the pairing of query blocks and the 64- / 128-query workgroups only move work."""
    _alone(L, "heads", dh, 6, causal, kernel, 288, check(L, "heads", dh, 6, causal, kernel, 288))


def test_hook_refuses_what_the_kernels_do_not_take(L):
    """-3 before anything launches, `out` untouched: the kernels clamp to row len - 1 and trust their offsets"""
    qkv, ss, h, nh = ac.batch("text", 64, 1)
    rows = qkv.shape[0]
    ss = ss.astype(np.int32)
    bad = {}
    bad["length 0"] = (np.array([128, 130, 130, 140], np.int32), 80)
    bad["length > max_len"] = (ss, 76)
    bad["decreasing offsets"] = (np.array([128, 160, 150, 170], np.int32), 80)
    bad["seq_start[nseq] > rows_total"] = (np.array([rows - 40, rows - 20, rows + 1], np.int32), 80)
    bad["seq_start[0] < 0"] = (np.array([-1, 20, 40], np.int32), 80)
    for kernel in (AUTO, WHOLE, STREAM, F32):
        for what, (starts, max_len) in bad.items():
            rc, out = ac.run_ragged(L, qkv, starts, max_len, h, nh, 1, kernel)
            assert rc == -3, (what, KNAME[kernel], rc)
            assert np.all(out.view(np.uint32) == SENTINEL_BITS), (what, "out was written")
        rc, out = ac.run_ragged(L, qkv, ss, 80, h, 3, 1, kernel)
        assert rc == -3 and np.all(out.view(np.uint32) == SENTINEL_BITS), "h % n_head"
        rc, out = ac.run_ragged(L, qkv, None, 80, h, nh, 1, kernel, nseq=rows // 80 + 1)
        assert rc == -3 and np.all(out.view(np.uint32) == SENTINEL_BITS), "uniform sequences past rows_total"
    # -2: the whole-row kernel holds 288 keys at d_head 32 and 592 at d_head 64
    q32, s32, h32, _ = ac.batch("heads", 32, 1)
    rc, out = ac.run_ragged(L, q32, s32, 289, h32, 2, 0, WHOLE)
    assert rc == -2 and np.all(out.view(np.uint32) == SENTINEL_BITS), rc
    rc, out = ac.run_ragged(L, qkv, ss, 593, h, nh, 1, WHOLE)
    assert rc == -2 and np.all(out.view(np.uint32) == SENTINEL_BITS), rc
