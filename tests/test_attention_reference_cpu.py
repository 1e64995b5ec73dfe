"""The attention tests' own reference and bounds (tests/attention_common.py), checked without a GPU on every input set that
test_gpu_attention_ragged.py runs: numpy emulations of the kernels' arithmetic (fp16: whole-row and streaming order, with and without
subnormal flush; f32: sequential FMA chains and key-by-key accumulation) stay inside the element-wise bounds, and the bounds are sharp:
four planted errors of the kind a kernel makes (causal mask off by one, the last partial key tile left unmasked, one key dropped, V of one
key read from the neighbouring sequence) are rejected on every input set, flat and peaked.  Last, the host-side argument checks of the
test hook itself, which need the library but no device."""
import numpy as np
import pytest

import attention_common as ac

FP16_SETS = ac.fp16_sets()
F32_SETS = ac.f32_sets()
_id = lambda s: "%s-d%d-%s" % (s[0], s[1], "causal" if s[2] else "full")


def test_input_sets_are_what_the_kernels_paths_need():
    qkv, ss, h, nh = ac.batch("text", 64, 6)
    assert ss[0] == ac.GUARD and qkv.shape == (2 * ac.GUARD + sum(ac.TEXT_LENS), 3 * h)
    assert np.isnan(qkv[:ss[0]]).all() and np.isnan(qkv[ss[-1]:]).all() and np.isfinite(qkv[ss[0]:ss[-1]]).all()
    assert list(np.diff(ss)) == ac.TEXT_LENS
    # the 128-query workgroup form of the streaming kernel: n_seq * n_head * ceil(max_len / 128) >= 256
    assert len(ac.WIDE_LENS) * 2 * ((max(ac.WIDE_LENS) + 127) // 128) >= 256
    # a peaked row: one key holds the whole probability in fp16, the rest underflow
    ref = ac.reference("heads", 64, 1, 0, True)
    assert (ref.psub > 0).any() and (ref.psub[ref.inside] == 0).any()


def test_reference_matches_dense_softmax():
    """the looped reference against a dense one-line softmax on a uniform batch"""
    nseq, T, h, nh = 3, 19, 64, 2
    qkv, ss = ac.make_ragged_qkv([T] * nseq, h, nh, 1, 5, guard=0)
    for causal in (0, 1):
        ref = ac.attention_ref_ragged(qkv, ss, h, nh, causal, True)
        x = ac.h16(qkv).astype(np.float64).reshape(nseq, T, 3, nh, h // nh)
        s = np.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1])
        if causal:
            s = np.where(np.triu(np.ones((T, T), dtype=bool), 1), -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        dense = np.einsum("bhqk,bkhd->bqhd", p, x[:, :, 2]).reshape(nseq * T, h)
        np.testing.assert_allclose(ref.want, dense, rtol=1e-12, atol=1e-14)
        assert ref.inside.all() and (ref.pabs >= np.abs(ref.want) - 1e-15).all()


@pytest.mark.parametrize("cfg", FP16_SETS, ids=_id)
def test_fp16_emulation_inside_bound_and_plants_outside(cfg):
    name, dh, causal = cfg
    for scale in ac.SCALES:
        qkv, ss, h, nh = ac.batch(name, dh, scale)
        ref = ac.reference(name, dh, scale, causal, True)
        bound = ac.fp16_bound(ref)
        for flush in (False, True):
            for chunk in (None, 64):
                r = ac.err_over_bound(ac.emulate_fp16(qkv, ss, h, nh, causal, flush, chunk), ref, bound)
                assert r <= 1.0, (cfg, scale, flush, chunk, r)
        for plant in ac.PLANTS:
            if plant == "causal_off_by_one" and not causal:
                continue        # (without the causal mask this plant is "the last key dropped": drop_key covers it)
            bad = ac.attention_ref_ragged(qkv, ss, h, nh, causal, True, plant=plant)
            r = ac.err_over_bound(bad.want, ref, bound)
            assert r > 1.0, (cfg, scale, plant, r)


@pytest.mark.parametrize("cfg", F32_SETS, ids=_id)
def test_f32_emulation_inside_bound_and_plants_outside(cfg):
    name, dh, causal = cfg
    for scale in ac.SCALES:
        qkv, ss, h, nh = ac.batch(name, dh, scale)
        ref = ac.reference(name, dh, scale, causal, False)
        bound = ac.f32_bound(ref)
        got = ac.emulate_f32(qkv, ss, h, nh, causal)
        r = ac.err_over_bound(got, ref, bound)
        assert r <= 1.0, (cfg, scale, r)
        # what the GPU test asserts next to the bound: an f32 result is far inside the fp16 bound of the same data
        assert ac.err_over_bound(got, ref, ac.fp16_bound(ref) / 8) <= 1.0
        # ... and a result with one fp16 step in it (the probabilities, or the inputs) is not
        assert ac.err_over_bound(ac.emulate_fp16(qkv, ss, h, nh, causal, False), ref, ac.fp16_bound(ref) / 8) > 1.0
        for plant in ac.PLANTS:
            if plant == "causal_off_by_one" and not causal:
                continue
            bad = ac.attention_ref_ragged(qkv, ss, h, nh, causal, False, plant=plant)
            assert ac.err_over_bound(bad.want, ref, bound) > 1.0, (cfg, scale, plant)


def test_hook_checks_its_arguments_before_it_looks_for_a_device(clip_lib):
    """clip_amd_test_attention_ragged refuses a batch outside the kernels' contract with -3 on the host: the answer is the same with and
    without a GPU (no device would be -1), so nothing can have been launched, and `out` comes back untouched."""
    L = clip_lib.lib()
    qkv, ss, h, nh = ac.batch("text", 64, 1)
    rows = qkv.shape[0]
    bad = [("length 0", [128, 130, 130, 140], 80, nh), ("length > max_len", ss, 76, nh), ("decreasing offsets", [128, 160, 150, 170], 80, nh),
           ("seq_start[nseq] > rows_total", [rows - 40, rows - 20, rows + 1], 80, nh), ("seq_start[0] < 0", [-1, 20, 40], 80, nh),
           ("h % n_head", ss, 80, 3)]
    for kernel in range(4):
        for what, starts, max_len, heads in bad:
            rc, out = ac.run_ragged(L, qkv, starts, max_len, h, heads, 1, kernel)
            assert rc == -3, (what, kernel, rc)
            assert np.all(out == np.float32(ac.SENTINEL)), (what, "out was written")
    assert ac.run_ragged(L, qkv, ss, 80, h, nh, 1, 4)[0] == -3, "kernel 4 does not exist"
    assert ac.run_ragged(L, qkv, None, 80, h, nh, 1, 0, nseq=rows // 80 + 1)[0] == -3, "uniform sequences past rows_total"
    assert ac.run_ragged(L, qkv, None, 80, h, nh, 1, 0, nseq=0)[0] == -3, "no sequence"
