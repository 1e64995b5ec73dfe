"""GPU tier: sequences past the whole-row attention kernel (k_attn.hip: 592 keys at d_head 64, 288 at every other head size) run the
streaming kernel of k_attn_long.hip.  Kernel level against a numpy softmax(Q K^T) V, the two kernels against each other where both
apply, run-to-run bit equality, and whole towers at 378 / 448 / 336 px (T = 730 / 1025 / 577) and a 700-position text tower against
the CPU oracle (ggml-faithful numerics), with the tolerances of test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

import attention_common as ac
from oracle import fixtures, ref

pytestmark = pytest.mark.gpu

# 1 - cos(gpu, oracle_faithful), as test_gpu_parity.TOL
TOL = {"f32": 1e-6, "f16": 1e-4, "q4_0": 1e-3, "q5_1": 1e-3}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def one_minus_cos(a, b):
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    return 1.0 - (a * b).sum(-1)


@pytest.fixture(scope="module")
def L(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib.lib()


def attention_ref(qkv, nseq, T, h, nh, causal):
    """softmax(Q K^T) V in float64 on the fp16-rounded inputs; qkv [nseq*T][3h] with Q pre-scaled: the definition and what its element-wise
    fp16 bound is made of (tests/attention_common.py)"""
    return ac.attention_ref_ragged(qkv, ac.uniform_starts(nseq, T), h, nh, causal, True)


def make_qkv(cfg, seed=None):
    nseq, T, h, nh, causal = cfg
    rng = np.random.default_rng(sum(cfg) if seed is None else seed)
    qkv = (rng.standard_normal((nseq * T, 3 * h)) * 0.7).astype(np.float32)
    qkv[:, :h] *= 1.0 / np.sqrt(h // nh)     # q arrives pre-scaled
    return qkv


def run(L, qkv, cfg, kernel=None):
    nseq, T, h, nh, causal = cfg
    out = np.full((nseq * T, h), np.nan, dtype=np.float32)
    if kernel is None:
        rc = L.clip_amd_test_attention(_fp(qkv), nseq, T, h, nh, causal, _fp(out))
    else:
        rc = L.clip_amd_test_attention_ex(_fp(qkv), nseq, T, h, nh, causal, _fp(out), kernel)
    return rc, out


# (nseq, T, h, n_head, causal).  Workgroups take 128 queries where nseq * n_head * ceil(T / 128) >= 256, 64 otherwise: both forms appear.
LONG_SHAPES = [
    (1, 730, 1280, 16, 0),      # ViT-H/14 at 378 px, d_head 80
    (2, 577, 1280, 16, 0),      # ViT-H/14 at 336 px
    (3, 730, 1280, 16, 0),      # (128-query workgroups)
    (1, 1025, 1024, 16, 0),     # ViT-L/14 at 448 px, d_head 64
    (4, 1025, 1024, 16, 0),     # (128-query workgroups)
    (1, 1025, 768, 12, 0),      # ViT-B/16 at 512 px
    (2, 289, 160, 2, 0),        # first length past the d_head-80 limit
    (1, 593, 128, 2, 0),        # first length past the d_head-64 limit
    (1, 300, 64, 2, 0), (2, 450, 64, 2, 1), (64, 300, 64, 2, 1),           # d_head 32
    (1, 640, 176, 2, 0), (1, 1025, 176, 2, 0), (32, 400, 176, 2, 0),      # d_head 88
    (1, 800, 192, 2, 0), (26, 600, 192, 2, 0),                              # d_head 96
    (1, 1025, 208, 2, 0), (48, 300, 208, 2, 0), (1, 577, 1664, 16, 0),     # d_head 104
    (1, 600, 128, 2, 1), (1, 1025, 208, 2, 1), (40, 400, 128, 2, 1),       # causal
]


@pytest.mark.parametrize("cfg", LONG_SHAPES)
def test_long_attention_vs_reference(L, cfg):
    nseq, T, h, nh, causal = cfg
    peaked = ac.make_ragged_qkv([T] * nseq, h, nh, 6, sum(cfg), guard=0)[0]      # score scale 6 and one dominant key per sequence
    for what, qkv in (("flat", make_qkv(cfg)), ("peaked", peaked)):
        rc, out = run(L, qkv, cfg)
        assert rc == 0, rc
        assert np.all(np.isfinite(out))
        defn = attention_ref(qkv, nseq, T, h, nh, causal)
        err = np.abs(out - defn.want).max()
        assert err < 4e-3, (cfg, what, err)
        r = ac.err_over_bound(out, defn, ac.fp16_bound(defn))
        assert r <= 1.0, (cfg, what, "max err / element-wise fp16 bound", r)


AGREE_SHAPES = [(2, T, 2 * dh, 2, 0) for T in (17, 257, 288) for dh in (32, 64, 80, 88, 96, 104)]
AGREE_SHAPES += [(2, T, 2 * dh, 2, 0) for T in (577, 592) for dh in (32, 64)] + [(3, 77, 128, 2, 1), (2, 592, 128, 2, 1), (2, 288, 208, 2, 1)]


@pytest.mark.parametrize("cfg", AGREE_SHAPES)
def test_kernels_agree_where_both_apply(L, cfg):
    nseq, T, h, nh, causal = cfg
    dh = h // nh
    qkv = make_qkv(cfg)
    rc_auto, auto = run(L, qkv, cfg, 0)
    rc_row, whole = run(L, qkv, cfg, 1)
    rc_str, stream = run(L, qkv, cfg, 2)
    assert rc_auto == 0 and rc_str == 0, (rc_auto, rc_str)
    assert np.all(np.isfinite(stream))
    if T > (592 if dh == 64 else 288):
        # the whole-row kernel holds 592 keys at d_head 64 only: d_head 32 past 288 keys is the streaming kernel's
        assert rc_row == -2, rc_row
        assert np.array_equal(auto, stream)
        return
    assert rc_row == 0, rc_row
    assert np.array_equal(auto, whole), "automatic dispatch left the whole-row kernel at T = %d" % T
    u = ac.ulps_at_row_scale(whole, stream, h, nh)
    assert u <= 2.0, (cfg, u)
    assert np.abs(stream - attention_ref(qkv, nseq, T, h, nh, causal).want).max() < 4e-3


@pytest.mark.parametrize("cfg", [(2, 730, 1280, 16, 0), (4, 1025, 1024, 16, 0), (1, 1025, 208, 2, 1)])
def test_long_attention_is_deterministic(L, cfg):
    qkv = make_qkv(cfg)
    rc0, a = run(L, qkv, cfg)
    rc1, b = run(L, qkv, cfg)
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(a, b)


# ---- whole towers against the oracle ----
TXT = fixtures.CONFIGS["tiny"]["t"]
TOWERS = {   # vision-only; the loader wants hidden sizes that are multiples of 64
    "s378_d80": dict(v=dict(S=378, P=14, h=320, L=2, nh=4, ff=256, proj=64), t=TXT),     # T = 730
    "s448_d64": dict(v=dict(S=448, P=14, h=128, L=2, nh=2, ff=256, proj=64), t=TXT),     # T = 1025
    "s336_d104": dict(v=dict(S=336, P=14, h=832, L=2, nh=8, ff=256, proj=64), t=TXT),    # T = 577
}


def _tower(cache, name, ftype):
    import os
    path = os.path.join(cache, "long_%s_%s.gguf" % (name, ftype))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        fixtures.make_model(tmp, TOWERS[name], ftype, text=False, vision=True)
        os.replace(tmp, path)
    return path


@pytest.mark.parametrize("name,ftype", [(n, f) for n in TOWERS for f in ("f16", "q4_0", "q5_1")] + [("s378_d80", "f32")])
def test_long_vision_towers_vs_oracle(clip_lib, fixture_cache, name, ftype):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device")
    path = _tower(fixture_cache, name, ftype)
    clip, orc = clip_lib.Clip(path, device=0), ref.OracleModel(path)
    S = TOWERS[name]["v"]["S"]
    nt = ref.host_cores()
    for n in (1, 3):
        imgs = fixtures.synthetic_images(n, S, seed=60 + n)
        got = clip.encode_images(imgs)
        want = orc.image_batch_encode(imgs, normalize=True, mode=ref.MODE_FAITHFUL, n_threads=nt)
        d = one_minus_cos(got, want)
        assert np.all(np.isfinite(got)) and np.all(d <= TOL[ftype]), (name, ftype, n, float(d.max()))
    if ftype == "f32":
        clip.close()
        return
    # a large batch (large-M GEMM kernels, graph capture at this T): 4 rows against the oracle, every row against the same image in a small batch
    big = fixtures.synthetic_images(40, S, seed=77)
    got = clip.encode_images(big)
    assert np.all(np.isfinite(got))
    rows = [0, 13, 26, 39]
    want = orc.image_batch_encode(big[rows], normalize=True, mode=ref.MODE_FAITHFUL, n_threads=nt)
    d = one_minus_cos(got[rows], want)
    assert np.all(d <= TOL[ftype]), (name, ftype, "B=40", float(d.max()))
    small = np.concatenate([clip.encode_images(big[i:i + 4]) for i in range(0, 40, 4)])
    assert np.all(one_minus_cos(got, small) <= 1e-6), float(one_minus_cos(got, small).max())
    assert np.array_equal(got, clip.encode_images(big))
    # GPU preprocessing at this image size == host preprocessing + encode_images
    rng = np.random.default_rng(5)
    raw = [rng.integers(0, 256, size=(sz[0], sz[1], 3), dtype=np.uint8) for sz in ((S + 37, S - 21), (2 * S, S), (S // 2, S // 3 + 5))]
    host = np.stack([clip.preprocess(im) for im in raw])
    assert np.array_equal(clip.encode_images_u8(raw), clip.encode_images(host))
    clip.close()


def _texts(lens, seed):
    rng = np.random.default_rng(seed)
    out = []
    for ln in lens:
        if ln == 1:
            out.append(np.array([49406], np.int32))
            continue
        ids = rng.integers(0, fixtures.N_VOCAB - 2, size=ln - 2).astype(np.int32)
        out.append(np.concatenate([[49406], ids, [49407]]).astype(np.int32))
    return out


@pytest.mark.parametrize("ftype", ["f16", "q4_0"])
def test_long_ragged_causal_text_tower_vs_oracle(clip_lib, fixture_cache, ftype):
    """700 positions (d_head 64): ragged causal batches past the whole-row kernel's 592 keys through clip_text_batch_encode.  Text
    graphs are keyed on (texts, token rows, 16-key tile bucket of the longest text); the streaming kernel reads every length from the
    device offsets and its grid only depends on that bucket, so a replayed graph serves a batch with other lengths in the same bucket."""
    import os
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device")
    path = os.path.join(fixture_cache, "long_t700_%s.gguf" % ftype)
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        fixtures.make_model(tmp, dict(v=fixtures.CONFIGS["tiny"]["v"], t=dict(h=128, L=2, nh=2, ff=256, proj=64, npos=700)), ftype, text=True, vision=False)
        os.replace(tmp, path)
    clip, orc = clip_lib.Clip(path, device=0), ref.OracleModel(path)
    assert clip.text_config["num_positions"] == 700
    nt = ref.host_cores()
    tol = 6e-4 if ftype.startswith("q") else TOL[ftype]

    def check(texts, what):
        got = clip.encode_texts(texts, normalize=True)
        want = np.stack([orc.text_encode(t, normalize=True, mode=ref.MODE_FAITHFUL, n_threads=nt) for t in texts])
        d = one_minus_cos(got, want)
        assert np.all(np.isfinite(got)) and np.all(d <= tol), (what, float(d.max()), len(texts[int(d.argmax())]))
        return got

    lens = [1, 2, 700, 699, 593, 592, 300, 9, 450, 64]
    texts = _texts(lens, seed=1)
    first = check(texts, "ragged 1..700")
    assert np.array_equal(first, clip.encode_texts(texts, normalize=True))
    for i in (2, 4, 5):      # the text alone: the small-M path for short rows, the tiled one here
        single = np.asarray(clip.encode_text(list(texts[i]), normalize=True), dtype=np.float32)
        assert one_minus_cos(single, first[i]) <= 1e-6, (i, lens[i])
    # graph replay within one key-tile bucket: 1024 rows (the graph limit), longest text 700 then 695 (bucket 44), other lengths
    a = _texts([700, 200, 50, 1, 73], seed=2)
    b = _texts([695, 205, 50, 1, 73], seed=3)
    for _ in range(3):       # captured on the second sighting, replayed on the third
        ga = check(a, "graph A")
    gb = check(b, "graph B (replayed A's graph)")
    assert np.array_equal(ga, clip.encode_texts(a, normalize=True)) and np.array_equal(gb, clip.encode_texts(b, normalize=True))
    # a bucket below the limit next to one above it: 592 keys (whole-row kernel) and 593 (streaming) in one process
    check(_texts([592, 100, 30], seed=4), "max 592")
    check(_texts([593, 100, 30], seed=5), "max 593")
    clip.close()
