"""GPU tier: the workspace overlay (forward.cpp carve_tower, CLIP_AMD_WS_ALIAS) moves three pointers and nothing else, so a context loaded with the
switch at 1 and one loaded with it at 0 — same file, same inputs — must return the SAME BITS.  No tolerance appears anywhere.  The layout itself is
checked without a device in tests/test_workspace_plan_cpu.py.

Tiny synthetic models from clip_cpp_amd.synth (T = 17 tokens per image unless stated; 5 images = 85 rows: past the 64-row small-M path, so the GEMM
form with the pruned last layer; 1 image / 1 text: the small-M form)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from clip_cpp_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_T = dict(h=64, L=3, nh=2, ff=256, proj=32, npos=77)
MODELS = {
    # name: (architecture, file type, images for 85 rows or more)
    "ff4h": (dict(v=dict(S=32, P=8, h=64, L=3, nh=2, ff=256, proj=32), t=_T), "q4_0", 5),
    "ff4h_f32": (dict(v=dict(S=32, P=8, h=64, L=3, nh=2, ff=256, proj=32), t=_T), "f32", 5),                      # f32 file: float activations
    "ff2h": (dict(v=dict(S=32, P=8, h=64, L=3, nh=2, ff=128, proj=32), t=dict(_T, ff=128)), "q4_0", 5),             # ff < 4 h: qkv + att make the region
    "ff8h": (dict(v=dict(S=32, P=8, h=64, L=3, nh=2, ff=512, proj=32), t=dict(_T, ff=512)), "q4_0", 5),             # ff > 4 h: mid reaches past att
    # patch 14: K = 588 of Kpad = 640 columns of the im2col matrix are pixels, and col (17 x 4 x 640 fp16) is larger than mid (85 x 256): the
    # region is col's, and the zero columns lie where an earlier call's activations lay
    "p14": (dict(v=dict(S=28, P=14, h=128, L=3, nh=2, ff=256, proj=32), t=_T), "f16", 17),
}


def model_path(cache, name):
    arch, ftype, _ = MODELS[name]
    path = os.path.join(cache, "ws_overlay_%s_%s.gguf" % (name, ftype))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        synth.write_model(tmp, arch, ftype, seed=77)
        os.replace(tmp, path)
    return path


@pytest.fixture(scope="module")
def gpu(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib


def load(gpu, path, alias, **env):
    """a context with CLIP_AMD_WS_ALIAS = alias (and further load-time switches) — the switches are read at load, so the environment is restored at once"""
    env = dict(env, CLIP_AMD_WS_ALIAS=str(alias))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return gpu.Clip(path, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def ws_bytes(gpu, c):
    """bytes of the context's activation workspace (grown on demand: the largest call so far)"""
    head = (C.c_int64 * 5)()
    assert gpu.lib().clip_amd_test_ctx_state(c.ctx, 0, head, None, 0) >= 0
    return int(head[4])


def images(n, S, seed):
    return np.random.default_rng(seed).standard_normal((n, S, S, 3), dtype=np.float32)


def texts(lengths, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[49406], rng.integers(0, synth.N_VOCAB - 2, size=n - 2), [49407]]).astype(np.int32) if n > 1 else np.array([49406], np.int32)
            for n in lengths]


RAGGED = [2, 5, 9, 12, 16, 20, 30]             # 94 rows: the GEMM form; a BOS + EOS pair, and lengths on both sides of the 16-key tile


def same_bits(a, b, what):
    assert a.shape == b.shape and np.all(np.isfinite(a)), what
    bad = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert bad == 0, "%s: %d of %d words differ between CLIP_AMD_WS_ALIAS=1 and =0" % (what, bad, a.size)


def both_towers(c, name, n_img):
    S = MODELS[name][0]["v"]["S"]
    out = {}
    big = images(n_img, S, seed=3)
    for k in range(3):                          # first sighting, capture, replay (batches of <= 32 images go through the graph cache)
        out["img%d_call%d" % (n_img, k)] = c.encode_images(big)
    out["img1"] = c.encode_images(images(1, S, seed=4))
    ragged = texts(RAGGED, seed=5)
    assert sum(len(t) for t in ragged) > 64
    for k in range(3):
        out["txt7_call%d" % k] = c.encode_texts(ragged)
    out["txt1"] = c.encode_texts(texts([9], seed=6))
    return out


@pytest.mark.parametrize("name,env", [("ff4h", {}), ("ff4h", {"CLIP_AMD_LNFOLD": "0"}), ("ff4h_f32", {}), ("ff2h", {}), ("ff8h", {}), ("p14", {})],
                         ids=["ff4h", "ff4h-lnfold0", "f32-file", "ff-below-4h", "ff-above-4h", "patch14"])
def test_overlay_returns_the_bits_of_separate_buffers(gpu, fixture_cache, name, env):
    path = model_path(fixture_cache, name)
    n_img = MODELS[name][2]
    T = (MODELS[name][0]["v"]["S"] // MODELS[name][0]["v"]["P"]) ** 2 + 1
    assert n_img * T >= 85
    on, off = load(gpu, path, 1, **env), load(gpu, path, 0, **env)
    try:
        a, b = both_towers(on, name, n_img), both_towers(off, name, n_img)
        for k in a:
            same_bits(a[k], b[k], "%s %s" % (name, k))
        assert 0 < ws_bytes(gpu, on) < ws_bytes(gpu, off)          # the two contexts did run on different layouts
        for k in a:                              # ... and a replayed graph returns what the eager call returned
            if k.endswith("call1") or k.endswith("call2"):
                same_bits(a[k], a[k[:-1] + "0"], "%s %s against the first call" % (name, k))
    finally:
        on.close()
        off.close()


def test_staged_patch_pieces_and_a_small_batch_behind_a_large_one(gpu, fixture_cache):
    """70 images through clip_image_batch_encode: three copy pieces (32, 32, 6) whose patch stages write disjoint parts of col before the layers
    run once on the whole group.  Then 17 images in the same contexts — the region now holds the large batch's activations — against a fresh context."""
    path = model_path(fixture_cache, "p14")
    S = MODELS["p14"][0]["v"]["S"]
    big, small = images(70, S, seed=8), images(17, S, seed=9)
    on, off, fresh = load(gpu, path, 1), load(gpu, path, 0), load(gpu, path, 1)
    try:
        same_bits(on.encode_images(big), off.encode_images(big), "70 images, staged")
        want = fresh.encode_images(small)
        same_bits(on.encode_images(small), want, "17 images behind 70, overlay")
        same_bits(off.encode_images(small), want, "17 images behind 70, separate buffers")
        tx = texts(RAGGED, seed=10)
        want_t = fresh.encode_texts(tx)
        same_bits(on.encode_texts(tx), want_t, "texts behind images, overlay")
        same_bits(off.encode_texts(tx), want_t, "texts behind images, separate buffers")
    finally:
        for c in (on, off, fresh):
            c.close()


def test_guard_mode_accepts_the_overlay(gpu, fixture_cache, tmp_path):
    """One fresh child with CLIP_AMD_GUARD=1 (canary blocks behind every buffer, the region included; the workspace starts as NaN patterns):
    both towers must return, finite, with the bits of the unguarded context."""
    path = model_path(fixture_cache, "p14")
    S = MODELS["p14"][0]["v"]["S"]
    imgs, tx = images(17, S, seed=11), texts(RAGGED, seed=12)
    np.save(str(tmp_path / "imgs.npy"), imgs)
    np.savez(str(tmp_path / "tx.npz"), *tx)
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, clip_cpp_amd\n"
        "c = clip_cpp_amd.Clip(%r, device=0)\n"
        "tx = np.load(%r)\n"
        "np.save(%r, c.encode_images(np.load(%r)))\n"
        "np.save(%r, c.encode_texts([tx[k] for k in tx.files]))\n"
        "c.close()\n"
        "print('GUARD-OK')\n"
    ) % (ROOT, path, str(tmp_path / "tx.npz"), str(tmp_path / "out_i.npy"), str(tmp_path / "imgs.npy"), str(tmp_path / "out_t.npy"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, errors="replace", timeout=300,
                       env=dict(os.environ, CLIP_AMD_GUARD="1", CLIP_AMD_WS_ALIAS="1"))
    assert r.returncode == 0 and "GUARD-OK" in r.stdout and "CLIP_AMD_GUARD" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    c = load(gpu, path, 1)
    try:
        same_bits(np.load(str(tmp_path / "out_i.npy")), c.encode_images(imgs), "images under the guard")
        same_bits(np.load(str(tmp_path / "out_t.npy")), c.encode_texts(tx), "texts under the guard")
    finally:
        c.close()


def test_vit_b32_q4_0_when_the_fixture_is_cached(gpu, fixture_cache):
    """8 images + 8 texts of the benchmark's model, if a suite or benchmark run has left the file in the fixture cache (it is not generated here)."""
    have = [p for p in (os.path.join(fixture_cache, n) for n in ("synth_b32_q4_0_tv_s1234.gguf", "b32_q4_0_tv_s1234.gguf")) if os.path.exists(p)]
    if not have:
        pytest.skip("no cached ViT-B/32 q4_0 file")
    on, off = load(gpu, have[0], 1), load(gpu, have[0], 0)
    try:
        imgs, tx = images(8, 224, seed=13), texts([77, 2, 9, 33, 40, 41, 16, 17], seed=14)
        same_bits(on.encode_images(imgs), off.encode_images(imgs), "ViT-B/32 q4_0, 8 images")
        same_bits(on.encode_texts(tx), off.encode_texts(tx), "ViT-B/32 q4_0, 8 texts")
    finally:
        on.close()
        off.close()
