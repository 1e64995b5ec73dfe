"""End to end: `python -m clip_cpp_amd.image_search build --dtype i8` and `search` over a temporary tree of images with a synthetic
two-tower `tiny` model: the file holds the int8 quantisation of the library's own embeddings, text-query hits match a numpy restatement
of the i8 distance, and an indexed image finds itself."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def quantize(x):
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    amax = np.abs(x).max(1, keepdims=True)
    assert np.all(amax > 0) and np.all(np.isfinite(x))
    return np.rint((x / amax).astype(np.float32) * np.float32(127)).astype(np.int8)


def distances(rows8, q8):
    r = rows8.astype(np.float64)
    q = q8.astype(np.float64).ravel()
    return 1.0 - (r @ q) / np.sqrt((r * r).sum(1)) / np.sqrt((q * q).sum())


def parse_results(stdout):
    lines = stdout.splitlines()
    i = lines.index("search results:")
    assert lines[i + 1] == "distance path"
    out = []
    for line in lines[i + 2:]:
        if not line.startswith("  "):
            break
        d, path = line.strip().split(" ", 1)
        out.append((float(d), path))
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture_cache):
    from PIL import Image
    from oracle import fixtures
    imgs = tmp_path_factory.mktemp("search_i8") / "pictures"
    rng = np.random.default_rng(8)
    made = []
    for sub, ext, n in (("a", "png", 6), ("b/deep", "jpg", 5), ("c", "gif", 3)):
        os.makedirs(imgs / sub, exist_ok=True)
        for i in range(n):
            arr = rng.integers(0, 256, size=(int(rng.integers(20, 70)), int(rng.integers(20, 70)), 3), dtype=np.uint8)
            p = imgs / sub / ("img%d.%s" % (i, ext))
            Image.fromarray(arr).save(p, format={"jpg": "JPEG", "png": "PNG", "gif": "GIF"}[ext])
            made.append(str(p))
    for name in ("red_apple.jpg", "white.jpg"):
        shutil.copy(os.path.join(GOLDEN, name), imgs / name)
        made.append(str(imgs / name))
    return dict(imgs=imgs, made=made, model=fixtures.cached_model(fixture_cache, "tiny", "f32"))


def library_embeddings(clip, clip_lib, paths):
    L = clip_lib.lib()
    arrays = []
    for p in paths:
        im = L.clip_image_u8_make()
        assert L.clip_image_load_from_file(p.encode(), im)
        c = im.contents
        arrays.append(np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy())
        L.clip_image_u8_free(im)
    return clip.encode_images_u8(arrays, normalize=True)


def test_build_and_search_i8(tree, clip_lib, tmp_path):
    from clip_cpp_amd import image_search
    db = tmp_path / "db"
    r = run("build", "-m", tree["model"], "-v", "0", "--dtype", "i8", "--db", db, tree["imgs"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    n = len(tree["made"])
    assert "%d images processed and indexed" % n in r.stdout
    paths = (db / "images.paths").read_text().split("\n")[1:-1]
    assert sorted(paths) == sorted(tree["made"])
    ver, dim, dtype, rows = image_search.read_index_header(str(db / "images.index"))
    assert (ver, dtype, rows) == (1, 3, n)
    assert os.path.getsize(db / "images.index") == 28 + n * dim

    clip = clip_lib.Clip(tree["model"], verbosity=0, device=0)
    emb = library_embeddings(clip, clip_lib, paths)             # one batch, as `build` encodes fewer than 64 images
    assert emb.shape == (n, dim)
    stored = np.fromfile(str(db / "images.index"), dtype=np.int8, offset=28).reshape(n, dim)
    assert np.array_equal(stored, quantize(emb))

    text = "a photo of a red apple"
    r = run("search", "--db", db, "-n", "5", *text.split())
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hits = parse_results(r.stdout)
    assert len(hits) == 5
    q = np.asarray(clip.encode_text(clip.tokenize(text), normalize=True), dtype=np.float32)
    refd = distances(stored, quantize(q))
    tol = dim * 2.0 ** -24 + 1e-6
    order = np.lexsort((np.arange(n), refd))
    kth = refd[order[4]]
    got = [paths.index(p) for _, p in hits]
    for (d, _), i in zip(hits, got):
        assert abs(d - refd[i]) <= tol + 5e-7                 # printed with %f
    for x in set(got) ^ set(order[:5].tolist()):
        assert abs(refd[x] - kth) <= tol
    assert [d for d, _ in hits] == sorted(d for d, _ in hits)

    # an indexed image as the query finds itself first, at the distance of its own quantised embedding
    me = paths[3]
    r = run("search", "--db", db, "-v", "1", me)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hits = parse_results(r.stdout)
    q8 = quantize(library_embeddings(clip, clip_lib, [me]))
    assert hits[0][1] == me and abs(hits[0][0] - distances(stored[3:4], q8)[0]) <= tol + 5e-7
    if np.array_equal(q8[0], stored[3]):
        assert hits[0][0] <= 1e-6
    clip.close()
