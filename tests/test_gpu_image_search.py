"""End to end: `python -m clip_cpp_amd.image_search build / search` (the reference's examples/image-search on the exact GPU index) over a
temporary tree of images in several formats, the two reference JPEGs and one corrupt file, with a synthetic two-tower `tiny` model."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(*args):
    r = subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    return r


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture_cache):
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("search")
    imgs = base / "pictures"
    rng = np.random.default_rng(4)
    made = []
    for sub, ext, n in (("a", "png", 5), ("a/deep", "jpg", 4), ("b", "gif", 3), ("b", "PNG", 2), ("c", "jpeg", 3)):
        os.makedirs(imgs / sub, exist_ok=True)
        for i in range(n):
            arr = rng.integers(0, 256, size=(int(rng.integers(20, 70)), int(rng.integers(20, 70)), 3), dtype=np.uint8)
            p = imgs / sub / ("img%d.%s" % (i, ext))
            Image.fromarray(arr).save(p, format={"jpg": "JPEG", "jpeg": "JPEG", "png": "PNG", "PNG": "PNG", "gif": "GIF"}[ext])
            made.append(str(p))
    for name in ("red_apple.jpg", "white.jpg"):
        shutil.copy(os.path.join(GOLDEN, name), imgs / name)
        made.append(str(imgs / name))
    (imgs / "c" / "broken.jpg").write_bytes(b"\xff\xd8\xff\xe0 this is not a jpeg")
    (imgs / "c" / "notes.txt").write_text("not an image")
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    return dict(base=base, imgs=imgs, made=made, model=model)


def library_embeddings(clip, clip_lib, paths):
    """decode with the library's loader, encode in one batch (as `build` does for fewer than 64 images), normalised"""
    L = clip_lib.lib()
    arrays = []
    for p in paths:
        im = L.clip_image_u8_make()
        assert L.clip_image_load_from_file(p.encode(), im)
        c = im.contents
        arrays.append(np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy())
        L.clip_image_u8_free(im)
    return clip.encode_images_u8(arrays, normalize=True)


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


def test_build_and_search(tree, clip_lib, tmp_path):
    db = tmp_path / "db"
    r = run("build", "-m", tree["model"], "-v", "1", "--db", db, tree["imgs"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    bad = os.path.join(str(tree["imgs"]), "c", "broken.jpg")
    assert "failed to load image from '%s'" % bad in r.stderr
    n = len(tree["made"])
    assert "%d images processed and indexed" % n in r.stdout
    lines = (db / "images.paths").read_text().split("\n")
    assert lines[0] == tree["model"] and lines[-1] == ""
    paths = lines[1:-1]
    assert sorted(paths) == sorted(tree["made"]) and bad not in paths

    clip = clip_lib.Clip(tree["model"], verbosity=0, device=0)
    emb = library_embeddings(clip, clip_lib, paths)
    nrm = np.sqrt((emb * emb).sum(1, dtype=np.float32))[:, None]
    stored = (emb / nrm).astype(np.float16).astype(np.float64)
    ix = clip_lib.Index.load(clip, str(db / "images.index"))
    assert len(ix) == n and ix.dim == emb.shape[1]
    ix.close()

    text = "a photo of a red apple"
    r = run("search", "--db", db, "-n", "5", *text.split())
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hits = parse_results(r.stdout)
    assert len(hits) == 5
    q = np.asarray(clip.encode_text(clip.tokenize(text), normalize=True), dtype=np.float32)
    q = (q / np.sqrt((q * q).sum(dtype=np.float32))).astype(np.float16).astype(np.float64)
    refd = 1.0 - stored @ q
    tol = emb.shape[1] * 2.0 ** -24 + 1e-6
    order = np.lexsort((np.arange(n), refd))
    kth = refd[order[4]]
    got = [paths.index(p) for _, p in hits]
    for (d, p), i in zip(hits, got):
        assert abs(d - refd[i]) <= tol + 5e-7
    for x in set(got) ^ set(order[:5].tolist()):
        assert abs(refd[x] - kth) <= tol
    assert [d for d, _ in hits] == sorted(d for d, _ in hits)

    # an indexed image as the query finds itself first
    me = paths[3]
    r = run("search", "--db", db, "-v", "1", me)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hits = parse_results(r.stdout)
    assert hits[0][1] == me and hits[0][0] < 1e-3
    clip.close()

    # verbosity 0: the hit lines only, no header
    r = run("search", "--db", db, "-v", "0", "-n", "2", "apple")
    assert r.returncode == 0 and "search results:" not in r.stdout
    assert len([l for l in r.stdout.splitlines() if l.startswith("  ")]) == 2


def test_wrong_tower_models_fail_clearly(tree, fixture_cache, tmp_path):
    from oracle import fixtures
    text_only = fixtures.cached_model(fixture_cache, "tiny", "f32", vision=False)
    r = run("build", "-m", text_only, "--db", tmp_path / "t", tree["imgs"])
    assert r.returncode != 0 and "no vision encoder" in r.stderr
    db = tmp_path / "v"
    vision_only = fixtures.cached_model(fixture_cache, "tiny", "f32", text=False)
    r = run("build", "-m", vision_only, "-v", "0", "--db", db, tree["imgs"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = run("search", "--db", db, "a", "cat")
    assert r.returncode != 0 and "no text encoder" in r.stderr
    r = run("search", "--db", db, "-v", "0", tree["made"][0])      # image queries work on a vision-only model
    hits = [l for l in r.stdout.splitlines() if l.startswith("  ")]
    assert r.returncode == 0 and hits and hits[0].endswith(" " + tree["made"][0])
