"""End to end: `python -m clip_cpp_amd.image_search dedup` and `search -d` over a tree that holds byte-identical copies of some images in
other directories next to distinct images, against the connected components computed in numpy from the library's own embeddings of the
same files (the synthetic `tiny` model gives no natural distances, so the radius is chosen from those embeddings)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache):
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("dedup")
    imgs = base / "pictures"
    rng = np.random.default_rng(12)
    originals = []
    for i in range(10):
        os.makedirs(imgs / "orig", exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        p = imgs / "orig" / ("img%d.png" % i)
        Image.fromarray(arr).save(p, format="PNG")
        originals.append(p)
    for src, dst in ((0, "copies/a/x0.png"), (0, "copies/b/y0.png"), (3, "copies/a/x3.png"), (7, "z/z7.png")):
        os.makedirs((imgs / dst).parent, exist_ok=True)
        shutil.copy(originals[src], imgs / dst)
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    r = run("build", "-m", model, "-v", "0", "--db", out, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    return dict(db=out, paths=paths, model=model)


def stored_embeddings(clip_lib, model, paths):
    """the library's own embeddings of the files (one batch, as `build` encodes fewer than 64 images), in the stored f16 form"""
    clip = clip_lib.Clip(model, verbosity=0, device=0)
    L = clip_lib.lib()
    arrays = []
    for p in paths:
        im = L.clip_image_u8_make()
        assert L.clip_image_load_from_file(p.encode(), im)
        c = im.contents
        arrays.append(np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy())
        L.clip_image_u8_free(im)
    emb = clip.encode_images_u8(arrays, normalize=True)
    single = clip.encode_images_u8(arrays[:1], normalize=True)[0]     # a query image is encoded on its own
    clip.close()

    def f16(v):
        v = np.atleast_2d(np.asarray(v, np.float32))
        nrm = np.sqrt((v * v).sum(1, dtype=np.float32))[:, None]
        return (v / nrm).astype(np.float16).astype(np.float64)
    return f16(emb), f16(single)[0]


def query_vector(clip, clip_lib, path):
    """the f32 query `search` makes of an image: the file decoded by the library, encoded on its own, normalised"""
    L = clip_lib.lib()
    im = L.clip_image_u8_make()
    assert L.clip_image_load_from_file(path.encode(), im)
    c = im.contents
    arr = np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    L.clip_image_u8_free(im)
    return clip.encode_images_u8([arr], normalize=True)[0]


def choose_radius(dist, same, tol):
    """a radius in a gap of the pair distances at least 8 tol wide, above every byte-identical pair when the distances allow"""
    iu = np.triu_indices(dist.shape[0], 1)
    v = np.unique(dist[iu])
    floor = dist[same].max()
    for lo, hi in zip(v[:-1], v[1:]):
        if lo >= floor and hi - lo > 8 * tol:
            return float((lo + hi) / 2)
    pytest.fail("no gap in the pair distances of the tree's embeddings")


def components(dist, radius):
    n = dist.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a in range(n):
        for b in range(a + 1, n):
            if dist[a, b] <= radius:
                ra, rb = find(a), find(b)
                parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for x in range(n):
        groups.setdefault(find(x), []).append(x)
    return [g for r, g in sorted(groups.items()) if len(g) > 1]


def parse_groups(stdout):
    lines = stdout.splitlines()
    i = lines.index("duplicate groups:")
    groups, cur = [], []
    for line in lines[i + 1:]:
        if line.startswith("main: "):
            break
        if not line:
            groups.append(cur)
            cur = []
            continue
        assert line.startswith("  "), line
        d, p = line.strip().split(" ", 1)
        cur.append((float(d), p))
    if cur:
        groups.append(cur)
    return groups, lines[-1]


def test_dedup_groups_match_numpy_components(db, clip_lib):
    paths = db["paths"]
    emb, _ = stored_embeddings(clip_lib, db["model"], paths)
    dist = 1.0 - emb @ emb.T
    name = lambda p: open(p, "rb").read()
    same = np.array([[a != b and name(paths[a]) == name(paths[b]) for b in range(len(paths))] for a in range(len(paths))])
    assert same.sum() == 2 * 5                    # 3 copies of img0 (3 pairs), 2 of img3 (1), 2 of img7 (1)
    tol = emb.shape[1] * 2.0 ** -24 + 1e-6
    radius = choose_radius(dist, same, tol)
    want = components(dist, radius)
    r = run("dedup", "--db", db["db"], "-d", "%.9g" % radius)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got, last = parse_groups(r.stdout)
    assert [[p for _, p in g] for g in got] == [[paths[x] for x in g] for g in want]
    assert last == "main: %d groups, %d images" % (len(want), sum(len(g) for g in want))
    for g, w in zip(got, want):
        for (d, _), x in zip(g, w):
            nearest = min(dist[x, y] for y in w if y != x)
            assert abs(d - nearest) <= tol + 5e-7
    for a in range(len(paths)):                  # every byte-identical copy is grouped with its original
        for b in np.nonzero(same[a])[0]:
            assert any(a in g and b in g for g in want)
    r0 = run("dedup", "--db", db["db"], "-v", "0", "--max-distance", "%.9g" % radius)
    assert r0.returncode == 0 and "duplicate groups:" not in r0.stdout
    assert r0.stdout.splitlines()[-1] == last
    r = run("dedup", "--db", db["db"], "-d", "-1")
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "main: 0 groups, 0 images"


def test_search_max_distance_prints_every_image_within(db, clip_lib):
    paths = db["paths"]
    emb, q = stored_embeddings(clip_lib, db["model"], paths)
    dist = 1.0 - emb @ q                          # the query: the first indexed image, encoded on its own as `search` does
    tol = emb.shape[1] * 2.0 ** -24 + 1e-6
    v = np.sort(dist)
    gaps = [(hi - lo, (lo + hi) / 2) for lo, hi in zip(v[:-1], v[1:]) if hi - lo > 8 * tol]
    assert gaps
    radius = float(max(gaps)[1]) if len(gaps) == 1 else float(sorted(gaps, key=lambda g: g[1])[len(gaps) // 2][1])
    r = run("search", "--db", db["db"], "-d", "%.9g" % radius, paths[0])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    k = lines.index("search results:")
    assert lines[k + 1] == "distance path"
    hits = [(float(l.split(" ", 3)[2]), l.split(" ", 3)[3]) for l in lines[k + 2:] if l.startswith("  ")]
    want = [paths[x] for x in np.lexsort((np.arange(len(paths)), dist)) if dist[x] <= radius]
    assert sorted(p for _, p in hits) == sorted(want)
    assert [d for d, _ in hits] == sorted(d for d, _ in hits)
    for d, p in hits:
        assert abs(d - dist[paths.index(p)]) <= tol + 5e-7
    # without -d: exactly the -n nearest of Index.search, in the format `search` printed before -d existed
    r = run("search", "--db", db["db"], "-n", "3", paths[0])
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    k = lines.index("search results:")
    clip = clip_lib.Clip(db["model"], verbosity=0, device=0)
    ix = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    sd, si = ix.search(query_vector(clip, clip_lib, paths[0])[None, :], 3)
    ix.close()
    clip.close()
    assert lines[k:] == ["search results:", "distance path"] + ["  %f %s" % (d, paths[i]) for d, i in zip(sd[0], si[0])]
