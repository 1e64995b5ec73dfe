"""End to end: `python -m clip_cpp_amd.image_search albums` over a tree of ten images, five byte-identical copies of some of them (the tree
of tests/test_gpu_image_search_prune.py) and two noisy copies: the printed albums are album_groups of Index.modes on the same database, a
family of copies has its lowest id as the cover, --min and -n cut the list, and nothing in the database changes."""
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
    base = tmp_path_factory.mktemp("albums")
    imgs = base / "pictures"
    rng = np.random.default_rng(12)
    originals, arrays = [], []
    for i in range(10):
        os.makedirs(imgs / "orig", exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        p = imgs / "orig" / ("img%d.png" % i)
        Image.fromarray(arr).save(p, format="PNG")
        originals.append(p)
        arrays.append(arr)
    for src, dst in ((0, "copies/a/x0.png"), (0, "copies/b/y0.png"), (3, "copies/a/x3.png"), (7, "z/z7.png"), (7, "z/zz7.png")):
        os.makedirs((imgs / dst).parent, exist_ok=True)
        shutil.copy(originals[src], imgs / dst)
    for src, dst in ((2, "zz_noisy/n2.png"), (7, "zz_noisy/n7.png")):       # a few grey levels of noise: far nearer than any other image
        os.makedirs((imgs / dst).parent, exist_ok=True)
        noisy = np.clip(arrays[src].astype(np.int16) + rng.integers(-8, 9, size=arrays[src].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(imgs / dst, format="PNG")
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    # f32 rows: the synthetic `tiny` model embeds any two images within about 1e-3 of each other, which f16 rows would round away
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", out, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 17
    family = np.array([int("".join(c for c in os.path.basename(p) if c.isdigit())) for p in paths])      # the image a file was made from
    return dict(db=out, paths=paths, model=model, family=family)


def choose_radius(db):
    """a radius in a gap of the stored rows' pair distances at least 8 tol wide, above every pair of one family (an image, its byte-identical
    copies and its noisy copy) and below every other pair; returns it with the matrix "same family, another file" """
    import struct
    p = str(db["db"] / "images.index")
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    assert dt == 0 and n == len(db["paths"])
    emb = np.fromfile(p, dtype=np.float32, offset=28).reshape(n, dim).astype(np.float64)
    dist = 1.0 - emb @ emb.T
    fam = db["family"]
    same = (fam[:, None] == fam[None, :]) & ~np.eye(n, dtype=bool)
    assert sorted(np.bincount(fam).tolist()) == [1] * 6 + [2, 2, 3, 4]
    tol = dim * 2.0 ** -24 + 1e-6
    lo, hi = dist[same].max(), dist[~same & ~np.eye(n, dtype=bool)].min()
    print("one family at most %.3g apart, other images at least %.3g, tol %.3g" % (lo, hi, tol))
    assert hi - lo > 8 * tol, "no gap between the families' distances and the other pairs'"
    return float((lo + hi) / 2), same


def printed_albums(stdout, paths):
    """(albums as album_groups gives them, with printed distances as text; the closing line) of an `albums` run at verbosity > 0"""
    lines = stdout.splitlines()
    k = lines.index("albums:")
    assert lines[-1].startswith("main: ")
    ids = {p: i for i, p in enumerate(paths)}
    albums = []
    for line in lines[k + 1:-1]:
        if line == "":
            continue
        if line.startswith("  "):
            d, path = line[2:].split(" ", 1)
            albums[-1][1].append((ids[path], d))
        else:
            albums.append((ids[line], []))
    blanks = sum(1 for line in lines[k + 1:-1] if line == "")
    assert blanks == max(len(albums) - 1, 0)      # albums are separated by one blank line
    return albums, lines[-1]


def as_printed(groups):
    return [(cover, [(i, "%f" % d) for i, d in members]) for cover, members in groups]


def snapshot(d):
    return {f: (open(os.path.join(d, f), "rb").read(), os.stat(os.path.join(d, f)).st_mtime_ns) for f in sorted(os.listdir(d))}


def test_albums_prints_the_groups_of_index_modes(db, clip_lib):
    from clip_cpp_amd import image_search
    paths = db["paths"]
    n = len(paths)
    radius, same = choose_radius(db)
    R = "%.9g" % radius
    before = snapshot(db["db"])
    clip = clip_lib.Clip(db["model"], verbosity=0)
    index = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    results = {link: index.modes(float(R), None if link is None else float(link)) for link in (None, "1")}
    index.close()
    clip.close()

    # link = radius: only the files of one family are linked, every family is a clique of equal densities, so its lowest id is the cover
    labels, parent, pdist, density = results[None]
    r = run("albums", "--db", db["db"], "-d", R)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got, closing = printed_albums(r.stdout, paths)
    assert got == as_printed(image_search.album_groups(labels, pdist, 2))
    assert closing == "main: 4 albums, 11 images"
    families = {}
    for x in range(n):
        families.setdefault(int(db["family"][x]), []).append(x)
    want = sorted(([m[0], m[1:]] for m in families.values()), key=lambda a: (-len(a[1]), a[0]))      # largest first, then by cover id
    assert [len(m) for _, m in want] == [3, 2, 1, 1] + [0] * 6
    assert [[c, [i for i, _ in m]] for c, m in got] == want[:4]
    assert np.array_equal(density, same.sum(1))

    # --min 1 lists the single images too, --min 3 only the two larger families, -n the first COUNT of the list
    r = run("albums", "--db", db["db"], "-d", R, "--min", "1")
    assert r.returncode == 0 and printed_albums(r.stdout, paths) == (as_printed(image_search.album_groups(labels, pdist, 1)), "main: 10 albums, 17 images")
    assert [[c, [i for i, _ in m]] for c, m in printed_albums(r.stdout, paths)[0]] == want
    r = run("albums", "--db", db["db"], "-d", R, "--min", "3")
    assert r.returncode == 0 and printed_albums(r.stdout, paths) == (got[:2], "main: 2 albums, 7 images")
    r = run("albums", "--db", db["db"], "-d", R, "-n", "1")
    assert r.returncode == 0 and printed_albums(r.stdout, paths) == (got[:1], "main: 1 albums, 4 images")
    r = run("albums", "--db", db["db"], "-d", R, "-v", "0")
    assert r.returncode == 0 and "albums:" not in r.stdout and r.stdout.splitlines()[-1] == "main: 4 albums, 11 images"

    # a link that reaches everything: one album under the top-ranked image, the lowest id of the largest family
    labels, parent, pdist, density = results["1"]
    r = run("albums", "--db", db["db"], "-d", R, "--link", "1")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got, closing = printed_albums(r.stdout, paths)
    assert got == as_printed(image_search.album_groups(labels, pdist, 2)) and closing == "main: 1 albums, 17 images"
    assert got[0][0] == want[0][0]
    assert snapshot(db["db"]) == before              # nothing in the database directory changed
