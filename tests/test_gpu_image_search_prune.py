"""End to end: `python -m clip_cpp_amd.image_search dedup --prune` over a tree of ten images and five byte-identical copies of some of them
(the tree of tests/test_gpu_dedup_cli.py): of every group only the lowest id stays in the database, the image files stay on disk, and the
pruned database has no duplicates left, searches only kept paths and is not rewritten by a second prune."""
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
    base = tmp_path_factory.mktemp("prune")
    imgs = base / "pictures"
    rng = np.random.default_rng(12)
    originals = []
    for i in range(10):
        os.makedirs(imgs / "orig", exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        p = imgs / "orig" / ("img%d.png" % i)
        Image.fromarray(arr).save(p, format="PNG")
        originals.append(p)
    for src, dst in ((0, "copies/a/x0.png"), (0, "copies/b/y0.png"), (3, "copies/a/x3.png"), (7, "z/z7.png"), (7, "z/zz7.png")):
        os.makedirs((imgs / dst).parent, exist_ok=True)
        shutil.copy(originals[src], imgs / dst)
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    # f32 rows: the synthetic `tiny` model embeds any two images within 1e-4 of each other, below the rounding of f16 rows
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", out, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 15
    return dict(db=out, paths=paths, model=model)


def choose_radius(clip_lib, db):
    """a radius in a gap of the stored rows' pair distances at least 8 tol wide, above every byte-identical pair and below every other"""
    import struct
    p = str(db["db"] / "images.index")
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    assert dt == 0 and n == len(db["paths"])
    emb = np.fromfile(p, dtype=np.float32, offset=28).reshape(n, dim).astype(np.float64)
    dist = 1.0 - emb @ emb.T
    blob = [open(q, "rb").read() for q in db["paths"]]
    same = np.array([[a != b and blob[a] == blob[b] for b in range(n)] for a in range(n)])
    assert same.sum() == 2 * 7                    # three files of img0 and of img7 (3 pairs each), two of img3 (1)
    tol = dim * 2.0 ** -24 + 1e-6
    lo, hi = dist[same].max(), dist[~same & ~np.eye(n, dtype=bool)].min()
    print("copies at most %.3g apart, other images at least %.3g, tol %.3g" % (lo, hi, tol))
    assert hi - lo > 8 * tol, "no gap between the copies' distances and the other pairs'"
    return float((lo + hi) / 2), same


def test_prune_keeps_the_lowest_id_of_every_group(db, clip_lib):
    paths = db["paths"]
    radius, same = choose_radius(clip_lib, db)
    R = "%.9g" % radius
    keep = [x for x in range(len(paths)) if not np.any(same[x, :x])]       # no earlier byte-identical file
    assert len(keep) == 10
    before = run("dedup", "--db", db["db"], "-d", R)
    assert before.returncode == 0 and before.stdout.splitlines()[-1] == "main: 3 groups, 8 images"
    r = run("dedup", "--prune", "--db", db["db"], "-d", R)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "main: 5 removed, 10 kept"
    k = lines.index("duplicate groups:")                                     # the groups as `dedup` prints them
    assert lines[k:-1] == before.stdout.splitlines()[before.stdout.splitlines().index("duplicate groups:"):-1]
    after = (db["db"] / "images.paths").read_text().split("\n")
    assert after[0] == db["model"] and after[-1] == "" and after[1:-1] == [paths[x] for x in keep]
    from clip_cpp_amd import image_search
    assert image_search.read_index_header(str(db["db"] / "images.index"))[3] == 10      # the index's size matches
    assert all(os.path.exists(p) for p in paths)                             # files on disk are never touched
    assert not [f for f in os.listdir(db["db"]) if f.endswith(".tmp")]
    r = run("dedup", "--db", db["db"], "-d", R)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "main: 0 groups, 0 images"
    r = run("search", "--db", db["db"], "-n", "10", paths[0])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hits = [l.split(" ", 3)[3] for l in r.stdout.splitlines() if l.startswith("  ")]
    assert sorted(hits) == sorted(paths[x] for x in keep)
    files = [db["db"] / "images.paths", db["db"] / "images.index"]
    stamps = [os.stat(f).st_mtime_ns for f in files]
    r = run("dedup", "--prune", "-v", "0", "--db", db["db"], "-d", R)      # nothing to remove: nothing is rewritten
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "main: 0 removed, 10 kept"
    assert "duplicate groups:" not in r.stdout
    assert [os.stat(f).st_mtime_ns for f in files] == stamps
