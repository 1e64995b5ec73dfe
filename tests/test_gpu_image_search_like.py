"""End to end: `python -m clip_cpp_amd.image_search search --like PATH` and `neighbors` over a small database built by `build`: the lines
printed are the results of Index.search_ids / Index.knn_graph on the loaded index, the queried image is never listed, --in restricts the
candidates."""
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
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache, clip_lib):
    """a database of 8 images (two JPEGs of tests/golden, six generated PNGs in two directories) and its index, loaded"""
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("like")
    imgs = base / "pictures"
    rng = np.random.default_rng(9)
    for sub in ("a", "b"):
        os.makedirs(imgs / sub)
        for i in range(3):
            arr = rng.integers(0, 256, size=(int(rng.integers(20, 60)), int(rng.integers(20, 60)), 3), dtype=np.uint8)
            Image.fromarray(arr).save(imgs / sub / ("img%d.png" % i), format="PNG")
    for name in ("red_apple.jpg", "white.jpg"):
        shutil.copy(os.path.join(GOLDEN, name), imgs / "b" / name)
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    r = run("build", "-m", model, "-v", "0", "--db", base / "db", imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (base / "db" / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 8
    clip = clip_lib.Clip(model, verbosity=0, device=0)
    ix = clip_lib.Index.load(clip, str(base / "db" / "images.index"))
    yield dict(dir=base / "db", paths=paths, index=ix, prefix_b=str(imgs / "b") + os.sep)
    ix.close()
    clip.close()


def hit_lines(stdout):
    return [l for l in stdout.splitlines() if l.startswith("  ")]


def test_search_like(db):
    paths, ix = db["paths"], db["index"]
    for me in (paths[0], paths[5], paths[7]):
        r = run("search", "--db", db["dir"], "--like", me, "-n", "3")
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        dist, ids = ix.search_ids([paths.index(me)], 3)
        assert hit_lines(r.stdout) == ["  %f %s" % (d, paths[i]) for d, i in zip(dist[0], ids[0])]
        assert "search results:" in r.stdout and all(not l.endswith(" " + me) for l in hit_lines(r.stdout))
    # --in: only paths under the prefix, still without the image itself
    me = paths.index(db["prefix_b"] + "white.jpg")
    allow = np.array([p.startswith(db["prefix_b"]) for p in paths])
    r = run("search", "--db", db["dir"], "-v", "0", "--in", db["prefix_b"], "--like", paths[me], "-n", "8")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    dist, ids = ix.search_ids([me], 8, allow=allow)
    want = ["  %f %s" % (d, paths[i]) for d, i in zip(dist[0], ids[0]) if i >= 0]
    assert hit_lines(r.stdout) == want and len(want) == int(allow.sum()) - 1
    assert all(l.split(" ", 3)[3].startswith(db["prefix_b"]) for l in want) and "search results:" not in r.stdout
    r = run("search", "--db", db["dir"], "--like", "pictures/nowhere.png")
    assert r.returncode == 1 and "is not in the database" in r.stderr


def test_neighbors(db):
    paths, ix = db["paths"], db["index"]
    r = run("neighbors", "--db", db["dir"], "-n", "2")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    dist, ids = ix.knn_graph(2)
    want = ["neighbours:"]
    for i, p in enumerate(paths):
        if i:
            want.append("")
        want.append(p)
        want += ["  %f %s" % (d, paths[j]) for d, j in zip(dist[i], ids[i])]
    want.append("main: 8 images, 2 neighbours each")
    lines = r.stdout.splitlines()
    assert lines[lines.index("neighbours:"):] == want
    r = run("neighbors", "--db", db["dir"], "-v", "0")
    assert r.returncode == 0 and "neighbours:" not in r.stdout and r.stdout.splitlines()[-1] == "main: 8 images, 5 neighbours each"
    assert len(hit_lines(r.stdout)) == 8 * 5
