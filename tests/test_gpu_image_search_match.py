"""End to end: `python -m clip_cpp_amd.image_search match` over a database built with --grid.  Two images of a small synthetic tree carry
the same distinctive patch, each in another tile of its grid: the two must find each other through that pair of tiles, with both boxes
printed, and never themselves; the patch as a file of its own must find both; a plain build of the same files refuses the command."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 2
SIDE = 96            # tiles of 48 x 48
H = SIDE // 2


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def _smooth(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    f = rng.uniform(0.02, 0.2, size=6)
    img = np.stack([np.sin(xx * f[0] + yy * f[1]), np.cos(xx * f[2] - yy * f[3]), np.sin(xx * f[4]) * np.cos(yy * f[5])], -1)
    return ((img * 0.5 + 0.5) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture_cache):
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("grid_match")
    pics = base / "pictures"
    os.makedirs(pics / "album")
    patch = np.random.default_rng(99).integers(0, 256, size=(H, H, 3), dtype=np.uint8)
    for i in range(6):
        arr = _smooth(i)
        if i == 3:
            arr[0:H, H:SIDE] = patch                    # tile (i = 1, j = 0): x 48 ... 95, y 0 ... 47
        if i == 4:
            arr[H:SIDE, 0:H] = patch                    # tile (i = 0, j = 1): x 0 ... 47, y 48 ... 95
        Image.fromarray(arr).save(pics / ("album" if i % 2 else "") / ("img%d.png" % i), format="PNG")
    query = base / "query.png"
    Image.fromarray(patch).save(query, format="PNG")
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    gdb, pdb = base / "gdb", base / "pdb"
    r = run("build", "-m", model, "-v", "0", "--db", gdb, "--grid", G, pics)
    assert r.returncode == 0 and "main: 6 images processed and indexed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert run("build", "-m", model, "-v", "0", "--db", pdb, pics).returncode == 0
    return dict(gdb=gdb, pdb=pdb, query=query, img3=str(pics / "album" / "img3.png"), img4=str(pics / "img4.png"))


def hits(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [line[2:].split(" ", 1) for line in r.stdout.split("\n") if line.startswith("  ")]


BOX3, BOX4 = "[%d,0,%d,%d]" % (H, H, H), "[0,%d,%d,%d]" % (H, H, H)


def test_indexed_image_finds_the_other_through_the_shared_tile(tree):
    got = hits(run("match", "--db", tree["gdb"], "-v", "0", "-n", "6", tree["img3"]))
    assert len(got) == 5 and got[0][1] == "%s %s <- %s" % (tree["img4"], BOX4, BOX3)       # the stored tile, then the query's own tile
    assert not any(h[1].startswith(tree["img3"]) for h in got)                             # never itself
    assert len(set(h[1].split(" ")[0] for h in got)) == 5                                  # every other image once
    d = [float(h[0]) for h in got]
    assert d == sorted(d) and d[0] < d[1]
    got = hits(run("match", "--db", tree["gdb"], "-v", "0", "-n", "1", tree["img4"]))
    assert len(got) == 1 and got[0][1] == "%s %s <- %s" % (tree["img3"], BOX3, BOX4)


def test_image_file_finds_both(tree):
    got = hits(run("match", "--db", tree["gdb"], "-v", "0", "-n", "6", tree["query"]))
    assert len(got) == 6
    # the whole query image is the patch: it meets the two tiles; no " <- " box, the query row is the whole file
    assert sorted(h[1] for h in got[:2]) == sorted(["%s %s" % (tree["img3"], BOX3), "%s %s" % (tree["img4"], BOX4)])
    assert float(got[1][0]) < float(got[2][0])


def test_every_image(tree):
    r = run("match", "--db", tree["gdb"], "-n", "2")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    text = r.stdout[r.stdout.index("matches:\n") + len("matches:\n"):]
    body, tail = text.rsplit("main:", 1)
    assert tail.strip() == "6 images, 2 matches each"
    blocks = [b.split("\n") for b in body.strip("\n").split("\n\n")]
    paths = (tree["gdb"] / "images.paths").read_text().split("\n")[1:-1]
    assert [b[0] for b in blocks] == paths                                                 # one block per image, in id order
    for b in blocks:
        assert len(b) == 3 and all(line.startswith("  ") for line in b[1:])
        assert not any(line[2:].split(" ", 1)[1].startswith(b[0]) for line in b[1:])       # no image in its own block
    by_path = {b[0]: b[1:] for b in blocks}
    assert by_path[tree["img3"]][0].endswith("%s %s <- %s" % (tree["img4"], BOX4, BOX3))
    assert by_path[tree["img4"]][0].endswith("%s %s <- %s" % (tree["img3"], BOX3, BOX4))


def test_plain_database_is_refused(tree):
    for extra in ([], [tree["img3"]]):
        r = run("match", "--db", tree["pdb"], *extra)
        assert r.returncode == 1 and "was not built with --grid" in r.stderr and str(tree["pdb"]) in r.stderr
        assert "search --like" in r.stderr and "neighbors" in r.stderr and not r.stdout.strip()
