"""End to end: `python -m clip_cpp_amd.image_search build --grid G` and `search` over it.  One image of a small synthetic tree carries a
distinctive patch confined to one tile of the grid; a query with exactly that patch must list the image once, first, with the tile's
box, while a plain build of the same files lists whole images without a box and writes the files the code path without --grid writes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 2
SIDE = 96            # tiles of 48 x 48


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
    base = tmp_path_factory.mktemp("grid_search")
    pics = base / "pictures"
    os.makedirs(pics / "album")
    patch = np.random.default_rng(99).integers(0, 256, size=(SIDE // 2, SIDE // 2, 3), dtype=np.uint8)
    for i in range(6):
        arr = _smooth(i)
        if i == 3:
            arr[0:SIDE // 2, SIDE // 2:SIDE] = patch                  # tile (i = 1, j = 0): x 48 ... 95, y 0 ... 47
        Image.fromarray(arr).save(pics / ("album" if i % 2 else "") / ("img%d.png" % i), format="PNG")
    query = base / "query.png"
    Image.fromarray(patch).save(query, format="PNG")
    return dict(base=base, pics=pics, query=query, target=str(pics / "album" / "img3.png"),
                model=fixtures.cached_model(fixture_cache, "tiny", "f32"))


def hits(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [line[2:].split(" ", 1) for line in r.stdout.split("\n") if line.startswith("  ")]


def test_gridded_build_and_search(tree, clip_lib):
    from clip_cpp_amd import image_search
    gdb, pdb = tree["base"] / "gdb", tree["base"] / "pdb"
    r = run("build", "-m", tree["model"], "-v", "0", "--db", gdb, "--grid", G, tree["pics"])
    assert r.returncode == 0 and "main: 6 images processed and indexed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (gdb / "images.paths").read_text().split("\n")
    assert paths[0] == tree["model"] and len(paths) == 8 and paths[-1] == "" and tree["target"] in paths      # one line per image
    R = 1 + G * G
    grid, rows = image_search.read_regions(str(gdb))
    assert grid == G and rows.shape == (6 * R, 5)
    assert image_search.read_index_header(str(gdb / "images.index"))[3] == 6 * R
    boxes = clip_lib.grid_boxes(SIDE, SIDE, G)
    for i in range(6):
        assert np.all(rows[i * R:(i + 1) * R, 0] == i) and np.array_equal(rows[i * R:(i + 1) * R, 1:], boxes)
    assert not [f for f in os.listdir(gdb) if f.endswith(".tmp")]

    # the patch as the query: the image once, first, with the tile's box; every image at most once
    got = hits(run("search", "--db", gdb, "-v", "0", "-n", "6", tree["query"]))
    assert len(got) == 6 and got[0][1] == "%s [%d,0,%d,%d]" % (tree["target"], SIDE // 2, SIDE // 2, SIDE // 2)
    names = [h[1].split(" [")[0] for h in got]
    assert sorted(names) == sorted(paths[1:-1])
    d = [float(h[0]) for h in got]
    assert d == sorted(d) and d[0] < d[1]                              # the tile holds the query's pixels: the same embedding but for f16 storage
    # --in selects the rows of the matching images
    got = hits(run("search", "--db", gdb, "-v", "0", "-n", "6", "--in", str(tree["pics"] / "album"), tree["query"]))
    assert len(got) == 3 and got[0][1].startswith(tree["target"] + " [") and all("/album/" in h[1] for h in got)

    # a plain build of the same files, into a directory that holds a regions file of an earlier gridded build: whole images, no box
    os.makedirs(pdb)
    (pdb / "images.regions").write_text((gdb / "images.regions").read_text())
    assert run("build", "-m", tree["model"], "-v", "0", "--db", pdb, tree["pics"]).returncode == 0
    got = hits(run("search", "--db", pdb, "-v", "0", "-n", "6", tree["query"]))
    assert len(got) == 6 and not any("[" in h[1] for h in got)
    # ... and its files are what the code path without --grid writes: the same library calls, made here
    clip = clip_lib.Clip(tree["model"], verbosity=0, device=0)
    files = image_search.image_files(str(tree["pics"]))
    vecs, ok, consumed = clip.encode_image_files(clip.ImageFileList(files), normalize=True, n_threads=4, max_images=image_search.BATCH, start=0)
    assert ok.all() and consumed == 6
    ix = clip_lib.Index(clip, clip.vision_config["projection_dim"], dtype="f16")
    ix.add(vecs)
    ix.save(str(tree["base"] / "ref.index"))
    ix.close()
    clip.close()
    want_index = (tree["base"] / "ref.index").read_bytes()
    want_paths = "".join(p + "\n" for p in [tree["model"]] + files)
    assert sorted(os.listdir(pdb)) == ["images.index", "images.paths"]
    assert (pdb / "images.index").read_bytes() == want_index and (pdb / "images.paths").read_text() == want_paths
