"""End to end: `python -m clip_cpp_amd.image_search spread` over the seventeen-image tree of tests/test_gpu_image_search_albums.py (ten
images, five byte-identical copies of some of them and two noisy copies; rebuilt here, that file stays as it is): the printed lines are
spread_lines of Index.spread on the same database, -n, -d, --in and --from do what they say, the byte-identical copies of a chosen image
are picked last and are owned by it, a gridded database and an unknown --from path are refused, and nothing in the database changes."""
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
    base = tmp_path_factory.mktemp("spread")
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
    content = {}
    same_file = np.array([content.setdefault(open(p, "rb").read(), len(content)) for p in paths])      # equal: byte-identical files
    assert sorted(np.bincount(same_file).tolist()) == [1] * 9 + [2, 3, 3]
    return dict(db=out, base=base, paths=paths, model=model, same_file=same_file)


def printed(stdout, verbose=True):
    """(the lines of the picks, the closing line) of a `spread` run"""
    lines = stdout.splitlines()
    k = lines.index("spread:") + 1 if verbose else 0
    assert lines[-1].startswith("main: ")
    return lines[k:-1], lines[-1]


def closing(result):
    return "main: %d images, every other image within %f of one of them" % (len(result[0]), result[4])


def snapshot(d):
    return {f: (open(os.path.join(d, f), "rb").read(), os.stat(os.path.join(d, f)).st_mtime_ns) for f in sorted(os.listdir(d))}


def test_spread_prints_the_lines_of_index_spread(db, clip_lib):
    from clip_cpp_amd.image_search import spread_lines
    paths, same_file = db["paths"], db["same_file"]
    n = len(paths)
    before = snapshot(db["db"])
    clip = clip_lib.Clip(db["model"], verbosity=0)
    index = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    whole = index.spread(n)
    twelve = index.spread(12)
    reach = whole[1].astype(np.float64)
    # a stop radius inside the widest step of the reach sequence among the picks of distinct files
    t = 1 + int(np.argmax(reach[1:11] - reach[2:12]))
    stop = "%.9g" % ((reach[t] + reach[t + 1]) / 2)
    assert reach[t + 1] < float(np.float32(float(stop))) < reach[t]
    stopped = index.spread(n, float(stop))
    in_orig = np.array([p.startswith(str(db["base"] / "pictures" / "orig")) for p in paths])
    assert in_orig.sum() == 10
    inside = index.spread(4, allow=in_orig)
    seeds = [paths.index(p) for p in paths if p.endswith(("z/zz7.png", "orig/img4.png"))][::-1]
    seeded = index.spread(5, seeds=seeds)
    index.close()
    clip.close()

    r = run("spread", "--db", db["db"], "-n", n)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert printed(r.stdout) == (spread_lines(whole[0], whole[1], whole[2], paths), closing(whole))
    assert printed(r.stdout)[0][0] == "inf %s (+0)" % paths[0] and printed(r.stdout)[1].startswith("main: 17 images, every other image within 0.000000")
    # every file's content is picked before any second copy of one: the five byte-identical copies come last, at the distance of a row
    # from itself (zero but for the rounding of the norm)
    print("reach:", " ".join("%.3g" % v for v in whole[1]))
    assert len(set(same_file[whole[0][:12]].tolist())) == 12
    assert np.abs(whole[1][12:]).max() < whole[1][1:12].min() and np.abs(whole[1][12:]).max() <= 4 * 2.0 ** -23      # a few ulp of 1

    r = run("spread", "--db", db["db"], "-n", 12)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert printed(r.stdout) == (spread_lines(twelve[0], twelve[1], twelve[2], paths), closing(twelve))
    assert np.array_equal(twelve[0], whole[0][:12])
    rest = np.setdiff1d(np.arange(n), twelve[0])
    assert np.array_equal(same_file[twelve[2][rest]], same_file[rest])       # each copy is owned by the chosen image with its bytes
    assert np.all(twelve[2][rest] < rest)                                        # ... the lowest id of them
    assert sum(int(line.rsplit("(+", 1)[1][:-1]) for line in printed(r.stdout)[0]) == 5

    r = run("spread", "--db", db["db"], "-n", n, "-d", stop, "-v", "0")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "spread:" not in r.stdout and len(stopped[0]) == t + 1
    assert printed(r.stdout, verbose=False) == (spread_lines(stopped[0], stopped[1], stopped[2], paths), closing(stopped))

    r = run("spread", "--db", db["db"], "-n", 4, "--in", db["base"] / "pictures" / "orig")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert printed(r.stdout) == (spread_lines(inside[0], inside[1], inside[2], paths), closing(inside))
    assert np.all(in_orig[inside[0]]) and np.all(inside[2][~in_orig] == -1) and sum(int(line.rsplit("(+", 1)[1][:-1]) for line in printed(r.stdout)[0]) == 6

    r = run("spread", "--db", db["db"], "-n", 5, "--from", paths[seeds[0]], "--from", paths[seeds[1]])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert printed(r.stdout) == (spread_lines(seeded[0], seeded[1], seeded[2], paths), closing(seeded))
    assert seeded[0][:2].tolist() == seeds and [line.split(" ")[0] for line in printed(r.stdout)[0][:3]].count("inf") == 2

    r = run("spread", "--db", db["db"], "-n", 5, "--from", "no/such/image.png")
    assert r.returncode == 1 and "'no/such/image.png' is not in the database" in r.stderr and "spread:" not in r.stdout
    gridded = db["base"] / "gridded"
    shutil.copytree(db["db"], gridded)
    (gridded / "images.regions").write_text("grid 2\n")
    r = run("spread", "--db", gridded, "-n", 5)
    assert r.returncode == 1 and "`spread` does not support such a database yet" in r.stderr and "spread:" not in r.stdout
    assert snapshot(db["db"]) == before              # nothing in the database directory changed
