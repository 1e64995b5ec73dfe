"""End to end: `python -m clip_cpp_amd.image_search update` (remove the vanished, append the new, encode nothing twice) and
`search --in PREFIX` (subset search) over a small generated tree with a synthetic two-tower `tiny` model."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def hit_lines(stdout):
    """[(printed distance, path)] of the "  %f %s" lines"""
    return [tuple(line.strip().split(" ", 1)) for line in stdout.splitlines() if line.startswith("  ")]


def read_rows(path):
    raw = open(path, "rb").read()
    ver, dim, dt, n = struct.unpack("<IIIQ", raw[8:28])
    assert raw[:8] == b"CLIPIDX1" and ver == 1 and dt == 1 and len(raw) == 28 + n * dim * 2
    return [raw[28 + i * dim * 2: 28 + (i + 1) * dim * 2] for i in range(n)]


def save_image(rng, path):
    from PIL import Image
    arr = rng.integers(0, 256, size=(int(rng.integers(20, 70)), int(rng.integers(20, 70)), 3), dtype=np.uint8)
    Image.fromarray(arr).save(path, format="PNG" if str(path).endswith("png") else "JPEG")


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache):
    """build over 8 images in two sub-directories; then two files deleted, three added, `update`"""
    from oracle import fixtures
    base = tmp_path_factory.mktemp("update")
    imgs, dbdir = base / "pictures", base / "db"
    rng = np.random.default_rng(12)
    old = []
    for sub, ext in (("a", "png"), ("b", "jpg")):
        os.makedirs(imgs / sub)
        for i in range(4):
            save_image(rng, imgs / sub / ("img%d.%s" % (i, ext)))
            old.append(str(imgs / sub / ("img%d.%s" % (i, ext))))
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    r = run("build", "-m", model, "-v", "0", "--db", dbdir, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    before = dict(paths=(dbdir / "images.paths").read_text(), rows=read_rows(dbdir / "images.index"))
    assert before["paths"].split("\n")[1:-1] == old
    deleted = [old[1], old[6]]
    for p in deleted:
        os.remove(p)
    os.makedirs(imgs / "b" / "sub")
    new = [str(imgs / "a" / "new0.png"), str(imgs / "b" / "new1.jpg"), str(imgs / "b" / "sub" / "new2.png")]      # scan order
    for p in new:
        save_image(rng, p)
    r = run("update", "-v", "0", "--db", dbdir, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return dict(imgs=imgs, db=dbdir, old=old, deleted=deleted, new=new, before=before, update_stdout=r.stdout, model=model)


def test_update_reconciles_the_database(db):
    assert "main: 3 added, 2 removed, 6 kept" in db["update_stdout"]
    kept = [p for p in db["old"] if p not in db["deleted"]]
    lines = (db["db"] / "images.paths").read_text().split("\n")
    assert lines[0] == db["model"] and lines[-1] == "" and lines[1:-1] == kept + db["new"]       # survivors in old order, then the new files
    rows = read_rows(db["db"] / "images.index")
    assert len(rows) == 9
    for i, p in enumerate(kept):                                  # nothing already indexed was encoded again: the stored bytes moved
        assert rows[i] == db["before"]["rows"][db["old"].index(p)], p
    printed = db["update_stdout"]
    for p in db["new"]:                                           # each new image finds itself first (the f16 find-self bound)
        r = run("search", "--db", db["db"], "-v", "0", "-n", "9", p)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        hits = hit_lines(r.stdout)
        assert len(hits) == 9 and hits[0][1] == p and float(hits[0][0]) < 4e-3
        printed += r.stdout
    for p in db["deleted"]:
        assert p not in printed
    files = [(db["db"] / f).read_bytes() for f in ("images.index", "images.paths")]
    r = run("update", "-v", "0", "--db", db["db"], db["imgs"])     # nothing changed: nothing to do, nothing rewritten differently
    assert r.returncode == 0 and "main: 0 added, 0 removed, 9 kept" in r.stdout
    assert files == [(db["db"] / f).read_bytes() for f in ("images.index", "images.paths")]


def test_search_in_prefix(db):
    sub = os.path.join(str(db["imgs"]), "b") + os.sep
    under = [p for p in db["old"] + db["new"] if p.startswith(sub) and p not in db["deleted"]]
    assert len(under) == 5
    text = ["a", "photo", "of", "a", "cat"]
    for mode in (["-n", "9"], ["-d", "1.9"]):
        full = run("search", "--db", db["db"], "-v", "1", *mode, *text)
        part = run("search", "--db", db["db"], "-v", "1", "--in", sub, *mode, *text)
        assert full.returncode == 0 and part.returncode == 0, part.stdout[-3000:] + part.stderr[-3000:]
        all_hits, hits = hit_lines(full.stdout), hit_lines(part.stdout)
        assert len(all_hits) == 9 and sorted(p for _, p in hits) == sorted(under)       # only paths under the prefix, all of them
        assert hits == [h for h in all_hits if h[1].startswith(sub)]                    # the same distances, the same order
        assert "search results:" in part.stdout
    two = run("search", "--db", db["db"], "-v", "0", "--in", os.path.join(sub, "sub"), "--in", db["new"][0], "-n", "9", *text)
    assert two.returncode == 0 and sorted(p for _, p in hit_lines(two.stdout)) == sorted([db["new"][0], db["new"][2]])
    for mode in (["-n", "9"], ["-d", "1.9"]):
        none = run("search", "--db", db["db"], "-v", "1", "--in", "/no/such/prefix/", *mode, *text)
        assert none.returncode == 0 and "search results:" in none.stdout and hit_lines(none.stdout) == []
    for p in db["deleted"]:
        assert p not in full.stdout
