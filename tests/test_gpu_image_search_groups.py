"""End to end: `python -m clip_cpp_amd.image_search groups` / `levels` over the seventeen-image tree of
tests/test_gpu_image_search_albums.py (ten images, five byte-identical copies of some of them and two noisy copies; rebuilt here, that file
stays as it is): `groups -n N` prints exactly N groups that partition the database, the groups tree_groups makes of Index.linkage on the
same database, byte-identical files fall into one group; `levels` rows are monotone, end at one group and say what `dedup -d` finds;
--in restricts both; a gridded database is refused; nothing in the database changes."""
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
    base = tmp_path_factory.mktemp("groups")
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
    return dict(db=out, base=base, paths=paths, model=model, same_file=same_file)


def printed_groups(stdout, heading="groups:"):
    """(the groups as lists of (distance text, path), the closing line) of a `groups` or `dedup` run"""
    lines = stdout.splitlines()
    k = lines.index(heading) + 1
    assert lines[-1].startswith("main: ")
    groups = [[]]
    for line in lines[k:-1]:
        if line == "":
            groups.append([])
        else:
            dist, path = line.strip().split(" ", 1)
            groups[-1].append((dist, path))
    return [g for g in groups if g], lines[-1]


def snapshot(d):
    return {f: (open(os.path.join(d, f), "rb").read(), os.stat(os.path.join(d, f)).st_mtime_ns) for f in sorted(os.listdir(d))}


def test_groups_prints_exactly_n_groups_that_partition_the_database(db, clip_lib):
    from clip_cpp_amd.image_search import tree_groups
    paths, same_file = db["paths"], db["same_file"]
    n = len(paths)
    before = snapshot(db["db"])
    clip = clip_lib.Clip(db["model"], verbosity=0)
    index = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    lo, hi, d = index.linkage()
    in_orig = np.array([p.startswith(str(db["base"] / "pictures" / "orig")) for p in paths])
    inside = index.linkage(allow=in_orig)
    index.close()
    clip.close()
    assert len(lo) == n - 1 and in_orig.sum() == 10 and len(inside[0]) == 9

    for want_groups in (5,):
        r = run("groups", "--db", db["db"], "-n", want_groups, "--min", 1)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        groups, closing = printed_groups(r.stdout)
        assert len(groups) == want_groups                                       # exactly N
        members = [path for g in groups for _, path in g]
        assert sorted(members) == sorted(paths)                                 # a partition of the database
        assert [len(g) for g in groups] == sorted((len(g) for g in groups), reverse=True)           # largest first
        expect, kept, cut = tree_groups(n, lo, hi, d, want_groups, min_size=1)
        assert groups == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect]
        assert closing == ("main: %d groups, %d of them with at least 1 images, %d images in those; longest link kept %f, cut at %f"
                           % (want_groups, want_groups, n, kept, cut))
        assert kept <= cut
        group_of = {path: g for g, group in enumerate(groups) for _, path in group}
        for f in np.unique(same_file):                                          # byte-identical files are never split
            assert len({group_of[paths[i]] for i in np.flatnonzero(same_file == f)}) == 1

    r = run("groups", "--db", db["db"], "-n", 12)                              # default --min 2: the singles are counted, not printed
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    groups, closing = printed_groups(r.stdout)
    expect, kept, cut = tree_groups(n, lo, hi, d, 12)
    assert groups == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect] and all(len(g) >= 2 for g in groups)
    assert closing.startswith("main: 12 groups, %d of them with at least 2 images, %d images in those;" % (len(groups), sum(map(len, groups))))
    if kept < cut:                                                             # `dedup -d R` between the two distances finds the same groups
        radius = "%.9g" % kept                                                  # (nine digits: the f32 itself)
        assert float(np.float32(float(radius))) == kept
        rd = run("dedup", "--db", db["db"], "-d", radius)
        assert rd.returncode == 0, rd.stdout[-3000:] + rd.stderr[-3000:]
        dgroups, _ = printed_groups(rd.stdout, "duplicate groups:")
        assert sorted(sorted(p for _, p in g) for g in dgroups) == sorted(sorted(p for _, p in g) for g in groups)

    r = run("groups", "--db", db["db"], "-n", 3, "--min", 1, "--in", db["base"] / "pictures" / "orig", "-v", 0)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "groups:" not in r.stdout
    groups, closing = printed_groups("groups:\n" + r.stdout)
    assert len(groups) == 3 and sorted(p for g in groups for _, p in g) == sorted(p for p, ok in zip(paths, in_orig) if ok)
    expect, kept, cut = tree_groups(n, *inside, 3, eligible=in_orig, min_size=1)
    assert groups == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect]

    r = run("groups", "--db", db["db"], "-n", n + 1)
    assert r.returncode == 1 and "there are only 17 images to group" in r.stderr and "groups:" not in r.stdout
    assert snapshot(db["db"]) == before              # nothing in the database directory changed


def test_levels_rows_are_monotone_and_end_at_one_group(db, clip_lib):
    from clip_cpp_amd.image_search import level_rows
    paths = db["paths"]
    n = len(paths)
    clip = clip_lib.Clip(db["model"], verbosity=0)
    index = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    lo, hi, d = index.linkage()
    table = level_rows(n, lo, hi, d, 6)
    for dist, n_groups, images, largest in table:    # a row says what components (`dedup -d`) finds at its distance
        labels, nearest, _ = index.components(float(np.float32(dist)))
        sizes = np.bincount(labels)
        assert (n_groups, images, largest) == (int((sizes >= 2).sum()), int(sizes[sizes >= 2].sum()), int(sizes.max()))
    index.close()
    clip.close()
    r = run("levels", "--db", db["db"], "-n", 6)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    k = lines.index("levels:")
    assert lines[k + 1] == "distance groups images largest" and lines[-1] == "main: %d images, %d levels" % (n, len(table))
    got = [line.split() for line in lines[k + 2:-1]]
    assert got == [["%f" % dist, str(g), str(i), str(m)] for dist, g, i, m in table]
    assert 2 <= len(got) <= 6
    vals = [(float(a), int(b), int(c), int(e)) for a, b, c, e in got]
    assert all(x[0] <= y[0] and x[2] <= y[2] and x[3] <= y[3] for x, y in zip(vals, vals[1:]))       # monotone
    assert vals[-1][1:] == (1, n, n)                                                                  # ends at one group
    r = run("levels", "--db", db["db"], "--in", db["base"] / "pictures" / "orig", "-v", 0)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert "levels:" not in r.stdout and lines[-1].startswith("main: 10 images, ") and lines[-2].split()[1:] == ["1", "10", "10"]


def test_a_gridded_database_is_refused(db):
    before = snapshot(db["db"])
    gridded = db["base"] / "gridded"
    shutil.copytree(db["db"], gridded)
    (gridded / "images.regions").write_text("grid 2\n")
    r = run("groups", "--db", gridded, "-n", 5)
    assert r.returncode == 1 and "`groups` does not support such a database yet" in r.stderr and "groups:" not in r.stdout
    r = run("levels", "--db", gridded)
    assert r.returncode == 1 and "`levels` does not support such a database yet" in r.stderr and "levels:" not in r.stdout
    assert snapshot(db["db"]) == before
