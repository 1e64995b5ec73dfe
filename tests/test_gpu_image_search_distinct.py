"""End to end: `python -m clip_cpp_amd.image_search search --distinct R` over a tree in which three images are saved twice (the same
picture encoded again into a second file).  The radius comes from the database's own `dedup` output (the synthetic `tiny` model gives no
natural distances), and the expected listing is the definition (tests/distinct_common.py: walk) applied to the ranking that the same
command prints without --distinct."""
import os
import subprocess
import sys

import numpy as np
import pytest

from distinct_common import walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPIED = (0, 3, 5)


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def hits_of(r):
    """[(distance text, rest of the line)] of a search run"""
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    k = lines.index("search results:")
    assert lines[k + 1] == "distance path"
    out = []
    for line in lines[k + 2:]:
        assert line.startswith("  "), line
        d, rest = line[2:].split(" ", 1)
        out.append((d, rest))
    return out


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache):
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("distinct")
    imgs = base / "pictures"
    os.makedirs(imgs / "shots")
    os.makedirs(imgs / "copies")
    rng = np.random.default_rng(21)
    for i in range(7):
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        Image.fromarray(arr).save(imgs / "shots" / ("img%d.png" % i), format="PNG")
        if i in COPIED:                                                   # the same picture encoded again: other bytes, the same pixels
            Image.fromarray(arr).save(imgs / "copies" / ("img%d.png" % i), format="PNG", compress_level=1)
            assert (imgs / "copies" / ("img%d.png" % i)).read_bytes() != (imgs / "shots" / ("img%d.png" % i)).read_bytes()
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", out, imgs)      # f32 rows: a copy is closer than the f16 rounding
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 10
    pairs = [(str(imgs / "copies" / ("img%d.png" % i)), str(imgs / "shots" / ("img%d.png" % i))) for i in COPIED]
    # the radius: every image with the distance to its nearest other image (dedup at a radius that holds everything), then the middle
    # of the gap between the copies and the rest; at that radius dedup must list exactly the three pairs
    r = run("dedup", "--db", out, "-d", "2")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    nearest = {}
    for line in r.stdout.splitlines():
        if line.startswith("  "):
            d, p = line.strip().split(" ", 1)
            nearest[p] = float(d)
    assert set(nearest) == set(paths)
    copies = {p for pair in pairs for p in pair}
    lo, hi = max(nearest[p] for p in copies), min(nearest[p] for p in paths if p not in copies)
    assert lo < hi, "the copies are not closer to their originals than distinct pictures are to each other: %r" % (nearest,)
    radius = "%.9g" % ((lo + hi) / 2)
    r = run("dedup", "--db", out, "-v", "0", "-d", radius)
    groups = [sorted(l.strip().split(" ", 1)[1] for l in g.splitlines() if l.startswith("  ")) for g in r.stdout.split("\n\n")]
    assert sorted(g for g in groups if g) == sorted(sorted(p) for p in pairs), r.stdout
    return dict(db=out, paths=paths, pairs=pairs, radius=radius, query=pairs[1][1])


def expected_lines(ranking, pairs, k):
    """the walk over a printed ranking [(distance text, path)] with the copy pairs as the near relation"""
    order = {p: t for t, (_, p) in enumerate(ranking)}
    near = {(min(order[a], order[b]), max(order[a], order[b])) for a, b in pairs if a in order and b in order}
    kept, counts = walk(range(len(ranking)), near, k)
    return [(ranking[t][0], ranking[t][1] + (" (+%d)" % c if c > 0 else "")) for t, c in zip(kept, counts)]


def test_search_distinct_lists_each_copy_pair_once(db):
    full = hits_of(run("search", "--db", db["db"], "-n", "10", db["query"]))
    assert len(full) == 10 and not any("(+" in p for _, p in full)
    plain = hits_of(run("search", "--db", db["db"], "-n", "5", db["query"]))
    assert plain == full[:5]                                              # without --distinct: both copies, no suffix
    listed = [p for _, p in plain]
    assert db["pairs"][1][0] in listed and db["pairs"][1][1] in listed
    got = hits_of(run("search", "--db", db["db"], "--distinct", db["radius"], "-n", "5", db["query"]))
    assert got == expected_lines(full, db["pairs"], 5) and len(got) == 5
    assert got[0][1].endswith(" (+1)")                                    # the query's own picture stands for its copy
    every = hits_of(run("search", "--db", db["db"], "--distinct", db["radius"], "-n", "7", db["query"]))
    assert every == expected_lines(full, db["pairs"], 7) and len(every) == 7
    assert sum(p.endswith(" (+1)") for _, p in every) == 3
    for a, b in db["pairs"]:                                              # each pair once
        assert sum(p in (a, b, a + " (+1)", b + " (+1)") for _, p in every) == 1
    none = hits_of(run("search", "--db", db["db"], "--distinct", "-1", "-n", "5", db["query"]))
    assert none == plain                                                  # R < 0 folds nothing


def test_like_with_distinct(db):
    full = hits_of(run("search", "--db", db["db"], "--like", db["query"], "-n", "10"))
    assert len(full) == 9 and db["query"] not in [p for _, p in full]
    got = hits_of(run("search", "--db", db["db"], "--like", db["query"], "--distinct", db["radius"], "-n", "7"))
    assert got == expected_lines(full, db["pairs"], 7)
    assert sum(p.endswith(" (+1)") for _, p in got) == 2                  # the query itself is not in the pool: its copy stands alone
    assert (full[0][0], db["pairs"][1][0]) in got
    sub = hits_of(run("search", "--db", db["db"], "--like", db["query"], "--distinct", db["radius"], "--in", os.path.dirname(db["query"]), "-n", "7"))
    assert [p for _, p in sub] == [p for _, p in full if p.startswith(os.path.dirname(db["query"]))]      # --in: the copies are not eligible


def test_distinct_with_max_distance_is_a_usage_error(db):
    r = run("search", "--db", db["db"], "--distinct", db["radius"], "-d", "0.5", db["query"])
    assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search search" in r.stdout and "--distinct and -d cannot be combined" in r.stdout
