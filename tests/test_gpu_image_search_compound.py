"""End to end: `python -m clip_cpp_amd.image_search search --and TERM --not TERM` over a small tree of synthetic images with the tiny
two-tower model.  The expected listing is composed in this process from Index.search_compound over the terms encoded here the way the
command encodes them (every text in one encode_texts call, every image file in one batch; an indexed image is its stored row)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def hits_of(r):
    """[(distance text, path)] of a search run"""
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
def db(tmp_path_factory, fixture_cache, clip_lib):
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("compound")
    imgs = base / "pictures"
    os.makedirs(imgs / "a")
    os.makedirs(imgs / "b")
    rng = np.random.default_rng(33)

    def picture(path):
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        Image.fromarray(arr).save(path, format="PNG")

    for i in range(12):
        picture(imgs / ("a" if i % 2 == 0 else "b") / ("img%02d.png" % i))
    picture(base / "outside.png")                                         # an image file that is not indexed
    picture(base / "other.png")
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", out, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 12
    clip = clip_lib.Clip(model, verbosity=0)
    index = clip_lib.Index.load(clip, str(out / "images.index"))
    yield dict(db=out, paths=paths, clip=clip, index=index, outside=str(base / "outside.png"), other=str(base / "other.png"), lib=clip_lib)
    index.close()
    clip.close()


def encode_texts(db, texts):
    clip = db["clip"]
    return np.asarray(clip.encode_texts([clip.tokenize(t) for t in texts], normalize=True), dtype=np.float32)


def encode_files(db, files):
    from clip_cpp_amd import image_search
    L = db["lib"].lib()
    imgs = [L.clip_image_u8_make() for _ in files]
    try:
        for path, im in zip(files, imgs):
            assert L.clip_image_load_from_file(os.fsencode(path), im)
        return image_search._encode_batch(db["clip"], L, imgs)
    finally:
        for im in imgs:
            L.clip_image_u8_free(im)


def lines_of(db, query, k, allow=None):
    dist, ids = db["index"].search_compound([query], k, allow=allow, exclude_terms=True)
    return [("%f" % d, db["paths"][i]) for d, i in zip(dist[0], ids[0]) if i >= 0]


def test_and_not_print_the_lines_of_search_compound(db):
    t = encode_texts(db, ["a red apple", "on a table", "people"])
    f = encode_files(db, [db["outside"]])
    for margin, value in (("-4", -4.0), ("0", 0.0), ("0.001", 0.001)):   # -4: every image passes the --not terms; the others may drop some
        got = hits_of(run("search", "--db", db["db"], "-n", "6", "--and", "on a table", "--not", "people", "--not", db["outside"], "--not-margin", margin,
                          "a", "red", "apple"))
        query = [(t[0], "all"), (t[1], "all"), (t[2], "over", value), (f[0], "over", value)]
        assert got == lines_of(db, query, 6), margin
        assert len(got) == 6 or value >= 0
    got = hits_of(run("search", "--db", db["db"], "-n", "6", "--and", "on a table", "--not", "people", "a red apple"))      # the default margin: 0
    assert got == lines_of(db, [(t[0], "all"), (t[1], "all"), (t[2], "over")], 6)
    # --and alone, ranked by the worst term: not the ranking of either term alone
    got = hits_of(run("search", "--db", db["db"], "-n", "12", "--and", "on a table", "a red apple"))
    t2 = encode_texts(db, ["a red apple", "on a table"])
    assert got == lines_of(db, [(t2[0], "all"), (t2[1], "all")], 12) and len(got) == 12
    both = db["index"].search(t2, 12)
    worst = np.maximum(both[0][0][np.argsort(both[1][0])], both[0][1][np.argsort(both[1][1])])
    assert [p for _, p in got] == [db["paths"][i] for i in np.lexsort((np.arange(12), worst))]
    # an image file as the main query and as a term: one batch
    f2 = encode_files(db, [db["outside"], db["other"]])
    got = hits_of(run("search", "--db", db["db"], "-n", "4", "--and", db["other"], db["outside"]))
    assert got == lines_of(db, [(f2[0], "all"), (f2[1], "all")], 4) and len(got) == 4


def test_an_indexed_path_is_its_stored_row_and_is_not_listed(db):
    a, b = db["paths"][3], db["paths"][8]
    t = encode_texts(db, ["at night"])
    got = hits_of(run("search", "--db", db["db"], "-n", "12", "--and", a, "at night"))
    assert got == lines_of(db, [(t[0], "all"), (3, "all")], 12)
    assert len(got) == 11 and a not in [p for _, p in got]
    got = hits_of(run("search", "--db", db["db"], "-n", "12", "--like", a, "--and", b, "--not", "at night", "--not-margin", "-4"))
    assert got == lines_of(db, [(3, "all"), (8, "all"), (t[0], "over", -4.0)], 12)
    listed = [p for _, p in got]
    assert len(got) == 10 and a not in listed and b not in listed
    # the stored rows, as --like takes them: the single-term ranking of --like is search_ids'
    like = hits_of(run("search", "--db", db["db"], "-n", "5", "--like", a))
    dist, ids = db["index"].search_ids([3], 5)
    assert like == [("%f" % d, db["paths"][i]) for d, i in zip(dist[0], ids[0])]


def test_in_restricts_the_results(db):
    t = encode_texts(db, ["a red apple", "on a table"])
    prefix = os.path.dirname(db["paths"][0]) + os.sep
    allow = np.array([p.startswith(prefix) for p in db["paths"]])
    assert 0 < allow.sum() < 12
    got = hits_of(run("search", "--db", db["db"], "-n", "12", "--in", prefix, "--and", "on a table", "a red apple"))
    assert got == lines_of(db, [(t[0], "all"), (t[1], "all")], 12, allow=allow)
    assert len(got) == allow.sum() and all(p.startswith(prefix) for _, p in got)


def test_a_plain_search_prints_what_it_printed(db):
    clip = db["clip"]
    vec = np.asarray(clip.encode_text(clip.tokenize("a red apple"), n_threads=4, normalize=True), dtype=np.float32)
    dist, ids = db["index"].search(vec[None, :], 5)
    got = hits_of(run("search", "--db", db["db"], "a red apple"))
    assert got == [("%f" % d, db["paths"][i]) for d, i in zip(dist[0], ids[0])]


def test_usage_errors(db):
    r = run("search", "--db", db["db"], "--and", "x", "-d", "0.5", "a cat")
    assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search search" in r.stdout and "cannot be combined with -d or --distinct" in r.stdout
    r = run("search", "--db", db["db"], *sum([["--and", "t%d" % i] for i in range(8)], []), "a cat")
    assert r.returncode == 1 and "at most 8 terms" in r.stdout
