"""End to end: `python -m clip_cpp_amd.image_search file` and `audit` over a small synthetic database built by `build`: three folders of
generated PNGs, a pixel-identical copy of one folder's image planted in another folder, and the reference's red apple.  The lines `file`
prints are Index.vote_ids (an indexed path) or Index.vote of the re-encoded image (an outside file) over the folder labels; `audit` lists
the planted copy with the other copy as its witness; with --labels FILE the unlisted images ask but never vote.

The commands run in this process with one image per encoder batch (image_search.BATCH = 1), as in tests/test_gpu_image_search_cross.py:
an embedding is bit-identical between two batches only when both use the same GEMM kernels."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def cli(clip_lib):
    """run(capfd, args...) -> (exit code, stdout, stderr) of image_search.main"""
    from clip_cpp_amd import image_search
    old = image_search.BATCH
    image_search.BATCH = 1

    def run(capfd, *args):
        capfd.readouterr()
        rc = image_search.main([str(a) for a in args])
        out = capfd.readouterr()
        return rc, out.out, out.err

    yield run
    image_search.BATCH = old


@pytest.fixture(scope="module")
def library(tmp_path_factory, fixture_cache):
    """pictures/{a,b,c}: three generated PNGs each; b also holds the reference's red apple, c a pixel-identical copy of a/img0.png.
    outside.jpg, next to the folders, is the red apple again: a file the database does not hold."""
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("file")
    imgs = base / "pictures"
    rng = np.random.default_rng(23)
    for sub in ("a", "b", "c"):
        os.makedirs(imgs / sub)
        for i in range(3):
            arr = rng.integers(0, 256, size=(int(rng.integers(20, 60)), int(rng.integers(20, 60)), 3), dtype=np.uint8)
            Image.fromarray(arr).save(imgs / sub / ("img%d.png" % i), format="PNG")
    shutil.copy(os.path.join(GOLDEN, "red_apple.jpg"), imgs / "b" / "red_apple.jpg")
    shutil.copy(imgs / "a" / "img0.png", imgs / "c" / "copy.png")
    shutil.copy(os.path.join(GOLDEN, "red_apple.jpg"), base / "outside.jpg")
    return dict(base=base, imgs=imgs, model=fixtures.cached_model(fixture_cache, "tiny", "f32"))


@pytest.fixture(scope="module")
def db(cli, library, clip_lib):
    """the database (f32 rows: a pixel-identical copy is then at about 1e-7 of its original, far below the distances between the
    generated images), its paths, the open index and the folder labels"""
    from clip_cpp_amd import image_search
    d = library["base"] / "db"

    class Capture:                                            # the module-scoped build needs no captured output
        def readouterr(self):
            class O:
                out = err = ""
            return O()

    rc, out, err = cli(Capture(), "build", "-m", library["model"], "-v", "0", "--dtype", "f32", "--db", d, library["imgs"])
    assert rc == 0
    paths = (d / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 11
    clip = clip_lib.Clip(library["model"], verbosity=0, device=0)
    index = clip_lib.Index.load(clip, str(d / "images.index"))
    labels, names = image_search.read_labels(paths)
    assert len(names) == 3 and sorted(os.path.basename(n) for n in names) == ["a", "b", "c"]
    yield dict(dir=d, paths=paths, index=index, labels=labels, names=names, clip=clip)
    index.close()
    clip.close()


def find(paths, tail):
    (i,) = [i for i, p in enumerate(paths) if p.endswith(tail)]
    return i


def lines_of(res, r, counted, names, paths):
    return ["  %d/%d %f %s ~ %s" % (v, counted, d, names[c], paths[j]) for c, v, d, j in zip(res[0][r], res[1][r], res[2][r], res[3][r]) if c >= 0]


def embed(clip, clip_lib, path):
    """decode with the library's loader and encode in a batch of one, as `file` does"""
    L = clip_lib.lib()
    im = L.clip_image_u8_make()
    assert L.clip_image_load_from_file(str(path).encode(), im)
    c = im.contents
    arr = np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    L.clip_image_u8_free(im)
    return clip.encode_images_u8([arr], normalize=True)


def test_file_of_indexed_paths(cli, db, capfd):
    paths, labels, names, index = db["paths"], db["labels"], db["names"], db["index"]
    copy, apple, orig = find(paths, "c/copy.png"), find(paths, "b/red_apple.jpg"), find(paths, "a/img0.png")
    for k, n, m in ((4, 2, 2), (None, None, 3), (1, 5, 1)):
        extra = (["-k", k] if k else []) + (["-n", n] if n else [])
        k = k or 10
        rc, out, err = cli(capfd, "file", "--db", db["dir"], *extra, paths[copy], paths[apple])
        assert rc == 0, out[-3000:] + err[-3000:]
        res = index.vote_ids([copy, apple], k, labels, m=m)
        counted = min(k, 10)                                  # 11 labelled images, the asked one does not vote
        want = ["filing:", paths[copy]] + lines_of(res, 0, counted, names, paths) + ["", paths[apple]] + lines_of(res, 1, counted, names, paths)
        want.append("main: 2 images, %d voters each" % k)
        lines = out.splitlines()
        assert lines[lines.index("filing:"):] == want
        assert not any(l.endswith("~ " + paths[copy]) for l in want[2:2 + m])      # an image never votes for itself
        assert not any(l.endswith("~ " + paths[apple]) for l in want[-1 - m:-1])
    # the nearest other image of the copy is its original, in folder a, at distance ~0
    assert lines[lines.index("filing:") + 2] == "  1/1 %f %s ~ %s" % (res[2][0, 0], os.path.dirname(paths[orig]), paths[orig])
    assert abs(res[2][0, 0]) < 1e-6                           # (f32 rows: 1 - the dot of a row with itself, a rounding error of zero)
    rc, out, err = cli(capfd, "file", "--db", db["dir"], "-v", "0", paths[copy])
    assert rc == 0 and "filing:" not in out and out.splitlines()[-1] == "main: 1 images, 10 voters each"


def test_file_of_an_outside_file(cli, db, library, clip_lib, capfd):
    paths, labels, names, index = db["paths"], db["labels"], db["names"], db["index"]
    outside = library["base"] / "outside.jpg"
    apple, copy = find(paths, "b/red_apple.jpg"), find(paths, "c/copy.png")
    vec = embed(db["clip"], clip_lib, outside)
    rc, out, err = cli(capfd, "file", "--db", db["dir"], "-k", 3, "-n", 3, outside, paths[copy])
    assert rc == 0, out[-3000:] + err[-3000:]
    res_out, res_in = index.vote(vec, 3, labels, m=3), index.vote_ids([copy], 3, labels, m=3)
    want = ["filing:", str(outside)] + lines_of(res_out, 0, 3, names, paths) + ["", paths[copy]] + lines_of(res_in, 0, 3, names, paths)
    want.append("main: 2 images, 3 voters each")
    lines = out.splitlines()
    assert lines[lines.index("filing:"):] == want
    # the same pixels as b/red_apple.jpg: that image is the nearest voter, and nothing excludes it
    assert want[2].endswith(" %s ~ %s" % (os.path.dirname(paths[apple]), paths[apple])) and res_out[3][0, 0] == apple and abs(res_out[2][0, 0]) < 1e-6
    rc, out, err = cli(capfd, "file", "--db", db["dir"], library["base"] / "missing.png")
    assert rc == 1 and "failed to load image" in err


def test_audit(cli, db, capfd):
    paths, labels, names, index = db["paths"], db["labels"], db["names"], db["index"]
    copy, orig = find(paths, "c/copy.png"), find(paths, "a/img0.png")
    for k in (1, 3, None):
        rc, out, err = cli(capfd, "audit", "--db", db["dir"], *(["-k", k] if k else []))
        assert rc == 0, out[-3000:] + err[-3000:]
        k = k or 10
        c, v, d, i = index.vote_graph(k, labels, m=1)
        want = ["misfiled:"]
        for r in range(len(paths)):
            if c[r, 0] != labels[r]:
                want.append("  %d/%d %f %s -> %s ~ %s" % (v[r, 0], min(k, 10), d[r, 0], paths[r], names[c[r, 0]], paths[i[r, 0]]))
        want.append("main: 11 labelled images, %d filed against their neighbours, 0 with no voter" % (len(want) - 1))
        lines = out.splitlines()
        assert lines[lines.index("misfiled:"):] == want
        if k == 1:                                            # the planted copy and its original point at each other, at distance ~0
            assert "  1/1 %f %s -> %s ~ %s" % (d[copy, 0], paths[copy], os.path.dirname(paths[orig]), paths[orig]) in want
            assert "  1/1 %f %s -> %s ~ %s" % (d[orig, 0], paths[orig], os.path.dirname(paths[copy]), paths[copy]) in want
            assert abs(d[copy, 0]) < 1e-6 and d[copy, 0] == d[orig, 0]
    # --in: only folder c votes and is audited: four images, each with three voters of its own class
    rc, out, err = cli(capfd, "audit", "--db", db["dir"], "-v", "0", "--in", os.path.dirname(paths[copy]) + "/")
    assert rc == 0 and out.splitlines()[-1] == "main: 4 labelled images, 0 filed against their neighbours, 0 with no voter"
    assert not [l for l in out.splitlines() if l.startswith("  ")]


def test_labels_file(cli, db, library, capfd):
    paths, index = db["paths"], db["index"]
    from clip_cpp_amd import image_search
    copy, apple, orig = find(paths, "c/copy.png"), find(paths, "b/red_apple.jpg"), find(paths, "a/img0.png")
    listed = [i for i in range(len(paths)) if i not in (apple, orig)]      # two images left unlabelled
    f = library["base"] / "labels.tsv"
    f.write_text("".join("%s\t%s\n" % ("even" if i % 2 == 0 else "odd ones", paths[i]) for i in listed))
    labels, names = image_search.read_labels(paths, str(f))
    assert int((labels < 0).sum()) == 2 and labels[apple] == -1 and labels[orig] == -1
    rc, out, err = cli(capfd, "file", "--db", db["dir"], "--labels", f, "-k", 9, "-n", 2, paths[apple], paths[orig], paths[copy])
    assert rc == 0, out[-3000:] + err[-3000:]
    res = index.vote_ids([apple, orig, copy], 9, labels, m=2)
    want = ["filing:"]
    for r, (i, counted) in enumerate(((apple, 9), (orig, 9), (copy, 8))):      # 9 voters; the copy is one of them and does not count itself
        want += ([""] if r else []) + [paths[i]] + lines_of(res, r, counted, names, paths)
    want.append("main: 3 images, 9 voters each")
    lines = out.splitlines()
    assert lines[lines.index("filing:"):] == want
    assert paths[apple] in want and paths[orig] in want                 # asked about ...
    assert not any(l.endswith("~ " + paths[apple]) or l.endswith("~ " + paths[orig]) for l in want)      # ... never a witness
    assert np.all(res[1].sum(axis=1) == [9, 9, 8])                      # two classes in all: every voter is counted in the two lines
    rc, out, err = cli(capfd, "audit", "--db", db["dir"], "--labels", f, "-k", 3)
    assert rc == 0, out[-3000:] + err[-3000:]
    c, v, d, i = index.vote_graph(3, labels, m=1)
    wrong = [r for r in listed if c[r, 0] != labels[r]]
    assert out.splitlines()[-1] == "main: 9 labelled images, %d filed against their neighbours, 0 with no voter" % len(wrong)
    hits = [l for l in out.splitlines() if l.startswith("  ")]
    assert len(hits) == len(wrong) and not any(paths[apple] in l or paths[orig] in l for l in hits)
    # a path the database does not hold is named
    f.write_text("even\t%s\nodd ones\tno/such/image.png\n" % paths[copy])
    rc, out, err = cli(capfd, "audit", "--db", db["dir"], "--labels", f)
    assert rc == 1 and "no/such/image.png" in err
