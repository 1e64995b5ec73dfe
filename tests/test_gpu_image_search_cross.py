"""End to end: `python -m clip_cpp_amd.image_search label` and `merge` over small synthetic databases built by `build`: the lines `label`
prints are Index.search of an index of the labels with the re-encoded images; `merge` of two databases that share one path and one
pixel-identical copy gives the counts, the -d listing and the two files that `build` over the kept files gives.

The commands run in this process with one image per encoder batch (image_search.BATCH = 1): an embedding is bit-identical between two
batches only when both use the same GEMM kernels (tests/test_gpu_parity.py), and a database of 4 images, one of 5 and their union of 7
would otherwise be encoded in batches of three sizes."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LABELS = ["a red apple", "white", "static noise", "a dog"]


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
def pictures(tmp_path_factory, fixture_cache):
    """pictures/{a,shared,b,c}: three generated PNGs in a and in b, one in shared, and in c a pixel-identical copy of a/img0.png;
    b also holds the reference's red apple"""
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("cross")
    imgs = base / "pictures"
    rng = np.random.default_rng(19)
    for sub, count in (("a", 3), ("shared", 1), ("b", 3)):
        os.makedirs(imgs / sub)
        for i in range(count):
            arr = rng.integers(0, 256, size=(int(rng.integers(20, 60)), int(rng.integers(20, 60)), 3), dtype=np.uint8)
            Image.fromarray(arr).save(imgs / sub / ("img%d.png" % i), format="PNG")
    shutil.copy(os.path.join(GOLDEN, "red_apple.jpg"), imgs / "b" / "red_apple.jpg")
    os.makedirs(imgs / "c")
    shutil.copy(imgs / "a" / "img0.png", imgs / "c" / "copy.png")
    return dict(base=base, imgs=imgs, model=fixtures.cached_model(fixture_cache, "tiny", "f32"))


def db_paths(d):
    return (d / "images.paths").read_text().split("\n")[1:-1]


def embeddings(clip, clip_lib, paths):
    """decode with the library's loader, encode each image in a batch of its own (as the commands here do), normalised"""
    L = clip_lib.lib()
    out = []
    for p in paths:
        im = L.clip_image_u8_make()
        assert L.clip_image_load_from_file(p.encode(), im)
        c = im.contents
        arr = np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
        L.clip_image_u8_free(im)
        out.append(clip.encode_images_u8([arr], normalize=True))
    return np.concatenate(out)


def hit_lines(stdout):
    return [l for l in stdout.splitlines() if l.startswith("  ")]


def label_db(cli, capfd, pictures, dtype):
    """the database of all nine pictures in that dtype, built once"""
    db = pictures["base"] / ("label_" + dtype)
    if not (db / "images.index").exists():
        rc, out, err = cli(capfd, "build", "-m", pictures["model"], "-v", "0", "--dtype", dtype, "--db", db, pictures["imgs"])
        assert rc == 0, out[-3000:] + err[-3000:]
    return db


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_label(cli, pictures, clip_lib, capfd, dtype):
    db = label_db(cli, capfd, pictures, dtype)
    paths = db_paths(db)
    assert len(paths) == 9
    clip = clip_lib.Clip(pictures["model"], verbosity=0, device=0)
    labels = clip_lib.Index(clip, clip.text_config["projection_dim"], dtype)      # the database's dtype, read from its header
    labels.add(clip.encode_texts([clip.tokenize(t) for t in LABELS], normalize=True))
    vecs = embeddings(clip, clip_lib, paths)
    for n, k in ((2, 2), (None, 1), (9, 4)):                            # -n above the number of labels: all of them
        rc, out, err = cli(capfd, "label", "--db", db, *(["-n", n] if n else []), *LABELS)
        assert rc == 0, out[-3000:] + err[-3000:]
        dist, ids = labels.search(vecs, k)
        want = ["labels:"]
        for i, p in enumerate(paths):
            if i:
                want.append("")
            want.append(p)
            want += ["  %f %s" % (d, LABELS[j]) for d, j in zip(dist[i], ids[i])]
        want.append("main: 9 images, %d labels each" % k)
        lines = out.splitlines()
        assert lines[lines.index("labels:"):] == want
    rc, out, err = cli(capfd, "label", "--db", db, "-v", "0", "one label")
    assert rc == 0 and "labels:" not in out and out.splitlines()[-1] == "main: 9 images, 1 labels each" and len(hit_lines(out)) == 9
    labels.close()
    clip.close()


def test_label_needs_a_text_tower(cli, pictures, fixture_cache, capfd):
    from oracle import fixtures
    db = label_db(cli, capfd, pictures, "f16")
    vision_only = fixtures.cached_model(fixture_cache, "tiny", "f32", text=False)
    rc, out, err = cli(capfd, "label", "--db", db, "-m", vision_only, "a cat")
    assert rc == 1 and "has no text encoder: text queries need a two-tower model" in err


def test_merge(cli, pictures, clip_lib, capfd):
    base, imgs, model = pictures["base"], pictures["imgs"], pictures["model"]
    a, b, union = base / "merge_a", base / "merge_b", base / "merge_union"
    for db, dirs in ((a, ("a", "shared")), (b, ("shared", "b", "c")), (union, ("a", "shared", "b"))):
        # f32 rows: a pixel-identical copy is then at about 1e-7 from its original, below the distances between the generated images, which
        # this synthetic model puts at 1e-4 ... 1e-3 (in f16 the rounding of the rows alone moves a self distance up to 1.4e-4)
        rc, out, err = cli(capfd, "build", "-m", model, "-v", "0", "--dtype", "f32", "--db", db, *[imgs / d for d in dirs])
        assert rc == 0, out[-3000:] + err[-3000:]
    pa, pb = db_paths(a), db_paths(b)
    assert len(pa) == 4 and len(pb) == 6 and pb[0] == pa[3] and pb[5].endswith("copy.png")
    b_files = [(b / f).read_bytes() for f in ("images.index", "images.paths")]
    # what -d will list: the copy's nearest image of the target, from the two indexes as they are on disk
    clip = clip_lib.Clip(model, verbosity=0, device=0)
    ia, ib = clip_lib.Index.load(clip, str(a / "images.index")), clip_lib.Index.load(clip, str(b / "images.index"))
    dist, ids = ia.search_index(ib, 1)
    print("nearest target image of each source image:", dist[:, 0].tolist(), ids[:, 0].tolist())
    # the synthetic `tiny` model gives no natural distances: the radius lies between the copy's distance and the other images' distances
    assert ids[5, 0] == 0 and ids[0, 0] == 3 and dist[5, 0] < dist[1:5, 0].min()
    radius = "%.9g" % ((float(dist[5, 0]) + float(dist[1:5, 0].min())) / 2)
    listing = "  %f %s ~ %s" % (dist[5, 0], pb[5], pa[0])
    ia.close()
    ib.close()
    clip.close()
    rc, out, err = cli(capfd, "merge", "--db", a, "--from", b, "-d", radius)
    assert rc == 0, out[-3000:] + err[-3000:]
    assert out.splitlines()[-1] == "main: 4 added, 1 already present, 1 near duplicates skipped"
    assert hit_lines(out) == [listing]                                   # (the shared path is not listed: it was never a candidate)
    assert db_paths(a) == pa + pb[1:5]
    for f in ("images.paths", "images.index"):
        assert (a / f).read_bytes() == (union / f).read_bytes(), f
    assert b_files == [(b / f).read_bytes() for f in ("images.index", "images.paths")]      # the source is not changed
    # again: everything but the copy is there already, nothing is written
    before = os.stat(a / "images.index").st_mtime_ns
    rc, out, err = cli(capfd, "merge", "--db", a, "--from", b, "-v", "0", "-d", radius)
    assert rc == 0 and out.splitlines()[-1] == "main: 0 added, 5 already present, 1 near duplicates skipped" and hit_lines(out) == []
    assert os.stat(a / "images.index").st_mtime_ns == before
    # without -d the copy is an image like any other; two sources in one call
    rc, out, err = cli(capfd, "merge", "--db", a, "--from", b, "--from", union)
    assert rc == 0 and out.splitlines()[-1] == "main: 1 added, 13 already present, 0 near duplicates skipped"
    assert db_paths(a) == pa + pb[1:5] + pb[5:]
