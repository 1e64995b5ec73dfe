"""`python -m clip_cpp_amd.image_search build` over a tree of mixed image files, now that it decodes through Clip.encode_image_files:
the stored rows are what the command stored before — groups of BATCH consecutive loadable images, each group decoded by
clip_image_load_from_file and encoded by one encode_images_u8 call — images.paths lists the loadable files in scan order, and the file
that does not load is named.  Runs in this process with image_search.BATCH = 4."""
import io
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture()
def batch_of_four(clip_lib):
    from clip_cpp_amd import image_search
    old = image_search.BATCH
    image_search.BATCH = 4
    yield image_search
    image_search.BATCH = old


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture_cache):
    from oracle import fixtures
    base = tmp_path_factory.mktemp("files_tree")
    imgs = base / "pictures"
    rng = np.random.default_rng(23)
    made = []
    for sub, name, fmt, kw in (("a", "01.jpg", "JPEG", dict(quality=80)), ("a", "03.png", "PNG", {}), ("a", "04.jpg", "JPEG", dict(progressive=True, subsampling=1)),
                               ("a", "05.gif", "GIF", {}), ("a/deep", "06.jpeg", "JPEG", dict(subsampling=0)), ("a/deep", "07.PNG", "PNG", {}),
                               ("b", "08.jpg", "JPEG", dict(quality=50, restart_marker_blocks=3)), ("b", "09.png", "PNG", {}), ("b", "10.jpg", "JPEG", {})):
        os.makedirs(imgs / sub, exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(20, 70)), int(rng.integers(20, 70)), 3), dtype=np.uint8)
        pim = PIL.fromarray(arr)
        if name == "07.PNG":
            pim = pim.convert("LA")                                  # grey + alpha: another path of the PNG decoder
        (pim.convert("P") if fmt == "GIF" else pim).save(imgs / sub / name, format=fmt, **kw)
        made.append(str(imgs / sub / name))
    (imgs / "a" / "02_broken.jpg").write_bytes(b"\xff\xd8\xff\xe0 this is not a jpeg")          # inside the first window of four
    for name in ("red_apple.jpg", "white.jpg"):
        shutil.copy(os.path.join(GOLDEN, name), imgs / "b" / ("11_" + name))
        made.append(str(imgs / "b" / ("11_" + name)))
    return dict(base=base, imgs=imgs, made=sorted(made), model=fixtures.cached_model(fixture_cache, "tiny", "f32"))


def u8_rows(clip, clip_lib, paths):
    """clip_image_load_from_file + encode_images_u8 in groups of four consecutive images: the batches `build` has always cut"""
    L = clip_lib.lib()
    arrays = []
    for p in paths:
        im = L.clip_image_u8_make()
        assert L.clip_image_load_from_file(p.encode(), im)
        c = im.contents
        arrays.append(np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy())
        L.clip_image_u8_free(im)
    return np.concatenate([clip.encode_images_u8(arrays[i:i + 4], normalize=True) for i in range(0, len(arrays), 4)])


def assert_index_holds(clip, clip_lib, index_file, want, scratch):
    """f32 rows: the file holds the embeddings' bits, so an index of `want` saved next to it is the same file"""
    probe = clip_lib.Index(clip, want.shape[1], "f32")
    probe.add(want)
    probe.save(str(scratch))
    probe.close()
    assert index_file.read_bytes() == scratch.read_bytes()


@pytest.mark.parametrize("route", [None, "0"], ids=["default", "jpeg-on-host"])
def test_build_stores_the_rows_of_the_u8_route(batch_of_four, tree, clip_lib, capfd, monkeypatch, route):
    image_search = batch_of_four
    db = tree["base"] / ("db_" + str(route))
    if route is None:
        monkeypatch.delenv("CLIP_AMD_JPEG_DEVICE", raising=False)
    else:
        monkeypatch.setenv("CLIP_AMD_JPEG_DEVICE", route)
    # (by default the JPEG kernels run inside `build`: 7 of the 11 files are device-planned JPEGs)
    on_device = clip_lib.lib().clip_amd_test_jpeg_device_count()
    capfd.readouterr()
    rc = image_search.main(["build", "-m", tree["model"], "-v", "2", "-t", "3", "--dtype", "f32", "--db", str(db), str(tree["imgs"])])
    out = capfd.readouterr()
    assert rc == 0, out.out[-3000:] + out.err[-3000:]
    assert clip_lib.lib().clip_amd_test_jpeg_device_count() - on_device == (7 if route is None else 0)
    bad = str(tree["imgs"] / "a" / "02_broken.jpg")
    assert "main: failed to load image from '%s'" % bad in out.err
    assert out.err.count("main: failed to load image from") == 1
    scan = image_search.image_files(str(tree["imgs"]))
    assert [l for l in out.out.splitlines() if l.startswith("main: found image file")] == ["main: found image file '%s'" % p for p in scan]
    assert "main: 11 images processed and indexed" in out.out
    lines = (db / "images.paths").read_text().split("\n")
    paths = lines[1:-1]
    assert lines[0] == tree["model"] and paths == [p for p in scan if p != bad] and sorted(paths) == tree["made"]
    clip = clip_lib.Clip(tree["model"], verbosity=0, device=0)
    assert_index_holds(clip, clip_lib, db / "images.index", u8_rows(clip, clip_lib, paths), tree["base"] / ("ref_%s.index" % route))
    clip.close()


def test_batches_run_across_directory_arguments(batch_of_four, tree, clip_lib, capfd, monkeypatch):
    """Two directory arguments, the first with 6 loadable files: the second batch of four takes two files of each.  The lines of a
    directory come out once and in order, its header before its first file."""
    image_search = batch_of_four
    db = tree["base"] / "db2"
    a, b = str(tree["imgs"] / "a"), str(tree["imgs"] / "b")
    monkeypatch.delenv("CLIP_AMD_JPEG_DEVICE", raising=False)
    capfd.readouterr()
    rc = image_search.main(["build", "-m", tree["model"], "-v", "2", "-t", "2", "--dtype", "f32", "--db", str(db), a, b])
    out = capfd.readouterr()
    assert rc == 0, out.out[-3000:] + out.err[-3000:]
    fa, fb = image_search.image_files(a), image_search.image_files(b)
    bad = str(tree["imgs"] / "a" / "02_broken.jpg")
    assert len(fa) == 7 and len(fb) == 5 and bad in fa
    want = (["main: starting base dir scan of '%s'" % a, "main: processing 7 files in '%s'" % a] + ["main: found image file '%s'" % p for p in fa] +
            ["main: starting base dir scan of '%s'" % b, "main: processing 5 files in '%s'" % b] + ["main: found image file '%s'" % p for p in fb] +
            ["main: 11 images processed and indexed"])
    assert [l for l in out.out.splitlines() if l.startswith("main: ") and not l.startswith("main: Unable")][-len(want):] == want
    assert out.err.count("main: failed to load image from") == 1 and "main: failed to load image from '%s'" % bad in out.err
    paths = (db / "images.paths").read_text().split("\n")[1:-1]
    assert paths == [p for p in fa + fb if p != bad]
    clip = clip_lib.Clip(tree["model"], verbosity=0, device=0)
    assert_index_holds(clip, clip_lib, db / "images.index", u8_rows(clip, clip_lib, paths), tree["base"] / "ref2.index")
    clip.close()
