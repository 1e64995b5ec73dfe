"""Clip.encode_image_files / encode_image_bytes (clip_amd_image_batch_encode_files / _memory): encoded images in, embeddings out, against
the route the library had before — clip_image_load_from_file per file, then ONE clip_amd_image_batch_encode_u8 call over the loadable
images.  Every comparison is bit for bit: the JPEG pixel half on the GPU is integer arithmetic restated exactly, and the loadable images
of a call form the same encoder batch on both routes."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# device-planned JPEGs of the `files` fixture's list, and of `many` (every JPEG there is PIL-written and complete)
N_DEVICE_IN_ORDER = 5

PIL = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _photo(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(np.sin(xx / 17.0 + yy / 31.0) * 0.5 + 0.5) * 255, (np.cos(yy / 13.0) * 0.5 + 0.5) * 255, (xx * 3 + yy * 5) % 256], -1)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def _bytes(arr, fmt, mode=None, **kw):
    buf = io.BytesIO()
    pim = PIL.fromarray(arr)
    (pim.convert(mode) if mode else pim).save(buf, fmt, **kw)
    return buf.getvalue()


@pytest.fixture(scope="module")
def model(fixture_cache):
    from oracle import fixtures
    return fixtures.cached_model(fixture_cache, "tiny", "f32")


@pytest.fixture(scope="module")
def clip(clip_lib, model):
    c = clip_lib.Clip(model, verbosity=0, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path of a mixed set; `order` lists them with a corrupt file and a missing path in between"""
    d = tmp_path_factory.mktemp("files")
    blobs = {
        "a420.jpg": _bytes(_photo(57, 83, 1), "JPEG", quality=80, subsampling=2),                       # planned "device"
        "b422p.jpg": _bytes(_photo(40, 33, 2), "JPEG", quality=70, subsampling=1, progressive=True),    # "device"
        "c.png": _bytes(_photo(31, 47, 3), "PNG"),
        "d_grey.jpg": _bytes(_photo(25, 64, 4), "JPEG", mode="L", quality=85),                          # "device"
        "e_cmyk.jpg": _bytes(_photo(36, 36, 5), "JPEG", mode="CMYK", quality=85),                       # "host": four components
        "f.gif": _bytes(_photo(29, 52, 6), "GIF", mode="P"),
        "g444rst.jpg": _bytes(_photo(66, 21, 7), "JPEG", quality=90, subsampling=0, restart_marker_blocks=2),
        "i.bmp": _bytes(_photo(20, 71, 9), "BMP"),
    }
    whole = _bytes(_photo(64, 64, 8), "JPEG", quality=80, subsampling=2)
    sos = whole.rfind(b"\xff\xda")
    blobs["h_cut.jpg"] = whole[:sos + (len(whole) - sos) // 2]                                          # "host": cut inside its entropy data, still loadable
    blobs["apple.jpg"] = open(os.path.join(GOLDEN, "red_apple.jpg"), "rb").read()
    blobs["corrupt.jpg"] = b"\xff\xd8\xff\xe0 this is not a jpeg"
    paths = {}
    for name, b in blobs.items():
        paths[name] = str(d / name)
        open(paths[name], "wb").write(b)
    paths["missing.jpg"] = str(d / "missing.jpg")
    order = ["a420.jpg", "corrupt.jpg", "b422p.jpg", "c.png", "d_grey.jpg", "missing.jpg", "e_cmyk.jpg", "f.gif", "g444rst.jpg", "h_cut.jpg",
             "i.bmp", "apple.jpg"]
    return dict(dir=d, paths=paths, blobs=blobs, order=[paths[n] for n in order], bad={paths["corrupt.jpg"], paths["missing.jpg"]})


@pytest.fixture(autouse=True, params=[None, "0"], ids=["default", "jpeg-on-host"])
def route(request, monkeypatch):
    """Every test of this module runs twice: with CLIP_AMD_JPEG_DEVICE unset (the default: the JPEG kernels run inside the pipeline) and
    with =0 (every JPEG's pixel half on the host threads; the library reads the switch at every call).  The expected rows are the same."""
    if request.param is None:
        monkeypatch.delenv("CLIP_AMD_JPEG_DEVICE", raising=False)
    else:
        monkeypatch.setenv("CLIP_AMD_JPEG_DEVICE", request.param)
    return request.param


class staged:
    """with staged(clip_lib, route, n): the calls inside hand exactly n JPEGs to the JPEG kernels, none with CLIP_AMD_JPEG_DEVICE=0"""

    def __init__(self, clip_lib, route, n):
        self.count, self.want = clip_lib.lib().clip_amd_test_jpeg_device_count, 0 if route == "0" else n

    def __enter__(self):
        self.before = self.count()

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.count() - self.before == self.want


_decoded = {}


def pixels(clip_lib, path):
    """clip_image_load_from_file's pixels (decoded once per file), None for a file it does not load"""
    if path not in _decoded:
        L = clip_lib.lib()
        img = L.clip_image_u8_make()
        if L.clip_image_load_from_file(os.fsencode(path), img):
            c = img.contents
            _decoded[path] = np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
        else:
            _decoded[path] = None
        L.clip_image_u8_free(img)
    return _decoded[path]


def u8_route(clip, clip_lib, paths, normalize=True):
    arrays = [pixels(clip_lib, p) for p in paths]
    assert all(a is not None for a in arrays)
    return clip.encode_images_u8(arrays, normalize=normalize)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()


def test_plans_of_the_fixture_files(clip_lib, files):
    info = (C.c_int * 16)()
    routes = {}
    for name in ("a420.jpg", "b422p.jpg", "d_grey.jpg", "g444rst.jpg", "apple.jpg", "e_cmyk.jpg", "h_cut.jpg"):
        b = files["blobs"][name]
        assert clip_lib.lib().clip_amd_test_jpeg_plan(b, len(b), info) == 1
        routes[name] = info[0]
    assert routes == {"a420.jpg": 1, "b422p.jpg": 1, "d_grey.jpg": 1, "g444rst.jpg": 1, "apple.jpg": 1, "e_cmyk.jpg": 0, "h_cut.jpg": 0}


def test_device_planned_jpegs_are_staged(clip, clip_lib, files, monkeypatch):
    """The rows are the same whichever side runs a JPEG's pixel half, so the count of images handed to the JPEG kernels is what shows
    that the device route is taken: the five device-planned files of the list with CLIP_AMD_JPEG_DEVICE=1, none with =0."""
    count = clip_lib.lib().clip_amd_test_jpeg_device_count
    rows = {}
    for switch, staged in (("1", 5), ("0", 0)):
        monkeypatch.setenv("CLIP_AMD_JPEG_DEVICE", switch)           # (read by the library at every call)
        before = count()
        rows[switch], ok, consumed = clip.encode_image_files(files["order"], n_threads=3)
        assert count() - before == staged
    same_bits(rows["1"], rows["0"])


@pytest.mark.parametrize("normalize", [True, False])
def test_mixed_list(clip, clip_lib, files, normalize, route):
    order = files["order"]
    with staged(clip_lib, route, N_DEVICE_IN_ORDER):
        vecs, ok, consumed = clip.encode_image_files(order, normalize=normalize, n_threads=3)
    assert consumed == len(order)
    assert ok.tolist() == [p not in files["bad"] for p in order]
    good = [p for p in order if p not in files["bad"]]
    same_bits(vecs, u8_route(clip, clip_lib, good, normalize))
    if normalize:
        assert np.allclose(np.sqrt((vecs.astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-5)


def test_max_images_windows(clip, clip_lib, files, route):
    P = files["paths"]
    paths = [P[n] for n in ("a420.jpg", "corrupt.jpg", "c.png", "b422p.jpg", "f.gif", "d_grey.jpg", "e_cmyk.jpg", "g444rst.jpg", "apple.jpg", "i.bmp")]
    with staged(clip_lib, route, 2):
        vecs, ok, consumed = clip.encode_image_files(paths, max_images=4, n_threads=2)
    assert consumed == 5 and ok.tolist() == [True, False, True, True, True] and vecs.shape[0] == 4
    same_bits(vecs, u8_route(clip, clip_lib, [paths[0]] + paths[2:5]))
    with staged(clip_lib, route, 3):
        vecs, ok, consumed = clip.encode_image_files(paths[5:], max_images=4, n_threads=2)
    assert consumed == 4 and ok.all() and vecs.shape[0] == 4
    same_bits(vecs, u8_route(clip, clip_lib, paths[5:9]))
    prepared = clip.ImageFileList(paths)                                  # the same walk over a list prepared once
    vecs, ok, consumed = clip.encode_image_files(prepared, max_images=4, n_threads=2, start=9)
    assert consumed == 1 and ok.tolist() == [True]
    same_bits(vecs, u8_route(clip, clip_lib, paths[9:]))
    vecs, ok, consumed = clip.encode_image_files(prepared, max_images=4, n_threads=2, start=5)
    assert consumed == 4 and ok.all()
    same_bits(vecs, u8_route(clip, clip_lib, paths[5:9]))
    assert clip.encode_image_files(prepared, max_images=4, start=10)[2] == 0


def test_empty_and_unloadable_lists(clip, files):
    proj = clip.vision_config["projection_dim"]
    vecs, ok, consumed = clip.encode_image_files([])
    assert vecs.shape == (0, proj) and consumed == 0 and len(ok) == 0
    bad = [files["paths"]["corrupt.jpg"], files["paths"]["missing.jpg"], files["paths"]["corrupt.jpg"]]
    for mx in (None, 1, 2):
        vecs, ok, consumed = clip.encode_image_files(bad, max_images=mx)
        assert vecs.shape == (0, proj) and consumed == 3 and not ok.any()
    vecs, ok, consumed = clip.encode_image_bytes([])
    assert vecs.shape == (0, proj) and consumed == 0


def test_one_image_and_more_threads_than_images(clip, clip_lib, files, route):
    for name, device in (("a420.jpg", 1), ("c.png", 0), ("h_cut.jpg", 0)):
        p = files["paths"][name]
        with staged(clip_lib, route, device):
            vecs, ok, consumed = clip.encode_image_files([p], n_threads=16)
        assert consumed == 1 and ok.tolist() == [True]
        same_bits(vecs, u8_route(clip, clip_lib, [p]))


@pytest.fixture(scope="module")
def many(files):
    """65 files: small JPEGs of several layouts and sizes with the other formats in between"""
    d = files["dir"]
    out = []
    for i in range(65):
        h, w = 18 + (i * 7) % 23, 17 + (i * 5) % 29
        p = str(d / ("m%02d.%s" % (i, "png" if i % 9 == 4 else "jpg")))
        if i % 9 == 4:
            open(p, "wb").write(_bytes(_photo(h, w, 100 + i), "PNG"))
        else:
            open(p, "wb").write(_bytes(_photo(h, w, 100 + i), "JPEG", mode="L" if i % 7 == 3 else None, quality=60 + i % 35,
                                       progressive=bool(i % 4 == 1), **({} if i % 7 == 3 else {"subsampling": i % 3})))
        out.append(p)
    return out


def test_65_images(clip, clip_lib, many, route):
    with staged(clip_lib, route, sum(p.endswith(".jpg") for p in many)):
        vecs, ok, consumed = clip.encode_image_files(many, n_threads=8)
    assert consumed == 65 and ok.all()
    same_bits(vecs, u8_route(clip, clip_lib, many))


def test_bytes_equal_files(clip, clip_lib, files, route):
    order = files["order"]
    blobs = [open(p, "rb").read() if os.path.exists(p) else b"" for p in order]
    a = clip.encode_image_files(order, n_threads=4)
    with staged(clip_lib, route, N_DEVICE_IN_ORDER):
        b = clip.encode_image_bytes(blobs, n_threads=4)
    same_bits(b[0], a[0])
    assert b[1].tolist() == a[1].tolist() and b[2] == a[2]
    a = clip.encode_image_files(order, n_threads=1, max_images=3)
    b = clip.encode_image_bytes(blobs, n_threads=1, max_images=3)
    same_bits(b[0], a[0])
    assert b[1].tolist() == a[1].tolist() and b[2] == a[2] == 4


CHILD = """
import sys, numpy as np
import clip_cpp_amd
paths = open(sys.argv[2]).read().split("\\n")
clip = clip_cpp_amd.Clip(sys.argv[1], verbosity=0, device=0)
vecs, ok, consumed = clip.encode_image_files(paths, n_threads=4)
np.save(sys.argv[3], vecs)
print("rows", len(vecs), "consumed", consumed, "ok", int(ok.sum()), "on device", clip_cpp_amd.lib().clip_amd_test_jpeg_device_count())
clip.close()
"""


@pytest.mark.parametrize("env", [{"CLIP_AMD_JPEG_DEVICE": "0"}, {"CLIP_AMD_JPEG_DEVICE": "1", "CLIP_AMD_U8_PIECE": "16"}], ids=["jpeg-on-host", "staging-ring"])
def test_switches_in_a_child_process(clip, clip_lib, files, many, model, tmp_path, env, route):
    """A child with CLIP_AMD_JPEG_DEVICE=0 (every JPEG's pixel half on the host threads) and one with =1 and CLIP_AMD_U8_PIECE=16 (the 75
    loadable images are staged in pieces of 16 through the ring of preprocessing slots, decoded pixels and device-planned JPEGs mixed in
    a piece, the JPEG kernels ahead of each piece's preprocessing) give the rows of this process, on whichever route it runs."""
    paths = files["order"] + many
    n_device = N_DEVICE_IN_ORDER + sum(p.endswith(".jpg") for p in many)
    with staged(clip_lib, route, n_device):
        want, ok, consumed = clip.encode_image_files(paths, n_threads=4)
    listing, out = tmp_path / "paths.txt", tmp_path / "rows.npy"
    listing.write_text("\n".join(paths))
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("CLIP_AMD_JPEG_DEVICE", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, model, str(listing), str(out)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rows %d consumed %d ok %d on device %d" % (len(want), consumed, int(ok.sum()), n_device if env["CLIP_AMD_JPEG_DEVICE"] == "1" else 0) in r.stdout
    same_bits(np.load(out), want)
