"""The JPEG decoder's two stages, without a GPU: clip_amd_test_jpeg_plan runs the entropy stage and says where the pixel stage may run.
PIL-written baseline and progressive files of every sampling layout, grey files and files with restart markers are planned for the device
with the right geometry; a file cut inside its entropy data, a CMYK file and a non-JPEG stay on the host; and the refactored decoder
still gives the reference decoder's pixels for all of them (tests/golden/stb_decodes.npz, keyed by the files' bytes: the files here are
the ones tests/test_image_io.py writes)."""
import ctypes as C
import hashlib
import io
import os

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the keyword sets of tests/test_image_io.py JPEG_CASES, and its sizes and content, so that the recorded reference decodes apply
JPEG_CASES = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, progressive=True),
              dict(subsampling=0, progressive=True), dict(subsampling=1, progressive=True, quality=35), dict(quality=95, optimize=True),
              dict(gray=True), dict(gray=True, progressive=True),
              dict(subsampling=2, restart_marker_blocks=1), dict(subsampling=0, restart_marker_blocks=3),
              dict(subsampling=1, progressive=True, restart_marker_blocks=2), dict(gray=True, restart_marker_blocks=7),
              dict(subsampling=2, restart_marker_rows=1)]
SIZES = [(64, 64), (57, 83), (1, 1), (200, 3), (17, 250)]
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}          # PIL's subsampling -> the luma component's (h, v); chroma is (1, 1)
HOST, DEVICE = 0, 1


def _photo(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(np.sin(xx / 17.0 + yy / 31.0) * 0.5 + 0.5) * 255, (np.cos(yy / 13.0) * 0.5 + 0.5) * 255, (xx * 3 + yy * 5) % 256], -1)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def jpeg_bytes(size, case):
    kw = dict(JPEG_CASES[case])
    gray = kw.pop("gray", False)
    img = _photo(size[0], size[1], seed=case)
    pim = PIL.fromarray(img).convert("L") if gray else PIL.fromarray(img)
    buf = io.BytesIO()
    pim.save(buf, "JPEG", **{"quality": 80, **kw})
    return buf.getvalue()


def plan(clip_lib, data):
    info = (C.c_int * 16)()
    rc = clip_lib.lib().clip_amd_test_jpeg_plan(data, len(data), info)
    return rc, list(info)


def load_ours(clip_lib, path):
    L = clip_lib.lib()
    img = L.clip_image_u8_make()
    try:
        if not L.clip_image_load_from_file(os.fsencode(path), img):
            return None
        c = img.contents
        return np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    finally:
        L.clip_image_u8_free(img)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "stb_decodes.npz"))
    return {bytes(k): (tuple(int(v) for v in s), bytes(d)) for k, s, d in zip(z["input_sha256_16"], z["shape"], z["pixels_sha256_16"])}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", range(len(JPEG_CASES)))
def test_pil_files_are_planned_for_the_device(clip_lib, golden, tmp_path, size, case):
    data = jpeg_bytes(size, case)
    kw = JPEG_CASES[case]
    rc, info = plan(clip_lib, data)
    assert rc == 1
    route, width, height, ncomp, progressive, colour, complete = info[:7]
    assert route == DEVICE and complete == 1
    assert (height, width) == size
    assert ncomp == (1 if kw.get("gray") else 3) and colour == (0 if kw.get("gray") else 1)
    assert progressive == (1 if kw.get("progressive") else 0)
    if kw.get("gray"):
        assert info[7:9] == [1, 1]
    else:
        assert tuple(info[7:9]) == SAMPLING[kw.get("subsampling", 2)] and info[9:13] == [1, 1, 1, 1]   # (PIL's default for quality 80 / 95: 4:2:0)
    # the refactored decoder still gives the reference decoder's pixels
    path = str(tmp_path / "t.jpg")
    open(path, "wb").write(data)
    got = load_ours(clip_lib, path)
    key = hashlib.sha256(data).digest()[:16]
    assert key in golden, "tests/golden/stb_decodes.npz has no reference decode of this file"
    shape, digest = golden[key]
    assert got is not None and got.shape == shape
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest()[:16] == digest


@pytest.mark.parametrize("case", [0, 2, 3, 9])
def test_truncated_entropy_data_stays_on_the_host(clip_lib, case):
    data = jpeg_bytes((64, 64), case)
    sos = data.rfind(b"\xff\xda")
    cut = data[:sos + (len(data) - sos) // 2]                      # in the middle of the (last) scan's entropy-coded data
    rc, info = plan(clip_lib, cut)
    # still decodable (the reference's decoder reads such files too): the missing blocks are the host pixel stage's business
    assert rc == 1 and info[0] == HOST and info[6] == 0 and (info[2], info[1]) == (64, 64)


def test_cmyk_and_non_jpeg_stay_on_the_host(clip_lib):
    buf = io.BytesIO()
    PIL.fromarray(_photo(24, 40, 3)).convert("CMYK").save(buf, "JPEG", quality=85)
    rc, info = plan(clip_lib, buf.getvalue())
    assert rc == 1 and info[0] == HOST and info[3] == 4 and (info[2], info[1]) == (24, 40)
    buf = io.BytesIO()
    PIL.fromarray(_photo(24, 40, 3)).save(buf, "PNG")
    for blob in (buf.getvalue(), b"", b"\xff\xd8\xff\xe0 this is not a jpeg", b"\xff\xd8"):
        rc, info = plan(clip_lib, blob)
        assert rc == 0 and info[0] == HOST


def test_reference_images_are_planned_for_the_device(clip_lib):
    for name in ("red_apple.jpg", "white.jpg"):
        data = open(os.path.join(GOLDEN, name), "rb").read()
        rc, info = plan(clip_lib, data)
        w, h = PIL.open(io.BytesIO(data)).size
        assert rc == 1 and info[0] == DEVICE and (info[1], info[2]) == (w, h)
