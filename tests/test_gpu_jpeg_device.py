"""The GPU pixel half of the JPEG decoder (k_jpeg.hip: jpeg_idct_kernel + jpeg_rgb_kernel) against the host decoder, bit for bit:
clip_amd_test_jpeg_decode_device runs the entropy stage on the host and the two kernels on the device, clip_image_load_from_file is the
host decoder.  The sizes are the edges where the up-sampling filters, the last-row clamp and partial MCUs differ from the interior: one
sample per row or column, one block, just below / above one and two MCUs, two-pixel strips in both directions."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL.Image")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

JPEG_CASES = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, progressive=True),
              dict(subsampling=0, progressive=True), dict(subsampling=1, progressive=True, quality=35), dict(quality=95, optimize=True),
              dict(gray=True), dict(gray=True, progressive=True),
              dict(subsampling=2, restart_marker_blocks=1), dict(subsampling=0, restart_marker_blocks=3),
              dict(subsampling=1, progressive=True, restart_marker_blocks=2), dict(gray=True, restart_marker_blocks=7),
              dict(subsampling=2, restart_marker_rows=1)]
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 13), (33, 31), (2, 65), (65, 2)]


def _photo(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(np.sin(xx / 17.0 + yy / 31.0) * 0.5 + 0.5) * 255, (np.cos(yy / 13.0) * 0.5 + 0.5) * 255, (xx * 3 + yy * 5) % 256], -1)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def jpeg_bytes(size, kw, seed=0):
    kw = dict(kw)
    gray = kw.pop("gray", False)
    img = _photo(size[0], size[1], seed=seed)
    pim = PIL.fromarray(img).convert("L") if gray else PIL.fromarray(img)
    buf = io.BytesIO()
    pim.save(buf, "JPEG", **{"quality": 80, **kw})
    return buf.getvalue()


def host_pixels(clip_lib, tmp_path, data):
    path = str(tmp_path / "t.jpg")
    open(path, "wb").write(data)
    L = clip_lib.lib()
    img = L.clip_image_u8_make()
    try:
        assert L.clip_image_load_from_file(os.fsencode(path), img)
        c = img.contents
        return np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    finally:
        L.clip_image_u8_free(img)


def device_pixels(clip_lib, data, cap=None):
    """(return code, pixels or None)"""
    w, h = PIL.open(io.BytesIO(data)).size
    cap = 3 * w * h if cap is None else cap
    out = np.full(max(cap, 1), 0x5A, np.uint8)
    nx, ny = C.c_int(0), C.c_int(0)
    rc = clip_lib.lib().clip_amd_test_jpeg_decode_device(data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(nx), C.byref(ny))
    if rc != 0:
        return rc, None
    return rc, out[:3 * nx.value * ny.value].reshape(ny.value, nx.value, 3)


def assert_same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want), "%d of %d bytes differ, max diff %d" % (
        (got != want).sum(), want.size, np.abs(got.astype(int) - want.astype(int)).max())


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", range(len(JPEG_CASES)))
def test_device_pixels_equal_host_decoder(clip_lib, tmp_path, size, case):
    data = jpeg_bytes(size, JPEG_CASES[case], seed=case)
    want = host_pixels(clip_lib, tmp_path, data)
    rc, got = device_pixels(clip_lib, data)
    assert rc == 0
    assert_same(got, want)


@pytest.mark.parametrize("name", ["red_apple.jpg", "white.jpg"])
def test_reference_test_images(clip_lib, tmp_path, name):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    rc, got = device_pixels(clip_lib, data)
    assert rc == 0
    assert_same(got, host_pixels(clip_lib, tmp_path, data))


def _jpeg_patch(data, drop_app0=False, adobe_transform=None, ids=None):
    """Rewrite markers of a JPEG: remove the JFIF APP0, insert / change the Adobe APP14 transform, rename the component ids
    (as tests/test_image_io.py does)."""
    out, i = bytearray(data[:2]), 2
    if adobe_transform is not None and b"Adobe" not in data:
        out += b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe_transform)
    while i < len(data):
        assert data[i] == 0xFF
        m = data[i + 1]
        if m == 0xDA:
            seg = bytearray(data[i:])
            j = 0
            while ids and j >= 0:                      # every scan header (progressive files have several)
                for k in range(seg[j + 4]):
                    seg[j + 5 + 2 * k] = ids[seg[j + 5 + 2 * k] - 1]
                j = seg.find(b"\xff\xda", j + 2)
            out += seg
            break
        ln = struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = bytearray(data[i:i + 2 + ln])
        if m == 0xE0 and drop_app0:
            seg = b""
        if m == 0xEE and adobe_transform is not None and seg[4:9] == b"Adobe":
            seg[15] = adobe_transform
        if m in (0xC0, 0xC2) and ids:
            for k in range(seg[9]):
                seg[10 + 3 * k] = ids[seg[10 + 3 * k] - 1]
        out += seg
        i += 2 + ln
    return bytes(out)


@pytest.mark.parametrize("size", [(16, 16), (41, 29), (3, 70)])
@pytest.mark.parametrize("kw", [dict(), dict(progressive=True), dict(subsampling=0), dict(quality=30, restart_marker_blocks=2)])
def test_stored_rgb_variants_equal_host(clip_lib, tmp_path, size, kw):
    rgb = jpeg_bytes(size, {"quality": 85, **kw}, seed=11)
    info = (C.c_int * 16)()
    for patched, colour in ((_jpeg_patch(rgb, ids=b"RGB"), 2),                                   # component ids 'R' 'G' 'B': samples are RGB
                            (_jpeg_patch(rgb, ids=b"RGb"), 1),
                            (_jpeg_patch(rgb, adobe_transform=0), 1),                            # Adobe transform 0 in a JFIF file: still YCbCr
                            (_jpeg_patch(rgb, adobe_transform=0, drop_app0=True), 2),            # ... without JFIF: RGB
                            (_jpeg_patch(rgb, adobe_transform=1, drop_app0=True), 1)):
        assert clip_lib.lib().clip_amd_test_jpeg_plan(patched, len(patched), info) == 1 and info[0] == 1 and info[5] == colour
        rc, got = device_pixels(clip_lib, patched)
        assert rc == 0
        assert_same(got, host_pixels(clip_lib, tmp_path, patched))


def _as_440(data):
    """A PIL 4:2:2 file (luma 2x1) turned into a 4:4:0 one (luma 1x2, the layout PIL does not write) by its frame header alone: the
    sampling byte of the first component, and width and height exchanged so that the scan still holds exactly the MCUs the header
    promises (an MCU has two luma blocks either way).  The pixels mean nothing; the vertical-only up-sampling is what is run."""
    i = data.find(b"\xff\xc0")
    assert i > 0 and data[i + 9] == 3 and data[i + 11] == 0x21
    out = bytearray(data)
    out[i + 5:i + 7], out[i + 7:i + 9] = data[i + 7:i + 9], data[i + 5:i + 7]
    out[i + 11] = 0x12
    return bytes(out)


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (13, 17), (33, 31), (2, 65), (65, 2)])
def test_vertical_only_subsampling_equals_host(clip_lib, tmp_path, size):
    data = _as_440(jpeg_bytes(size, dict(subsampling=1), seed=5))
    info = (C.c_int * 16)()
    assert clip_lib.lib().clip_amd_test_jpeg_plan(data, len(data), info) == 1
    assert info[0] == 1 and (info[1], info[2]) == size and list(info[7:13]) == [1, 2, 1, 1, 1, 1]     # (width, height) = the written (height, width)
    want = host_pixels(clip_lib, tmp_path, data)
    out = np.full(3 * size[0] * size[1], 0x5A, np.uint8)
    nx, ny = C.c_int(0), C.c_int(0)
    rc = clip_lib.lib().clip_amd_test_jpeg_decode_device(data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(nx), C.byref(ny))
    assert rc == 0
    assert_same(out.reshape(ny.value, nx.value, 3), want)


def test_host_planned_files_are_refused(clip_lib):
    data = jpeg_bytes((64, 64), dict(subsampling=2), seed=2)
    sos = data.rfind(b"\xff\xda")
    cut = data[:sos + (len(data) - sos) // 2]
    buf = io.BytesIO()
    PIL.fromarray(_photo(24, 40, 3)).convert("CMYK").save(buf, "JPEG", quality=85)
    png = io.BytesIO()
    PIL.fromarray(_photo(24, 40, 3)).save(png, "PNG")
    for blob, dims in ((cut, (64, 64)), (buf.getvalue(), (40, 24)), (png.getvalue(), (40, 24))):
        out = np.full(3 * dims[0] * dims[1], 0x5A, np.uint8)
        nx, ny = C.c_int(0), C.c_int(0)
        rc = clip_lib.lib().clip_amd_test_jpeg_decode_device(blob, len(blob), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(nx), C.byref(ny))
        assert rc == -2 and (out == 0x5A).all()
    rc, got = device_pixels(clip_lib, data, cap=3 * 64 * 64 - 1)                                   # too small a buffer: refused as well
    assert rc == -3
