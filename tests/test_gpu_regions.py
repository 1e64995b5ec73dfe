"""GPU tier of regions through the encoder (clip_amd_image_batch_preprocess_regions_device / _encode_regions /
_encode_files_grid, the row stride of k_preproc.hip): a box of an uploaded image against the same box copied out on the host, bit for
bit; nothing outside a box is read; shared uploads across staging pieces; the grid over files against load + grid_boxes + regions."""
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    c = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield c
    c.close()


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()


def crop(images, box):
    i, x, y, w, h = box
    return np.ascontiguousarray(images[i][y:y + h, x:x + w])


def regions_device(clip, images, boxes):
    import torch
    S = clip.vision_config["image_size"]
    out = torch.full((len(boxes), S, S, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    clip.preprocess_regions_device(images, boxes, out.data_ptr())
    return out.cpu().numpy()


def whole_device(clip, images):
    import torch
    S = clip.vision_config["image_size"]
    out = torch.full((len(images), S, S, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    clip.preprocess_device(images, out.data_ptr())
    return out.cpu().numpy()


def test_preprocessing_against_the_host(clip):
    S = clip.vision_config["image_size"]
    assert S == 32
    a, b = _photo(230, 260, 1), _photo(205, 211, 2)      # [ny, nx]: two source sizes in one call
    images = [a, b]
    boxes = [
        (0, 0, 0, 260, 230),        # the whole image
        (1, 0, 0, 211, 205),
        (0, 100, 77, 1, 1),         # 1 x 1
        (0, 0, 0, 90, 70),          # the four corners
        (0, 170, 0, 90, 70),
        (0, 0, 160, 90, 70),
        (0, 170, 160, 90, 70),
        (1, 210, 204, 1, 1),        # the last pixel
        (1, 7, 3, 100, 90),         # first pixel at byte 3 * (3 * 211 + 7) = 1920 ... an odd one follows
        (1, 8, 3, 101, 90),         # 3 * (3 * 211 + 8) = 1923: odd
        (0, 30, 10, 5, 200),        # the centre crop lies inside the box
        (0, 10, 30, 200, 5),
        (1, 50, 60, 20, 13),        # smaller than image_size: upsampled
        (1, 50, 60, 31, 40),
    ]
    assert (3 * (3 * 211 + 8)) % 2 == 1
    got = regions_device(clip, images, boxes)
    for r, box in enumerate(boxes):
        same_bits(got[r], clip.preprocess(crop(images, box)))
    same_bits(got[:2], whole_device(clip, images))


def test_nothing_outside_the_box_is_read(clip):
    box = (0, 37, 21, 60, 45)
    inside = _photo(45, 60, 3)
    images = []
    for fill in (0, 255):
        im = np.full((120, 150, 3), fill, dtype=np.uint8)
        im[21:21 + 45, 37:37 + 60] = inside
        images.append(im)
    assert not np.array_equal(images[0], images[1])
    got = regions_device(clip, images, [box, (1,) + box[1:]])
    same_bits(got[0], got[1])
    same_bits(got[0], clip.preprocess(inside))


def test_regions_against_the_crop_loop(clip):
    rng = np.random.default_rng(5)
    images = [_photo(90, 120, 11), _photo(64, 64, 12), _photo(75, 50, 13)]
    boxes = [(0, 0, 0, 120, 90), (0, 3, 5, 40, 33), (0, 60, 45, 60, 45), (0, 119, 89, 1, 1), (0, 17, 0, 9, 90),     # image 0 five times
             (2, 0, 0, 50, 75), (2, 1, 1, 25, 37), (2, 25, 37, 25, 38), (2, 10, 10, 31, 31), (2, 0, 70, 50, 5), (2, 49, 0, 1, 75)]
    boxes = [boxes[i] for i in rng.permutation(len(boxes))]            # shuffled; image 1 is used by no box
    assert len(boxes) == 11 and sum(b[0] == 0 for b in boxes) == 5 and not any(b[0] == 1 for b in boxes)
    for normalize in (True, False):
        got = clip.encode_image_regions(images, boxes, normalize=normalize)
        same_bits(got, clip.encode_images_u8([crop(images, b) for b in boxes], normalize=normalize))


def test_piece_boundary_inside_an_image(clip):
    """130 boxes of one 64 x 48 image: more than one staging piece of 128, so the image is uploaded in both"""
    rng = np.random.default_rng(6)
    images = [_photo(48, 64, 21)]
    boxes = []
    for _ in range(130):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 49))
        boxes.append((0, int(rng.integers(0, 64 - w + 1)), int(rng.integers(0, 48 - h + 1)), w, h))
    got = clip.encode_image_regions(images, boxes)
    same_bits(got, clip.encode_images_u8([crop(images, b) for b in boxes]))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_files")
    blobs = {
        "apple.jpg": open(os.path.join(GOLDEN, "red_apple.jpg"), "rb").read(),                           # baseline, planned "device"
        "prog.jpg": _bytes(_photo(40, 33, 2), "JPEG", quality=70, subsampling=1, progressive=True),     # "device"
        "corrupt.jpg": b"\xff\xd8\xff\xe0 this is not a jpeg",
        "c.png": _bytes(_photo(31, 47, 3), "PNG"),
        "narrow.png": _bytes(_photo(30, 1, 4), "PNG"),                                                   # narrower than any grid
        "a420.jpg": _bytes(_photo(57, 83, 1), "JPEG", quality=80, subsampling=2),                       # "device"
    }
    paths = []
    for name, b in blobs.items():
        paths.append(str(d / name))
        open(paths[-1], "wb").write(b)
    return paths


def load(clip_lib, path):
    L = clip_lib.lib()
    img = L.clip_image_u8_make()
    try:
        if not L.clip_image_load_from_file(os.fsencode(path), img):
            return None
        c = img.contents
        return np.ctypeslib.as_array(c.data, shape=(c.ny, c.nx, 3)).copy()
    finally:
        L.clip_image_u8_free(img)


@pytest.mark.parametrize("G", [2, 3])
def test_grid_over_files(clip, clip_lib, files, G, monkeypatch):
    monkeypatch.delenv("CLIP_AMD_JPEG_DEVICE", raising=False)
    R = 1 + G * G
    count = clip_lib.lib().clip_amd_test_jpeg_device_count
    plain_ok = clip.encode_image_files(files, n_threads=3)[1]
    before = count()
    vecs, ok, consumed, boxes = clip.encode_image_files(files, n_threads=3, grid=G)
    assert count() - before == 3                                       # the device-planned JPEGs once each, not once per region
    want_ok = plain_ok.copy()
    want_ok[4] = False                                                 # the narrow image loads, but has no tiles
    assert consumed == len(files) and ok.tolist() == want_ok.tolist() == [True, True, False, True, False, True]
    images = [load(clip_lib, p) for p, good in zip(files, ok) if good]
    want_boxes = np.concatenate([clip_lib.grid_boxes(im.shape[1], im.shape[0], G) for im in images])
    assert boxes.dtype == np.int32 and np.array_equal(boxes, want_boxes) and len(boxes) == 4 * R
    regions = [(i // R,) + tuple(b) for i, b in enumerate(want_boxes.tolist())]
    want = clip.encode_image_regions(images, regions)
    same_bits(vecs, want)
    # The same list walked two images at a time: the same boxes and the same rows as the one call, bit for bit; every window is also,
    # bit for bit, one regions call over that window's images (the contract of the call).
    rows, got_boxes, pos, first = [], [], 0, 0
    while pos < len(files):
        v, o, c, b = clip.encode_image_files(files[pos:], n_threads=2, max_images=2, grid=G)
        n_img = int(o.sum())
        assert c > 0 and len(v) == len(b) == R * n_img and n_img <= 2
        window = images[first:first + n_img]
        same_bits(v, clip.encode_image_regions(window, [(i // R,) + tuple(x) for i, x in enumerate(b.tolist())]))
        rows.append(v)
        got_boxes.append(b)
        pos += c
        first += n_img
    rows = np.concatenate(rows)
    assert np.array_equal(np.concatenate(got_boxes), want_boxes) and rows.shape == want.shape
    print("windows of 2 against one call: max abs diff %g" % np.abs(rows - want).max())
    same_bits(rows, want)
    # from memory
    v, o, c, b = clip.encode_image_bytes([open(p, "rb").read() for p in files], n_threads=3, grid=G)
    same_bits(v, want)
    assert np.array_equal(b, want_boxes) and o.tolist() == ok.tolist()


def test_grid_1_is_the_existing_call(clip, clip_lib, files):
    a = clip.encode_image_files(files, n_threads=3)
    b = clip.encode_image_files(files, n_threads=3, grid=1)
    assert len(b) == 3 and a[2] == b[2] and a[1].tolist() == b[1].tolist()
    same_bits(b[0], a[0])
    # and the C entry point with grid 1: the same rows, whole-image boxes
    L = clip_lib.lib()
    n = len(files)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in files])
    out = np.empty((n, a[0].shape[1]), dtype=np.float32)
    boxes = np.full((n, 4), -1, dtype=np.int32)
    ok = np.zeros(n, dtype=np.uint8)
    consumed = C.c_int(0)
    rows = L.clip_amd_image_batch_encode_files_grid(clip.ctx, arr, n, n, 3, 1, True, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                    boxes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(consumed), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rows == len(a[0]) and consumed.value == n
    same_bits(out[:rows], a[0])
    assert np.all(boxes[:rows, :2] == 0) and np.all(boxes[:rows, 2:] > 0)
    for bad in (0, 9):
        assert L.clip_amd_image_batch_encode_files_grid(clip.ctx, arr, n, n, 3, bad, True, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                        boxes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(consumed), ok.ctypes.data_as(C.POINTER(C.c_uint8))) == -1


def test_bad_boxes(clip, clip_lib, capfd):
    L = clip_lib.lib()
    images = [_photo(40, 50, 31), _photo(20, 20, 32)]
    keep, arr, n = clip._u8_array(images)
    proj = clip.vision_config["projection_dim"]
    i32p = C.POINTER(C.c_int32)

    def call(boxes, n_boxes=None):
        b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5) if boxes is not None else None
        n_boxes = len(b) if n_boxes is None else n_boxes
        vec = np.full((max(n_boxes, 1), proj), -3.0, dtype=np.float32)
        ok = L.clip_amd_image_batch_encode_regions(clip.ctx, arr, n, b.ctypes.data_as(i32p) if b is not None else None, n_boxes,
                                                   vec.ctypes.data_as(C.POINTER(C.c_float)), True)
        return ok, bool(np.all(vec == -3.0))

    good = (0, 1, 2, 10, 10)
    capfd.readouterr()
    for bad in [(0, 45, 0, 10, 10), (0, 0, 35, 10, 10), (0, -1, 0, 10, 10), (1, 0, 0, 21, 20), (0, 0, 0, 0, 10), (0, 0, 0, 10, 0),
                (2, 0, 0, 5, 5), (-1, 0, 0, 5, 5), (0, 2 ** 31 - 5, 0, 10, 10)]:
        assert call([good, bad, good]) == (False, True), bad
        assert "box 1" in capfd.readouterr().err
    assert call(None, 3) == (False, True)
    assert call([good, good]) == (True, False)
