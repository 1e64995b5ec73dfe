"""CPU tier of regions and gridded image-search databases: grid_boxes tiles an image exactly; the new entry points on a NULL or host-only
context fail without a device; build --grid outside 1 ... 8 is a usage error; every sub-command that does not support a gridded database
says so and stops before it loads a model."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


@pytest.mark.parametrize("nx,ny,G", [(7, 5, 2), (7, 5, 3), (7, 5, 5), (640, 480, 3), (8, 8, 8), (9, 2, 1)])
def test_grid_boxes_tile_the_image_exactly(nx, ny, G):
    from clip_cpp_amd import grid_boxes
    b = grid_boxes(nx, ny, G)
    assert b.dtype == np.int32 and b.shape == ((1 if G == 1 else 1 + G * G), 4)
    assert b[0].tolist() == [0, 0, nx, ny]
    if G == 1:
        return
    cover = np.zeros((ny, nx), dtype=np.int32)
    for t, (x, y, w, h) in enumerate(b[1:].tolist()):
        i, j = t % G, t // G                                   # j outer, i inner
        assert (x, y) == (i * nx // G, j * ny // G) and w >= 1 and h >= 1 and x + w <= nx and y + h <= ny
        cover[y:y + h, x:x + w] += 1
    assert int((b[1:, 2].astype(np.int64) * b[1:, 3]).sum()) == nx * ny      # the areas sum to the image ...
    assert np.all(cover == 1)                                                  # ... and no pixel is covered twice


def test_grid_boxes_refuses_what_the_library_refuses():
    from clip_cpp_amd import grid_boxes
    for nx, ny, G in [(7, 5, 0), (7, 5, 9), (2, 5, 3), (5, 2, 3), (0, 5, 1)]:
        with pytest.raises(ValueError):
            grid_boxes(nx, ny, G)


def test_new_entry_points_without_a_context(clip_lib, capfd):
    L = clip_lib.lib()
    boxes = np.array([[0, 0, 0, 2, 2]], dtype=np.int32)
    bp = boxes.ctypes.data_as(C.POINTER(C.c_int32))
    vec = np.full(64, -3.0, dtype=np.float32)
    fp = vec.ctypes.data_as(C.POINTER(C.c_float))
    q = np.zeros(8, dtype=np.float32)
    ids = np.full(4, -3, dtype=np.int64)
    consumed = C.c_int(5)
    ok = np.zeros(2, dtype=np.uint8)
    paths = (C.c_char_p * 1)(b"x.png")
    capfd.readouterr()
    assert L.clip_amd_image_batch_encode_regions(None, None, 0, bp, 1, fp, True) is False
    assert L.clip_amd_image_batch_preprocess_regions_device(None, None, 0, bp, 1, None) is False
    assert capfd.readouterr().err.count("ctx is NULL") == 2
    assert L.clip_amd_image_batch_encode_files_grid(None, paths, 1, 1, 1, 2, True, fp, bp, C.byref(consumed), ok.ctypes.data_as(C.POINTER(C.c_uint8))) == -1
    assert consumed.value == 0
    assert L.clip_amd_index_search_grouped(None, q.ctypes.data_as(C.POINTER(C.c_float)), 1, 4, bp, None, fp, ids.ctypes.data_as(C.POINTER(C.c_int64))) is False
    assert L.clip_amd_index_search_grouped_device(None, None, 1, 4, None, None, None, None) is False
    assert capfd.readouterr().err.count("index is NULL") == 2
    assert np.all(vec == -3.0) and np.all(ids == -3)


def test_new_entry_points_on_a_host_only_context(fixture_cache):
    """in a process that sees no device: the calls fail with their message, nothing is written, the benchmark hook answers < 0"""
    from oracle import fixtures
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    code = """
import ctypes as C, sys
import numpy as np
import clip_cpp_amd as c
clip = c.Clip(%r, verbosity=0)
assert clip.device < 0
im = np.zeros((8, 9, 3), dtype=np.uint8)
for call in (lambda: clip.encode_image_regions([im], [(0, 0, 0, 4, 4)]), lambda: clip.preprocess_regions_device([im], [(0, 0, 0, 4, 4)], 0),
             lambda: clip.encode_image_files(["x.png"], grid=2), lambda: clip.encode_image_bytes([b"x"], grid=2)):
    try:
        call()
    except RuntimeError as e:
        print("refused:", e)
    else:
        sys.exit("a call went through without a device")
print("MICROS", c.bench_search_grouped("f16", 1024, 64, 1, 5, 4, 1))
""" % model
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("refused:") == 4 and float(r.stdout.split("MICROS")[1]) < 0
    assert r.stderr.count("no HIP device bound to this context") == 4


def _search(*args):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def test_build_grid_usage_errors(tmp_path, capsys):
    from clip_cpp_amd import image_search
    for bad in ("0", "9", "-1", "two"):
        assert image_search._parse(["--grid", bad, "pics"], True) is None
    out = capsys.readouterr().out
    assert "--grid takes 1 ... 8" in out
    assert image_search._parse(["--grid", "3", "pics"], True)["grid"] == 3
    assert "grid" not in image_search._parse(["pics"], True)
    for mode in ({"update": True}, {"dedup": True}, {"neighbors": True}, {"label": True}, {"merge": True}, {}):
        assert image_search._parse(["--grid", "2", "x"], False, **mode) is None, mode      # the flag belongs to build alone
    for bad in ("0", "9"):
        r = _search("build", "--grid", bad, "--db", tmp_path / "db", tmp_path)
        assert r.returncode == 1 and "--grid takes 1 ... 8" in r.stdout and "Usage: python -m clip_cpp_amd.image_search build" in r.stdout
        assert not (tmp_path / "db").exists()
    with pytest.raises(SystemExit):
        image_search.main(["build", "-h"])
    assert "--grid G" in capsys.readouterr().out and "--grid G" in image_search.__doc__


def _gridded_database(d):
    """a database whose model does not exist, with a hand-written images.regions: a run that got as far as loading the model says so"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "images.paths"), "w") as f:
        f.write("no/such/model.gguf\nimg/a.png\n")
    with open(os.path.join(d, "images.index"), "wb") as f:
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 8, 1, 5))
    with open(os.path.join(d, "images.regions"), "w") as f:
        f.write("grid 2\n0 0 0 10 10\n0 0 0 5 5\n0 5 0 5 5\n0 0 5 5 5\n0 5 5 5 5\n")


def test_unsupported_commands_refuse_a_gridded_database(tmp_path):
    g, plain = tmp_path / "g", tmp_path / "plain"
    _gridded_database(g)
    _gridded_database(plain)
    os.remove(plain / "images.regions")
    cases = {
        "update": ["update", "--db", g, tmp_path],
        "dedup": ["dedup", "--db", g],
        "neighbors": ["neighbors", "--db", g],
        "label": ["label", "--db", g, "a cat"],
        "merge": ["merge", "--db", g, "--from", plain],
        "search --like": ["search", "--db", g, "--like", "img/a.png"],
        "search -d": ["search", "--db", g, "-d", "0.2", "a cat"],
    }
    for name, argv in cases.items():
        r = _search(*argv)
        assert r.returncode == 1, (name, r.stdout[-1000:], r.stderr[-1000:])
        assert "was built with --grid" in r.stderr and ("`%s` does not support such a database yet" % name) in r.stderr, (name, r.stderr)
        assert str(g) in r.stderr and "Unable to load model" not in r.stdout, name
    r = _search("merge", "--db", plain, "--from", g)                       # a gridded source is refused as well
    assert r.returncode == 1 and "was built with --grid" in r.stderr and "Unable to load model" not in r.stdout
    # search itself supports the database: this run gets as far as the model, which does not exist
    r = _search("search", "--db", g, "a cat")
    assert r.returncode == 1 and "Unable to load model from no/such/model.gguf" in r.stdout and "--grid" not in r.stderr
    # a regions file that does not match the index is the size mismatch of a plain database: the rows of a second image, which neither
    # the index nor images.paths holds
    good = (g / "images.regions").read_text()
    (g / "images.regions").write_text(good + good.split("\n", 1)[1].replace("0 ", "1 ", 5).replace("\n0 ", "\n1 "))
    r = _search("search", "--db", g, "a cat")
    assert r.returncode == 1 and "index files size missmatch" in r.stdout, r.stdout + r.stderr
    # a file whose rows are not 1 + G * G per image, each image's rows together: refused by name, not searched with a wrong box
    from clip_cpp_amd import image_search
    for text in (good + "0 1 1 2 2\n", "grid 2\n" + "\n".join(["0 0 0 10 10", "1 0 0 5 5", "0 5 0 5 5", "0 0 5 5 5", "0 5 5 5 5"]) + "\n", good.replace("grid 2", "grid 9"),
                 "no header\n"):
        (g / "images.regions").write_text(text)
        with pytest.raises(ValueError):
            image_search.read_regions(str(g))
        r = _search("search", "--db", g, "a cat")
        assert r.returncode == 1 and "images.regions" in r.stderr and "Unable to load model" not in r.stdout
    (g / "images.regions").write_text(good)
    assert image_search.read_regions(str(g))[1].shape == (5, 5) and image_search.read_regions(str(plain)) is None
    # nothing was written
    assert (g / "images.paths").read_text() == "no/such/model.gguf\nimg/a.png\n"
    assert (plain / "images.paths").read_text() == "no/such/model.gguf\nimg/a.png\n" and not (plain / "images.regions").exists()
