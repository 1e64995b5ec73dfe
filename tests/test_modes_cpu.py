"""CPU tier of density modes (clip_amd_index_modes) and `image_search albums`: the numpy contract of tests/modes_common.py on hand-made pair
lists with known answers, the pure grouping of image_search.py, option parsing, usage texts and the gridded refusal of `albums`, the
checks the Python wrapper makes before the library is reached, and the refusals without a device.  Needs no device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from clip_cpp_amd import image_search
from modes_common import from_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def contract(n, pairs, radius, link, eligible=None):
    i, j, d = (np.array(c) for c in zip(*pairs)) if pairs else (np.zeros(0, dtype=np.int64),) * 3
    labels, parent, pdist, density, modes = from_pairs(n, i, j, np.asarray(d, dtype=np.float32), radius, link, eligible)
    assert labels.dtype == np.int64 and parent.dtype == np.int64 and pdist.dtype == np.float32 and density.dtype == np.int32
    return labels.tolist(), parent.tolist(), pdist.tolist(), density.tolist(), modes


def f(x):
    return float(np.float32(x))


def test_density_tie_is_broken_by_id():
    assert contract(2, [(0, 1, 0.1)], 0.2, 0.2) == ([0, 0], [-1, 0], [INF, f(0.1)], [1, 1], 1)
    assert contract(2, [], 0.2, 0.2) == ([0, 1], [-1, -1], [INF, INF], [0, 0], 2)              # singletons are modes
    assert contract(0, [], 0.2, 0.2) == ([], [], [], [], 0)


def test_equal_distances_are_broken_by_id():
    # densities 2, 2, 0, 2: rank 0 > 1 > 3; row 3 sees 0 and 1 at the same distance and takes the lower id
    got = contract(4, [(0, 3, 0.1), (1, 3, 0.1), (0, 1, 0.05)], 0.2, 0.2)
    assert got == ([0, 0, 2, 0], [-1, 0, -1, 0], [INF, f(0.05), INF, f(0.1)], [2, 2, 0, 2], 2)
    # the nearer row wins over the lower id, and a nearer row that does not outrank is no candidate
    got = contract(4, [(0, 3, 0.1), (1, 3, 0.05), (0, 1, 0.15), (2, 3, 0.01)], 0.2, 0.2)
    assert got == ([3, 3, 3, 3], [3, 3, 3, -1], [f(0.1), f(0.05), f(0.01), INF], [2, 2, 1, 3], 1)


def test_link_below_equal_and_above_radius():
    pairs = [(0, 1, 0.1), (1, 2, 0.3)]
    # radius 0.35: densities 1, 2, 1; row 2's only outranking row is 0.3 away
    assert contract(3, pairs, 0.35, 0.2) == ([1, 1, 2], [1, -1, -1], [f(0.1), INF, INF], [1, 2, 1], 2)
    assert contract(3, pairs, 0.35, 0.35) == ([1, 1, 1], [1, -1, 1], [f(0.1), INF, f(0.3)], [1, 2, 1], 1)
    # radius 0.2: densities 1, 1, 0, rank 0 > 1 > 2; the wider link reaches row 2
    assert contract(3, pairs, 0.2, 0.2) == ([0, 0, 2], [-1, 0, -1], [INF, f(0.1), INF], [1, 1, 0], 2)
    assert contract(3, pairs, 0.2, 0.35) == ([0, 0, 0], [-1, 0, 1], [INF, f(0.1), f(0.3)], [1, 1, 0], 1)
    assert contract(3, pairs, 0.2, np.inf) == contract(3, pairs, 0.2, 0.35)
    # d <= radius is compared in f32: 0.1 as f32 is above 0.1 as f64, and equal to itself
    assert contract(2, [(0, 1, 0.1)], f(0.1), f(0.1))[3] == [1, 1]
    assert contract(2, [(0, 1, 0.1)], np.nextafter(np.float32(0.1), np.float32(0)), 1.0) == ([0, 0], [-1, 0], [INF, f(0.1)], [0, 0], 1)


def test_chain_and_rows_that_are_not_eligible():
    # a path 0 - 1 - ... - 5: densities 1, 2, 2, 2, 2, 1; the interior ties go down the ids, the ends up to their only neighbour
    pairs = [(k, k + 1, 0.1) for k in range(5)]
    assert contract(6, pairs, 0.2, 0.2) == ([1] * 6, [1, -1, 1, 2, 3, 4], [f(0.1), INF] + [f(0.1)] * 4, [1, 2, 2, 2, 2, 1], 1)
    ok = np.array([True, True, False, True, True, True])
    got = contract(6, [p for p in pairs if 2 not in p[:2]], 0.2, 0.2, ok)
    assert got == ([0, 0, -1, 4, 4, 4], [-1, 0, -1, 4, -1, 4], [INF, f(0.1), INF, f(0.1), INF, f(0.1)], [1, 1, -1, 1, 2, 1], 2)
    with pytest.raises(AssertionError):
        contract(6, pairs, 0.2, 0.2, ok)


def test_album_groups_ordering_and_min():
    #          0    1    2    3    4   5    6    7    8
    labels = [4, 1, 4, 1, 4, -1, 6, 7, 7]
    dist = [0.25, INF, 0.5, 0.125, INF, INF, INF, INF, 0.0]
    got = image_search.album_groups(labels, dist, 2)
    assert got == [(4, [(0, 0.25), (2, 0.5)]), (1, [(3, 0.125)]), (7, [(8, 0.0)])]            # largest first, equal sizes by cover id
    assert all(type(c) is int and type(i) is int and type(d) is float for c, g in got for i, d in g)
    assert image_search.album_groups(labels, dist) == got                                     # the default is two
    assert image_search.album_groups(labels, dist, 3) == got[:1]
    assert image_search.album_groups(labels, dist, 4) == []
    assert image_search.album_groups(labels, dist, 1) == got + [(6, [])]
    assert image_search.album_groups(labels, dist, 0) == got + [(6, [])]
    assert image_search.album_groups([], [], 1) == []
    assert image_search.album_groups([-1, -1], [INF, INF], 1) == []


def test_albums_parsing(capsys):
    P = lambda argv: image_search._parse(list(argv), False, albums=True)
    p = P([])
    assert p["max_distance"] == image_search.DEDUP_RADIUS and p["link"] is None and p["min_size"] == 2 and p["results"] is None and p["db"] == "."
    p = P(["--db", "d", "-d", "0.2", "--link", "0.3", "--min", "1", "-n", "4", "-v", "0", "-m", "m.gguf"])
    assert (p["db"], p["max_distance"], p["link"], p["min_size"], p["results"], p["verbose"], p["model"]) == ("d", 0.2, 0.3, 1, 4, 0, "m.gguf")
    assert P(["--max-distance", "0.5", "--results", "2"])["results"] == 2
    assert P(["--link", "inf"])["link"] == float("inf")
    for bad in (["--link", "nan"], ["-d", "nan"], ["--min", "x"], ["--link"], ["-t", "2"], ["--prune"], ["pics"], ["--in", "a/"]):
        assert P(bad) is None, bad
    out = capsys.readouterr().out
    assert "unrecognized argument: -t" in out and "unexpected argument: pics" in out
    for other in (dict(build=False), dict(build=True), dict(build=False, dedup=True), dict(build=False, neighbors=True)):
        assert image_search._parse(["--link", "0.1", "x"], **other) is None                    # only albums knows it
        assert image_search._parse(["--min", "3", "x"], **other) is None
    base = image_search._parse([], build=False, dedup=True)
    assert "link" not in base and "min_size" not in base and base["results"] == 5             # dedup parses as before


def test_albums_in_usage_texts_and_docstring(capsys):
    assert image_search.main([]) == 1
    assert "image_search albums [options]" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        image_search.main(["albums", "-h"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "Usage: python -m clip_cpp_amd.image_search albums [options]" in out
    for option in ("  -d R, --max-distance R", "  --link T", "  --min N", "  -n COUNT", "  --db <dir>"):
        assert len([l for l in out.splitlines() if l.startswith(option)]) == 1, option
    assert "--threads" not in out and "--prune" not in out
    assert image_search.main(["albums", "--bogus"]) == 1 and "image_search albums [options]" in capsys.readouterr().out
    doc = image_search.__doc__
    assert "image_search albums [-m MODEL] [-v N] [--db DIR] [-d R | --max-distance R] [--link T] [--min N] [-n COUNT]" in doc
    assert "main: %d albums, %d images" in doc and "Index.modes" in doc


def test_albums_refuses_a_gridded_database_by_name_before_any_model_load(tmp_path, capsys):
    """the model of the database does not exist: a run that got as far as loading it says so on stdout"""
    d = tmp_path / "db"
    os.makedirs(d)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\n")
    (d / "images.regions").write_text("grid 2\n")
    assert image_search.main(["albums", "--db", str(d)]) == 1
    got = capsys.readouterr()
    assert "`albums` does not support such a database yet" in got.err and "images.regions" in got.err
    assert "Unable to load model" not in got.out
    os.remove(d / "images.regions")
    r = subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search", "albums", "--db", str(d)], capture_output=True, text=True,
                       env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 1 and "does not support" not in r.stderr                           # a plain database gets past the refusal


def test_wrapper_rejects_nan_and_a_malformed_allow_before_the_library(clip_lib):
    class Unreachable(clip_lib.Index):
        def __init__(self):                    # no handle: every library call would need one
            pass

        def __len__(self):
            return 10

        def _live(self):
            raise AssertionError("the library was reached")

    ix = Unreachable()
    nan = float("nan")
    for args in ((nan,), (0.1, nan), (nan, nan)):
        with pytest.raises(ValueError, match="NaN"):
            ix.modes(*args)
        with pytest.raises(ValueError, match="NaN"):
            ix.modes_device(args[0], 1, *args[1:])
    with pytest.raises(ValueError):
        ix.modes(0.1, allow=np.ones(9, dtype=bool))                                           # a mask of the wrong length
    with pytest.raises(ValueError):
        ix.modes(0.1, allow=[0, 10])                                                          # an id outside the index
    with pytest.raises(ValueError):
        ix.modes(0.1, allow=[-1])
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.modes(0.1, 0.2, allow=[0, 9])                                                      # well-formed: the call goes on


def test_entry_points_are_declared_and_refuse_without_an_index(clip_lib, capfd):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    for name in ("clip_amd_index_modes", "clip_amd_index_modes_device"):
        assert re.search(r"\b%s\(struct clip_amd_index \* ix, float radius, float link, const uint64_t \* (d_)?allow," % name, header), name
        assert name in clip_lib.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert re.search(r"float clip_amd_bench_modes\(int dtype, int64_t n, int dim, float radius, float link, int copies, int iters\);", header)
    assert "clip_amd_bench_modes" in clip_lib.AMD_SYMBOLS
    assert callable(clip_lib.Index.modes) and callable(clip_lib.Index.modes_device) and callable(clip_lib.bench_modes)
    # a host-only context holds no index (clip_amd_index_create refuses it: tests/test_search_cpu.py), so the call has none to work on
    L = clip_lib.lib()
    labels = np.full(4, -7, dtype=np.int64)
    lp = labels.ctypes.data_as(L.clip_amd_index_modes.argtypes[4])
    capfd.readouterr()
    assert L.clip_amd_index_modes(None, 0.1, 0.1, None, lp, None, None, None) == -1
    assert L.clip_amd_index_modes_device(None, 0.1, 0.1, None, labels.ctypes.data, None, None, None) is False
    assert capfd.readouterr().err.count("index is NULL") == 2 and np.all(labels == -7)
    code = "import clip_cpp_amd as c; print('us', c.bench_modes('f16', 1024, 64, 0.05, 0.1, 3, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def test_host_only_context_refuses_the_index_and_with_it_the_call(clip_lib, fixture_cache):
    from oracle import fixtures
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    code = ("import sys, clip_cpp_amd as c\n"
            "m = c.Clip(%r, verbosity=0)\n"
            "try:\n"
            "    c.Index(m, 32, 'f16').modes(0.1)\n"
            "except RuntimeError as e:\n"
            "    print('refused:', e)\n" % model)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "refused: clip_amd_index_create failed" in r.stdout and "clip_amd_index_create: host-only context" in r.stderr
