"""CPU tier of farthest-first selection (clip_amd_index_spread) and `image_search spread`: the numpy contract of tests/spread_common.py on
hand-made matrices with known answers, its 2-approximation against a brute-force optimum, the pure formatting of image_search.py, option
parsing, usage texts and the refusals of `spread`, the checks the Python wrapper makes before the library is reached, and the refusals
without a device.  Needs no device."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from clip_cpp_amd import image_search
from spread_common import matrix_from_pairs, spread_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def f(x):
    return float(np.float32(x))


def line(points):
    """the matrix of points on a line: |a - b|, all exact in f32 for small integers and halves"""
    x = np.asarray(points, dtype=np.float32)
    return np.abs(x[:, None] - x[None, :])


def contract(D, n_max, **kw):
    c, r, o, od, cover = spread_contract(D, n_max, **kw)
    assert c.dtype == np.int64 and r.dtype == np.float32 and o.dtype == np.int64 and od.dtype == np.float32 and np.float32(cover).dtype == np.float32
    return c.tolist(), r.tolist(), o.tolist(), od.tolist(), float(cover)


def test_points_on_a_line():
    D = line([0, 1, 2, 3, 10, 11, 20])
    # from row 0: the far end, then 10 (10 from 0 and from 20: gaps 10 | 9 at 11), then 3 (gap 3) ...
    assert contract(D, 1) == ([0], [INF], [0] * 7, [0, 1, 2, 3, 10, 11, 20], 20.0)
    assert contract(D, 2) == ([0, 6], [INF, 20.0], [0, 0, 0, 0, 0, 6, 6], [0, 1, 2, 3, 10, 9, 0], 10.0)      # 10 is as near to 0 as to 20: the earlier centre
    assert contract(D, 3) == ([0, 6, 4], [INF, 20.0, 10.0], [0, 0, 0, 0, 4, 4, 6], [0, 1, 2, 3, 0, 1, 0], 3.0)
    c, r, o, od, cover = contract(D, 7)
    assert c == [0, 6, 4, 3, 1, 2, 5] and r == [INF, 20.0, 10.0, 3.0, 1.0, 1.0, 1.0] and o == list(range(7)) and od == [0.0] * 7 and cover == 0.0
    for k in range(1, 7):                            # every prefix is the shorter call, and reach[k] is the cover radius of the k before it
        ck, rk, _, _, coverk = contract(D, k)
        assert ck == c[:k] and rk == r[:k] and coverk == r[k]


def test_exact_ties_lowest_id_is_picked_and_the_earliest_centre_owns():
    D = line([0, 5, -5, 5, -5])
    # rows 1 ... 4 are all 5 from row 0: row 1 is picked; then rows 2 and 4 (10 from row 1, 5 from row 0): row 2; row 3 is 0 from row 1
    c, r, o, od, cover = contract(D, 3)
    assert c == [0, 1, 2] and r == [INF, 5.0, 5.0]
    assert o == [0, 1, 2, 1, 2] and od == [0.0, 0.0, 0.0, 0.0, 0.0] and cover == 0.0
    by_id = []
    spread_contract(D, 5, picks_by_id=by_id)
    assert by_id == [True, True, True, False]        # 1 of {1, 2, 3, 4}, 2 of {2, 4}, 3 of {3, 4} (both copies of a centre: gap 0), then 4 alone
    # ownership ties: row 2 is 1 from both seeds; the earlier seed in the ORDER GIVEN wins, not the lower id
    D = line([0, 2, 1])
    assert contract(D, 2, seeds=[0, 1])[2] == [0, 1, 0]
    assert contract(D, 2, seeds=[1, 0])[2] == [0, 1, 1]


def test_seeds_and_a_stop_radius_met_mid_way():
    D = line([0, 1, 2, 3, 10, 11, 20])
    assert contract(D, 7, seeds=[4])[:2] == ([4, 0, 6, 3, 1, 2, 5], [INF, 10.0, 10.0, 3.0, 1.0, 1.0, 1.0])
    assert contract(D, 3, seeds=[5, 1]) == ([5, 1, 6], [INF, INF, 9.0], [1, 1, 1, 1, 5, 5, 6], [1, 0, 1, 2, 1, 0, 0], 2.0)
    assert contract(D, 2, seeds=[5, 1])[0] == [5, 1]                                            # n_max == the seeds: pure assignment
    # stop: gap <= radius ends the traversal without the row
    assert contract(D, 7, stop=3.0)[:2] == ([0, 6, 4], [INF, 20.0, 10.0])
    assert contract(D, 7, stop=2.5)[:2] == ([0, 6, 4, 3], [INF, 20.0, 10.0, 3.0])
    assert contract(D, 7, stop=2.5)[4] == 1.0
    assert contract(D, 7, stop=100.0) == ([0], [INF], [0] * 7, [0, 1, 2, 3, 10, 11, 20], 20.0)  # above every distance: the first row alone
    assert contract(D, 7, stop=100.0, seeds=[3, 2])[:2] == ([3, 2], [INF, INF])                 # ... or the seeds, whatever their distances
    assert contract(D, 7, stop=-INF) == contract(D, 7)


def test_n_max_beyond_the_eligible_count_and_ineligible_rows():
    D = line([0, 1, 2, 3, 10, 11, 20])
    assert contract(D, 1000) == contract(D, 7)
    ok = np.array([0, 1, 1, 0, 1, 1, 0], dtype=bool)
    c, r, o, od, cover = contract(D, 2, eligible=ok)
    assert c == [1, 5] and r == [INF, 10.0]          # the lowest eligible id starts; row 6 (20) is not there to be picked
    assert o == [-1, 1, 1, -1, 5, 5, -1] and od == [INF, 0.0, 1.0, INF, 1.0, 0.0, INF] and cover == 1.0
    c, r, o, od, cover = contract(D, 1000, eligible=ok)
    assert sorted(c) == [1, 2, 4, 5] and cover == 0.0 and o == [-1, 1, 2, -1, 4, 5, -1]
    assert contract(D, 3, eligible=np.zeros(7, dtype=bool)) == ([], [], [-1] * 7, [INF] * 7, 0.0)
    assert contract(np.zeros((0, 0), np.float32), 3) == ([], [], [], [], 0.0)
    with pytest.raises(AssertionError):
        spread_contract(D, 3, seeds=[0], eligible=ok)                                           # a seed that is not eligible
    with pytest.raises(AssertionError):
        spread_contract(D, 3, seeds=[1, 1])
    with pytest.raises(AssertionError):
        spread_contract(D, 1, seeds=[1, 2])


def test_matrix_from_pairs():
    D = matrix_from_pairs(3, [0, 0], [1, 2], np.array([0.5, 0.25], dtype=np.float32))
    assert D.dtype == np.float32 and D.tolist() == [[INF, 0.5, 0.25], [0.5, INF, INF], [0.25, INF, INF]]


@pytest.mark.parametrize("seed", range(5))
def test_every_prefix_is_a_2_approximation_of_the_best_k_centres(seed):
    rng = np.random.default_rng(seed)
    pts = rng.random((12, 2))
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    for k in range(1, 5):
        best = min(D[list(cs)].min(0).max() for cs in itertools.combinations(range(12), k))
        c, r, o, od, cover = spread_contract(D, k)
        assert len(c) == k and cover <= 2 * best * (1 + 1e-6)
        assert cover == np.where(np.isin(np.arange(12), c), 0, D[c].min(0)).max()                # the cover radius is what it says
        assert np.array_equal(od, np.where(np.isin(np.arange(12), c), 0, D[c].min(0)).astype(np.float32))


def test_spread_lines():
    paths = ["img/a.png", "img/b.png", "img/c.png", "img/d.png", "img/e.png"]
    owner = np.array([0, 2, 2, 0, -1])               # row 4 is not eligible
    got = image_search.spread_lines([2, 3], np.array([np.inf, 0.75], dtype=np.float32), np.array([2, 2, 2, 3, -1]), paths)
    assert got == ["inf img/c.png (+2)", "0.750000 img/d.png (+0)"]
    got = image_search.spread_lines([2, 0], np.array([np.inf, 0.75], dtype=np.float32), owner, paths)
    assert got == ["inf img/c.png (+1)", "0.750000 img/a.png (+1)"]
    assert image_search.spread_lines([], [], np.array([-1, -1]), paths[:2]) == []
    assert image_search.spread_lines([1], [np.inf], np.array([1, 1]), paths[:2]) == ["inf img/b.png (+1)"]
    assert image_search.spread_lines(np.array([0]), np.array([np.inf]), np.array([0]), paths[:1]) == ["inf img/a.png (+0)"]


def test_spread_option_parsing():
    P = lambda argv: image_search._parse(argv, build=False, spread=True)
    p = P(["--db", "d", "-n", "4"])
    assert p["db"] == "d" and p["results"] == 4 and p["max_distance"] is None and p["in"] == [] and p["from"] == []
    p = P(["-n", "4", "-d", "0.25", "--in", "a/", "--in", "b/", "--from", "a/1.png", "--from", "b/2.png", "-v", "0"])     # -n and -d go together here
    assert p["results"] == 4 and p["max_distance"] == 0.25 and p["in"] == ["a/", "b/"] and p["from"] == ["a/1.png", "b/2.png"] and p["verbose"] == 0
    assert P(["--results", "2", "--max-distance", "0.5"])["max_distance"] == 0.5
    assert P([]) is None and P(["--db", "d"]) is None                                           # -n is the question: no default
    assert P(["-n"]) is None and P(["-n", "x"]) is None and P(["-n", "3", "-d", "nan"]) is None
    assert P(["-n", "0"]) is None and P(["-n", "-2"]) is None
    assert P(["-n", "1", "--from", "a", "--from", "b"]) is None                                 # fewer picks than seeds
    assert P(["-n", "5", "--from", "a", "--from", "a"]) is None                                 # a seed twice
    assert P(["-n", "3", "query"]) is None and P(["-n", "3", "--link", "0.1"]) is None and P(["-n", "3", "-t", "2"]) is None
    assert P(["-n", "3", "--like", "a"]) is None
    assert image_search._parse(["-n", "3", "-d", "0.5", "q"], build=False) is None              # search still refuses -n with -d
    assert image_search._parse(["--from", "a", "q"], build=False) is None                       # and has no --from


def test_spread_usage_texts(capsys):
    assert image_search.main(["spread"]) == 1
    out = capsys.readouterr().out
    assert "image_search spread [options] -n N" in out and "--from <indexed/image/path>" in out and "--in <prefix>" in out and "-d R" in out
    with pytest.raises(SystemExit) as e:
        image_search.main(["spread", "-h"])
    assert e.value.code == 0 and "image_search spread [options] -n N" in capsys.readouterr().out
    assert image_search.main(["spread", "-n", "1", "--from", "a", "--from", "b"]) == 1
    assert "at least the 2 given with --from" in capsys.readouterr().out
    assert image_search.main(["nothing"]) == 1 and "image_search spread [options] -n N" in capsys.readouterr().out
    doc = image_search.__doc__
    assert "image_search spread [-m MODEL] [-v N] [--db DIR] -n N [-d R] [--in PREFIX]... [--from INDEXED/IMAGE/PATH]..." in doc
    assert "main: %d images, every other image within %f of one of them" in doc and "Index.spread" in doc


def test_spread_refusals_before_any_model_load(tmp_path, capsys):
    """the model of the database does not exist: a run that got as far as loading it says so on stdout"""
    d = tmp_path / "db"
    os.makedirs(d)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\nimg/b.png\nother/c.png\n")
    (d / "images.regions").write_text("grid 2\n")
    assert image_search.main(["spread", "--db", str(d), "-n", "2"]) == 1
    got = capsys.readouterr()
    assert "`spread` does not support such a database yet" in got.err and "images.regions" in got.err and "Unable to load model" not in got.out
    os.remove(d / "images.regions")
    with open(d / "images.index", "wb") as fh:       # a header is all _read_db looks at: 3 rows
        import struct
        fh.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 32, 1, 3))
    assert image_search.main(["spread", "--db", str(d), "-n", "2", "--from", "img/nope.png"]) == 1
    got = capsys.readouterr()
    assert "'img/nope.png' is not in the database" in got.err and "Unable to load model" not in got.out
    assert image_search.main(["spread", "--db", str(d), "-n", "2", "--in", "img/", "--from", "other/c.png"]) == 1
    got = capsys.readouterr()
    assert "'other/c.png' does not start with an --in prefix" in got.err and "Unable to load model" not in got.out


def test_wrapper_rejects_bad_arguments_before_the_library(clip_lib):
    class Unreachable(clip_lib.Index):
        def __init__(self):                    # no handle: every library call would need one
            pass

        def __len__(self):
            return 10

        def live_mask(self):
            m = np.ones(10, dtype=bool)
            m[3] = False
            return m

        def _live(self):
            raise AssertionError("the library was reached")

    ix = Unreachable()
    with pytest.raises(ValueError, match="NaN"):
        ix.spread(3, float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        ix.spread_device(3, 1, float("nan"))
    for n, seeds in ((0, None), (-1, None), (1, [0, 1]), (0, [])):
        with pytest.raises(ValueError, match="at least"):
            ix.spread(n, seeds=seeds)
        with pytest.raises(ValueError, match="at least"):
            ix.spread_device(n, 1, seeds=seeds)
    with pytest.raises(ValueError, match="twice"):
        ix.spread(3, seeds=[1, 2, 1])
    with pytest.raises(ValueError):
        ix.spread(3, seeds=[10])                                                                # outside the index
    with pytest.raises(ValueError):
        ix.spread(3, seeds=[-1])
    with pytest.raises(ValueError, match="seed 3 is removed or not allowed"):
        ix.spread(3, seeds=[1, 3])                                                              # removed
    with pytest.raises(ValueError, match="seed 2 is removed or not allowed"):
        ix.spread(3, seeds=[2], allow=[0, 1])                                                   # not allowed
    with pytest.raises(ValueError):
        ix.spread_device(3, 1, seeds=[1, 1])
    with pytest.raises(ValueError):
        ix.spread(3, allow=np.ones(9, dtype=bool))                                              # a mask of the wrong length
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.spread(3, 0.5, seeds=[1, 0], allow=[0, 1, 9])                                        # well-formed: the call goes on
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.spread_device(3, 1, seeds=[1, 0])


def test_entry_points_are_declared_and_refuse_without_an_index(clip_lib, capfd):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    for name in ("clip_amd_index_spread", "clip_amd_index_spread_device"):
        assert re.search(r"\b%s\(struct clip_amd_index \* ix, int64_t n_max, float stop_radius, const int64_t \* seeds, int64_t n_seeds,\s+"
                         r"const uint64_t \* (d_)?allow," % name, header), name
        assert name in clip_lib.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert re.search(r"float clip_amd_bench_spread\(int dtype, int64_t n, int dim, int64_t n_max, int copies, int iters\);", header)
    assert "clip_amd_bench_spread" in clip_lib.AMD_SYMBOLS
    assert callable(clip_lib.Index.spread) and callable(clip_lib.Index.spread_device) and callable(clip_lib.bench_spread)
    # a host-only context holds no index (clip_amd_index_create refuses it: tests/test_search_cpu.py), so the call has none to work on
    L = clip_lib.lib()
    centres = np.full(4, -7, dtype=np.int64)
    cp = centres.ctypes.data_as(L.clip_amd_index_spread.argtypes[6])
    capfd.readouterr()
    assert L.clip_amd_index_spread(None, 4, 0.1, None, 0, None, cp, None, None, None, None) == -1
    assert L.clip_amd_index_spread_device(None, 4, 0.1, None, 0, None, centres.ctypes.data, None, None, None, None, None) is False
    assert capfd.readouterr().err.count("index is NULL") == 2 and np.all(centres == -7)
    code = "import clip_cpp_amd as c; print('us', c.bench_spread('f16', 1024, 64, 16, 0, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def test_build_lists_name_the_kernel_file_in_the_same_position():
    mk = re.search(r"^KERNELS := (.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1).split()
    src = re.search(r"^HIP_SOURCES = \[(.*)\]$", open(os.path.join(ROOT, "clip_cpp_amd", "build.py")).read(), re.M).group(1)
    src = [s.strip().strip('"')[:-4] for s in src.split(",")]
    assert "k_spread" in mk and mk.index("k_spread") == src.index("k_spread")
    assert os.path.exists(os.path.join(ROOT, "clip_cpp_amd", "csrc", "k_spread.hip"))
