"""CPU tier of the extents of a labelling (clip_amd_index_extents) and `image_search groups --extents` / `dedup --extents`: the numpy
reference of tests/extents_common.py against hand-made cases (ties in reach, ties in distance, singletons, a label that is not a member,
rows that are not eligible), the wrapper's refusals before the library is reached, the pure formatting of the two commands, their option
parsing and usage texts, the refusal of a gridded database before a model is loaded, and the declarations of the entry points."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

from clip_cpp_amd import image_search
from extents_common import reference, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)

# eight rows.  Group 7 = {0, 1, 2, 5}: its label, row 7, is not a member.  Rows 4 and 6 are the only members of groups 2 and 3 (row 2
# belongs to another group, row 3 to none).  Rows 3 and 7 are not members.
LABELS = np.array([7, 7, 7, -1, 2, 7, 3, -1], dtype=np.int64)
PAIRS = [(0, 1, 0.5), (0, 2, 0.5), (0, 5, 0.25), (1, 2, 0.75), (1, 5, 0.5), (2, 5, 0.5),      # inside group 7
         (0, 4, 0.125), (3, 5, 1.5), (4, 6, 1.75), (2, 3, 0.0), (6, 7, 0.25)]                 # across groups or to a row of none: ignored


def pairs_of(p):
    return (np.array([a for a, _, _ in p], dtype=np.int64), np.array([b for _, b, _ in p], dtype=np.int64),
            np.array([d for _, _, d in p], dtype=np.float32))


def test_reference_on_a_hand_made_case():
    centre, radius, diameter, reach, far, groups = reference(8, LABELS, *pairs_of(PAIRS))
    # rows 0 and 5 both reach 0.5 (each through a tie between rows 1 and 2: the lower id is reported); the lower id is the centre
    assert reach.tolist() == [0.5, 0.75, 0.75, INF, 0.0, 0.5, 0.0, INF] and reach.dtype == np.float32
    assert far.tolist() == [1, 2, 1, -1, -1, 1, -1, -1]
    assert centre.tolist() == [0, 0, 0, -1, 4, 0, 6, -1]
    assert radius.tolist() == [0.5, 0.5, 0.5, INF, 0.0, 0.5, 0.0, INF]
    assert diameter.tolist() == [0.75, 0.75, 0.75, INF, 0.0, 0.75, 0.0, INF]
    assert groups == 3


def test_reference_honours_eligibility_and_nan():
    eligible = np.array([1, 0, 1, 1, 1, 1, 1, 1], dtype=bool)            # row 1 leaves group 7
    centre, radius, diameter, reach, far, groups = reference(8, LABELS, *pairs_of(PAIRS), eligible=eligible)
    assert reach.tolist() == [0.5, INF, 0.5, INF, 0.0, 0.5, 0.0, INF]
    assert far.tolist() == [2, -1, 0, -1, -1, 2, -1, -1]
    assert centre.tolist() == [0, -1, 0, -1, 4, 0, 6, -1] and groups == 3
    assert diameter.tolist() == [0.5, INF, 0.5, INF, 0.0, 0.5, 0.0, INF]
    # a NaN pair is not a pair: two members of one group without a pair are each reported like the only member of a group
    centre, radius, diameter, reach, far, groups = reference(2, [1, 1], [0], [1], [np.nan])
    assert centre.tolist() == [0, 0] and reach.tolist() == [0.0, 0.0] and far.tolist() == [-1, -1] and groups == 1
    # a slightly negative distance (copies in f32) is a reach like any other, below the 0 of a single row
    centre, radius, diameter, reach, far, groups = reference(3, [0, 0, 2], [0], [1], [-1e-7])
    assert reach.tolist() == [np.float32(-1e-7), np.float32(-1e-7), 0.0] and far.tolist() == [1, 0, -1] and groups == 2
    assert reference(0, [], [], [], [])[5] == 0


def test_reference_against_brute_force_with_ties():
    rng = np.random.default_rng(3)
    for n in (5, 9, 14):
        i, j = np.triu_indices(n, 1)
        d = (rng.integers(0, 4, len(i)) / np.float32(4)).astype(np.float32)
        labels = rng.integers(-1, 3, n).astype(np.int64)
        got = reference(n, labels, i, j, d)
        full = np.zeros((n, n), dtype=np.float32)
        full[i, j] = full[j, i] = d
        for x in range(n):
            g = [y for y in range(n) if labels[y] == labels[x] and labels[y] >= 0]
            if labels[x] < 0:
                assert got[0][x] == -1 and got[3][x] == INF and got[4][x] == -1
                continue
            reach = {y: max([full[y, z] for z in g if z != y], default=np.float32(0)) for y in g}
            assert got[3][x] == reach[x]
            assert got[4][x] == min([z for z in g if z != x and full[x, z] == reach[x]], default=-1)
            assert got[0][x] == min(g, key=lambda y: (reach[y], y))
            assert got[1][x] == reach[int(got[0][x])] and got[2][x] == max(reach.values())
        assert same_bits(got[:5], reference(n, labels, i, j, d)[:5])


def test_extent_groups_on_fixed_arrays():
    centre, radius, diameter, reach, far, _ = reference(8, LABELS, *pairs_of(PAIRS))
    found = image_search.extent_groups(LABELS, centre, radius, diameter, reach, 2)
    assert found == [(0, 0.5, 0.75, [(1, 0.75), (2, 0.75), (5, 0.5)])]
    found = image_search.extent_groups(LABELS, centre, radius, diameter, reach, 1)
    assert [(c, len(m)) for c, _, _, m in found] == [(0, 3), (4, 0), (6, 0)]                  # in order of the lowest id
    assert found[1] == (4, 0.0, 0.0, [])
    # a centre that is not its group's lowest id comes first all the same; largest_first sorts by size, then by the lowest id
    labels = np.array([0, 0, 0, 3, 3, 3, 3, -1], dtype=np.int64)
    centre = np.array([1, 1, 1, 5, 5, 5, 5, -1], dtype=np.int64)
    radius = np.array([.25, .25, .25, .5, .5, .5, .5, np.inf], dtype=np.float32)
    diameter = np.array([.5, .5, .5, 1, 1, 1, 1, np.inf], dtype=np.float32)
    reach = np.array([.5, .25, .5, 1, .75, .5, 1, np.inf], dtype=np.float32)
    assert image_search.extent_groups(labels, centre, radius, diameter, reach, 2) == [
        (1, 0.25, 0.5, [(0, 0.5), (2, 0.5)]), (5, 0.5, 1.0, [(3, 1.0), (4, 0.75), (6, 1.0)])]
    assert [g[0] for g in image_search.extent_groups(labels, centre, radius, diameter, reach, 2, largest_first=True)] == [5, 1]
    assert image_search.extent_groups(labels, centre, radius, diameter, reach, 5) == []
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        worst = image_search._print_extent_groups(image_search.extent_groups(labels, centre, radius, diameter, reach, 2), list("abcdefgh"))
    assert buf.getvalue() == ("  0.250000 0.500000 b\n  0.500000 a\n  0.500000 c\n\n"
                              "  0.500000 1.000000 f\n  1.000000 d\n  0.750000 e\n  1.000000 g\n") and worst == 1.0


def test_wrapper_checks_the_labels_before_the_library(clip_lib):
    class Unreachable(clip_lib.Index):
        def __init__(self):                    # no handle: every library call would need one
            pass

        def __len__(self):
            return 10

        def _live(self):
            raise AssertionError("the library was reached")

    ix = Unreachable()
    with pytest.raises(ValueError, match="9 entries"):
        ix.extents(np.zeros(9, dtype=np.int64))
    with pytest.raises(ValueError, match="11 entries"):
        ix.extents(np.zeros(11, dtype=np.int64))
    with pytest.raises(ValueError, match="labels holds 10"):
        ix.extents([0, 1, 2, 3, 4, 5, 6, 7, 8, 10])
    with pytest.raises(ValueError, match="integers"):
        ix.extents(np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError):
        ix.extents(np.zeros(10, dtype=np.int64), allow=np.ones(9, dtype=bool))
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.extents([-1, -5, 9, 0, 0, 0, 0, 0, 0, 0])                     # any negative label and len - 1 are fine
    with pytest.raises(AssertionError, match="the library was reached"):
        ix.extents_device(1, 1)


def test_option_parsing_and_usage_texts(capsys):
    G = lambda argv: image_search._parse(argv, build=False, groups=True)
    D = lambda argv: image_search._parse(argv, build=False, dedup=True)
    assert G(["-n", "4", "--extents"])["extents"] is True and "extents" not in G(["-n", "4"])
    assert D(["--extents", "--prune"])["extents"] is True and "extents" not in D(["--prune"])
    for other in (dict(build=False), dict(build=False, levels=True), dict(build=False, albums=True), dict(build=False, spread=True)):
        assert image_search._parse(["--extents", "-n", "3", "x"], **other) is None          # only groups and dedup know it
    assert "unrecognized argument: --extents" in capsys.readouterr().out
    for cmd in ("groups", "dedup"):
        with pytest.raises(SystemExit) as e:
            image_search.main([cmd, "-h"])
        out = capsys.readouterr().out
        assert e.value.code == 0 and len([l for l in out.splitlines() if l.startswith("  --extents: ")]) == 1
        assert "radius diameter path" in out
    with pytest.raises(SystemExit):
        image_search.main(["levels", "-h"])
    assert "--extents" not in capsys.readouterr().out
    doc = image_search.__doc__
    assert "[-d R | --max-distance R] [--prune] [--extents]" in doc and "-n N [--in PREFIX]... [--min M] [--extents]" in doc
    assert "Index.extents" in doc and "largest diameter %f" in doc and "keeps each\ngroup's centre" in doc


def test_a_gridded_database_is_refused_before_any_model_load(tmp_path, capsys):
    d = tmp_path / "db"
    os.makedirs(d)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\nimg/b.png\n")
    (d / "images.regions").write_text("grid 2\n")
    for argv in (["groups", "--db", str(d), "-n", "2", "--extents"], ["dedup", "--db", str(d), "--extents"],
                 ["dedup", "--db", str(d), "--prune", "--extents"]):
        assert image_search.main(argv) == 1
        got = capsys.readouterr()
        assert "`%s` does not support such a database yet" % argv[0] in got.err and "Unable to load model" not in got.out


def test_entry_points_are_declared_and_refuse_without_an_index(clip_lib, capfd):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    init = open(os.path.join(ROOT, "clip_cpp_amd", "__init__.py")).read()
    assert re.search(r"int64_t clip_amd_index_extents\(struct clip_amd_index \* ix, const int64_t \* labels, const uint64_t \* allow, "
                     r"int64_t \* centre, float \* radius,\s+float \* diameter, float \* reach, int64_t \* far\);", header)
    assert re.search(r"bool clip_amd_index_extents_device\(struct clip_amd_index \* ix, const int64_t \* d_labels, const uint64_t \* d_allow, "
                     r"int64_t \* d_centre,\s+float \* d_radius, float \* d_diameter, float \* d_reach, int64_t \* d_far, int64_t \* d_count\);",
                     header)
    assert re.search(r"float clip_amd_bench_extents\(int dtype, int64_t n, int dim, int group_size, int sorted, int iters\);", header)
    assert re.search(r"int64_t clip_amd_test_index_extents_route\(struct clip_amd_index \* ix, int route\);", header)
    for name in ("clip_amd_index_extents", "clip_amd_index_extents_device", "clip_amd_bench_extents", "clip_amd_test_index_extents_route"):
        assert name in clip_lib.AMD_SYMBOLS
        assert "L.%s.restype" % name in init and "L.%s.argtypes" % name in init
    assert "Device memory beyond the index: 24 bytes per row" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "owner = ix.spread(n)[2]" in integration and "ix.extents(owner)" in integration and "24 bytes per row" in integration
    for name in ("extents", "extents_device", "extents_route"):
        assert callable(getattr(clip_lib.Index, name))
    assert callable(clip_lib.bench_extents)
    L = clip_lib.lib()
    ids = np.full(4, -7, dtype=np.int64)
    flt = np.full(4, -7, dtype=np.float32)
    i64p, f32p = L.clip_amd_index_extents.argtypes[1], L.clip_amd_index_extents.argtypes[4]
    capfd.readouterr()
    assert L.clip_amd_index_extents(None, ids.ctypes.data_as(i64p), None, ids.ctypes.data_as(i64p), flt.ctypes.data_as(f32p), None, None, None) == -1
    assert L.clip_amd_index_extents_device(None, ids.ctypes.data, None, ids.ctypes.data, flt.ctypes.data, None, None, None, None) is False
    assert L.clip_amd_test_index_extents_route(None, 0) == -1
    assert capfd.readouterr().err.count("index is NULL") == 2
    assert np.all(ids == -7) and np.all(flt == -7)


def test_build_lists_name_the_kernel_file():
    mk = re.search(r"^KERNELS := (.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1).split()
    src = re.search(r"^HIP_SOURCES = \[(.*)\]$", open(os.path.join(ROOT, "clip_cpp_amd", "build.py")).read(), re.M).group(1)
    src = [s.strip().strip('"')[:-4] for s in src.split(",")]
    assert "k_extents" in mk and mk.index("k_extents") == src.index("k_extents")
    assert os.path.exists(os.path.join(ROOT, "clip_cpp_amd", "csrc", "k_extents.hip"))
