"""CPU tier of compound queries (Index.search_compound, `search --and / --not`): the option parsing and help texts, the refusal of a
gridded database before any model is loaded, the argument checks that need no device, the new entry points on NULL arguments, and the
numpy definition (tests/compound_common.py: compound) on hand-written cases."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from compound_common import ALL, BEYOND, OVER, WITHIN, compound, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clip_amd_index_search_compound", "clip_amd_index_search_compound_device", "clip_amd_test_index_compound_block",
       "clip_amd_bench_search_compound"]


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def _search(*argv):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in argv]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def _parse(argv, **kw):
    from clip_cpp_amd import image_search
    return image_search._parse(list(argv), kw.pop("build", False), **kw)


def test_compound_parsing(capsys):
    p = _parse(["--and", "on a beach", "a", "dog"])
    assert p is not None and p["and"] == ["on a beach"] and "not" not in p and "not_margin" not in p and p["rest"] == ["a", "dog"]
    p = _parse(["--and", "on a beach", "--not", "people", "--and", "pics/a.png", "--not", "cars", "--not-margin", "0.05", "-n", "3", "--in", "pics/",
                "--like", "pics/b.png"])
    assert p["and"] == ["on a beach", "pics/a.png"] and p["not"] == ["people", "cars"] and p["not_margin"] == 0.05
    assert p["results"] == 3 and p["in"] == ["pics/"] and p["like"] == "pics/b.png" and p["rest"] == []
    assert _parse(["--not", "people", "--not-margin", "-0.1", "a beach"])["not_margin"] == -0.1
    # a plain search parses to what it parsed to before
    plain = _parse(["a", "cat"])
    assert plain == dict(threads=4, verbose=1, db=".", dtype="f16", results=5, max_distance=None, model="", rest=["a", "cat"], like=None, **{"in": []})
    # --not-margin: a number, not NaN, and only with --not
    assert _parse(["--not", "people", "--not-margin", "nan", "a beach"]) is None
    assert _parse(["--not", "people", "--not-margin", "wide", "a beach"]) is None
    assert _parse(["--not", "people", "--not-margin"]) is None
    assert _parse(["--and", "x", "--not-margin", "0.1", "a beach"]) is None
    assert "--not-margin is the margin of the --not terms" in capsys.readouterr().out
    assert _parse(["--and"]) is None and _parse(["--and", "x"]) is None   # without a value; without a main query
    # the main query and 7 more terms is the limit
    seven = sum([["--and", "t%d" % i] for i in range(4)], []) + sum([["--not", "u%d" % i] for i in range(3)], [])
    assert _parse(seven + ["a cat"]) is not None
    assert _parse(seven + ["--not", "one more", "a cat"]) is None
    assert "at most 8 terms" in capsys.readouterr().out
    assert _parse(seven + ["--and", "one more", "--like", "pics/a.png"]) is None
    # not with -d, not with --distinct
    for extra in (["-d", "0.2"], ["--distinct", "0.05"]):
        assert _parse(["--and", "x"] + extra + ["a cat"]) is None and _parse(extra + ["--not", "x", "a cat"]) is None
        assert "--and / --not cannot be combined with -d or --distinct" in capsys.readouterr().out
    for mode in ({"build": True}, {"dedup": True}, {"neighbors": True}, {"update": True}, {"label": True}, {"merge": True}, {"match": True}):
        for opt in ("--and", "--not", "--not-margin"):
            assert _parse([opt, "0.05", "dir"], **mode) is None, (mode, opt)
            assert "unrecognized argument: %s" % opt in capsys.readouterr().out


def test_help_and_docstring(capsys):
    from clip_cpp_amd import image_search
    image_search._help(False, dict(threads=4, verbose=1, db=".", results=5))
    out = capsys.readouterr().out
    assert "--and <term>" in out and "--not <term>" in out and "--not-margin M" in out and "WORST term" in out and "Default: 0" in out
    image_search._help(False, dict(verbose=1, db=".", results=5), neighbors=True)
    assert "--and" not in capsys.readouterr().out
    doc = image_search.__doc__
    assert "[--and TERM]... [--not TERM]... [--not-margin M]" in doc and "--and ranks by the\nWORST term" in doc and "Index.search_compound" in doc


def test_terms_of_the_command_line():
    from clip_cpp_amd import image_search
    paths = ["pics/a.png", "pics/b.jpg", "pics/c.png"]
    p = {"and": ["on a beach", "pics/b.jpg", "elsewhere/d.png"], "not": ["people", "pics/c.png"]}
    assert image_search.compound_terms(p, paths, None, "", "a dog") == [
        ("text", "a dog", "all"), ("text", "on a beach", "all"), ("id", 1, "all"), ("file", "elsewhere/d.png", "all"), ("text", "people", "over"),
        ("id", 2, "over")]
    assert image_search.compound_terms({"not": ["pics/a.txt"]}, paths, 0, "", "") == [("id", 0, "all"), ("text", "pics/a.txt", "over")]
    assert image_search.compound_terms({"and": ["x"]}, paths, None, "q.png", "")[0] == ("file", "q.png", "all")


def _database(d, gridded):
    os.makedirs(d, exist_ok=True)
    (d / "images.paths").write_text("no/such/model.gguf\nimg/a.png\n")
    with open(d / "images.index", "wb") as f:                             # header only: nothing reads the rows before the check
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 8, 1, 5 if gridded else 1))
    if gridded:
        (d / "images.regions").write_text("grid 2\n0 0 0 10 10\n0 0 0 5 5\n0 5 0 5 5\n0 0 5 5 5\n0 5 5 5 5\n")


def test_gridded_database_is_refused_before_the_model(tmp_path):
    g, plain = tmp_path / "g", tmp_path / "plain"
    _database(g, True)
    _database(plain, False)
    for argv in (["search", "--db", g, "--and", "on a beach", "a dog"], ["search", "--db", g, "--not", "people", "--like", "img/a.png"]):
        r = _search(*argv)
        assert r.returncode == 1, (r.stdout[-1000:], r.stderr[-1000:])
        assert "was built with --grid" in r.stderr and "`search --and / --not` does not support such a database yet" in r.stderr
        assert str(g) in r.stderr and "Unable to load model" not in r.stdout
    r = _search("search", "--db", plain, "--and", "on a beach", "a dog")    # a plain database gets as far as the model, which does not exist
    assert r.returncode == 1 and "Unable to load model" in r.stdout and "--grid" not in r.stderr


def test_usage_errors_print_the_usage(tmp_path):
    _database(tmp_path / "d", False)
    for extra in (["--and", "x", "-d", "0.1", "a cat"], ["--and"], ["--not", "x", "--not-margin", "nan", "a cat"],
                  sum([["--and", "t"] for _ in range(8)], []) + ["a cat"]):
        r = _search("search", "--db", tmp_path / "d", *extra)
        assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search search" in r.stdout, extra


def test_python_argument_checks_need_no_device(clip_lib):
    I = clip_lib.Index
    v = np.ones(8, dtype=np.float32)
    two = [[(v, "all"), (3, "over"), (v * 2, "within", 0.5)], [(np.int64(7), "all"), (v, "beyond", 0.25), (v, "over", -0.1)]]
    terms, term_ids, kinds, bounds, lims = I._compound_args(two, 8)
    mine = flatten(two, 8)
    for a, b in zip((terms, term_ids, kinds, bounds, lims), mine):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert kinds.tolist() == [ALL, OVER, WITHIN, ALL, BEYOND, OVER] and lims.tolist() == [0, 3, 6] and term_ids.tolist() == [-1, 3, -1, 7, -1, -1]
    for queries, match in (([[]], "query 0 has no terms"), ([[(v, "all")], []], "query 1 has no terms"), ([[(v, "all")] * 9], "9 terms, more than 8"),
                           ([[(v, "within", 0.5), (v, "over")]], "no \"all\" term"), ([[(v, "all"), (v, "within")]], "'within' term needs a bound"),
                           ([[(v, "all"), (v, "beyond", None)]], "'beyond' term needs a bound"), ([[(v, "all"), (v, "over", float("nan"))]], "is NaN"),
                           ([[(v, "all"), (v, "within", float("nan"))]], "is NaN"), ([[(v, "any")]], "unknown kind 'any'"), ([[(v, 0)]], "unknown kind 0"),
                           ([[(np.ones(7, dtype=np.float32), "all")]], "must have 8 values"), ([[(np.ones((2, 8), dtype=np.float32), "all")]], "must have 8 values"),
                           ([[(-3, "all")]], "negative"), ([[(v,)]], "is not \\(what, kind\\)"), ([], "no queries")):
        with pytest.raises(ValueError, match=match):
            I._compound_args(queries, 8)
    ix = I.__new__(I)                                                     # no context, no handle: a check that passed would say "closed"
    ix.dim, ix.handle = 8, None
    with pytest.raises(ValueError, match="more than 8"):
        ix.search_compound([[(v, "all")] * 9], 5)
    with pytest.raises(ValueError, match="term_lims must end"):
        ix.search_compound_device(0, None, [0, 0], [0.0, 0.0], [0, 3], 5, 0, 0)
    with pytest.raises(RuntimeError, match="closed"):                     # the checks passed: only the handle is missing
        ix.search_compound([[(v, "all"), (v, "over")]], 5)


def test_new_entry_points_reject_null_arguments(clip_lib):
    L = clip_lib.lib()
    for name in NEW:
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
    assert L.clip_amd_index_search_compound(None, None, None, None, None, None, 1, 5, 1, None, None, None) is False
    assert L.clip_amd_index_search_compound_device(None, None, None, None, None, None, 1, 5, 1, None, None, None) is False
    assert L.clip_amd_test_index_compound_block(None, 3) == -1
    code = "import clip_cpp_amd as c; print('us', c.bench_search_compound('f16', 1024, 64, 4, 2, 5, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def test_the_definition_on_hand_written_cases():
    inf = np.float32(np.inf)
    f = lambda *x: np.array(x, dtype=np.float32)
    # all-of ranks by the worst term: row 1 is the best of neither term, and the best of both
    D = np.stack([f(0.1, 0.3, 0.9), f(0.9, 0.4, 0.1)])
    d, i = compound(D, [ALL, ALL], [0, 0], 3)
    assert i.tolist() == [1, 0, 2] and d.tolist() == [np.float32(0.4), np.float32(0.9), np.float32(0.9)]      # a tie at 0.9: the lower id first
    assert compound(D[:1], [ALL], [0], 2)[1].tolist() == [0, 1]
    # identical rows: the same score, the lower id first
    D = np.stack([f(0.5, 0.2, 0.5, 0.2), f(0.3, 0.6, 0.3, 0.6)])
    d, i = compound(D, [ALL, ALL], [0, 0], 4)
    assert i.tolist() == [0, 2, 1, 3] and d.tolist() == [np.float32(0.5)] * 2 + [np.float32(0.6)] * 2
    # over: d > score + bound, the sum in f32; at equality the row is not eligible
    D = np.stack([f(0.2, 0.2, 0.2, 0.2), f(0.2, 0.25, 0.5, 0.1)])
    assert compound(D, [ALL, OVER], [0, 0], 4)[1].tolist() == [1, 2, -1, -1]
    edge = np.float32(0.2) + np.float32(0.3)
    D = np.stack([f(0.2, 0.2, 0.2), np.array([edge, np.nextafter(edge, inf), np.nextafter(edge, -inf)], dtype=np.float32)])
    assert compound(D, [ALL, OVER], [0, 0.3], 3)[1].tolist() == [1, -1, -1]
    assert compound(D, [ALL, OVER], [0, -0.3], 3)[1].tolist() == [0, 1, 2]                      # a negative margin lets nearer rows through
    # with two all-terms the margin is over the score, the worse of them
    D = np.stack([f(0.1, 0.1), f(0.4, 0.2), f(0.3, 0.3)])
    assert compound(D, [ALL, ALL, OVER], [0, 0, 0], 2)[1].tolist() == [1, -1]
    # within is <=, beyond its complement; a filter can empty the result
    D = np.stack([f(0.3, 0.1, 0.2), f(0.5, 0.6, 0.7)])
    assert compound(D, [ALL, WITHIN], [0, 0.6], 3)[1].tolist() == [1, 0, -1]
    assert compound(D, [ALL, BEYOND], [0, 0.6], 3)[1].tolist() == [2, -1, -1]
    d, i = compound(D, [ALL, WITHIN], [0, 0.4], 3)
    assert i.tolist() == [-1, -1, -1] and np.isinf(d).all()
    D = np.stack([f(0.3, 0.1, 0.2), f(0.5, 0.6, 0.7), f(0.9, 0.5, 0.7)])
    assert compound(D, [WITHIN, ALL, BEYOND], [0.2, 0, 0.6], 2)[1].tolist() == [2, -1]          # the all-term need not come first
    # rows that are not live or not allowed (NaN in every term) and excluded ids are not eligible; k cuts the list
    D = np.stack([f(0.3, np.nan, 0.2, 0.1), f(0.1, np.nan, 0.1, 0.1)])
    assert compound(D, [ALL, ALL], [0, 0], 4)[1].tolist() == [3, 2, 0, -1]
    assert compound(D, [ALL, ALL], [0, 0], 4, excluded=[3, 7])[1].tolist() == [2, 0, -1, -1]
    assert compound(D, [ALL, ALL], [0, 0], 1)[1].tolist() == [3]
    with pytest.raises(AssertionError):
        compound(D, [WITHIN, OVER], [0.5, 0], 2)
