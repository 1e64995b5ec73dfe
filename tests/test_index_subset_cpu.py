"""CPU tier (no device) of removal / subset search: the `allow` helper of clip_cpp_amd.Index, the `update` and `--in` parsing of the
image-search CLI, and the reconciliation `update` performs, as a pure function."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import clip_cpp_amd  # noqa: E402
from clip_cpp_amd import image_search  # noqa: E402


def test_allow_words_layout():
    n = 130
    ids = [0, 5, 63, 64, 127, 129]
    mask = np.zeros(n, dtype=bool)
    mask[ids] = True
    w = clip_cpp_amd.allow_words(mask, n)
    assert w.dtype == np.uint64 and w.shape == (3,)
    want = [0, 0, 0]
    for i in ids:
        want[i >> 6] |= 1 << (i & 63)                       # bit id & 63 of word id >> 6
    assert [int(x) for x in w] == want
    for form in (ids, np.array(ids[::-1] + ids, dtype=np.int32), np.array(ids, dtype=np.uint8), tuple(ids)):
        assert np.array_equal(clip_cpp_amd.allow_words(form, n), w)          # ids in any order, duplicates, any integer type
    assert [int(x) for x in clip_cpp_amd.allow_words(np.ones(64, dtype=bool), 64)] == [(1 << 64) - 1]
    assert [int(x) for x in clip_cpp_amd.allow_words(np.ones(65, dtype=bool), 65)] == [(1 << 64) - 1, 1]      # bits past n stay 0
    assert [int(x) for x in clip_cpp_amd.allow_words([], 70)] == [0, 0]
    assert clip_cpp_amd.allow_words(np.zeros(0, dtype=bool), 0).shape == (0,)                                   # the empty index
    assert clip_cpp_amd.allow_words([], 0).shape == (0,)


def test_allow_words_rejects_bad_input():
    for bad, n in ((np.ones(9, dtype=bool), 10), (np.ones(11, dtype=bool), 10), (np.ones((2, 5), dtype=bool), 10), ([10], 10), ([-1], 10),
                   ([0, 3, 1 << 40], 10), ([0], 0), (np.ones(1, dtype=bool), 0), ([0.5], 10), (["a"], 10)):
        with pytest.raises(ValueError):
            clip_cpp_amd.allow_words(bad, n)


def parse(argv, **kw):
    with redirect_stdout(io.StringIO()) as out:
        return image_search._parse(argv, **kw), out.getvalue()


def test_update_and_in_parsing():
    p, _ = parse(["--db", "d", "-v", "0", "-t", "2", "x", "y"], build=False, update=True)
    assert p["rest"] == ["x", "y"] and p["db"] == "d" and p["verbose"] == 0 and p["threads"] == 2 and p["model"] == ""
    assert parse(["--db", "d"], build=False, update=True)[0] is None                    # update needs at least one dir
    assert parse([], build=False, update=True)[0] is None
    for opt in (["--dtype", "i8"], ["-n", "3"], ["-d", "0.1"], ["--in", "x"]):          # not options of update
        assert parse(opt + ["dir"], build=False, update=True)[0] is None
    p, _ = parse(["--in", "a/", "-n", "3", "--in", "b/", "a", "cat"], build=False)
    assert p["in"] == ["a/", "b/"] and p["results"] == 3 and p["rest"] == ["a", "cat"]
    p, _ = parse(["-d", "0.5", "--in", "a/", "cat"], build=False)
    assert p["in"] == ["a/"] and p["max_distance"] == 0.5
    assert parse(["a", "cat"], build=False)[0]["in"] == []
    assert parse(["--in"], build=False)[0] is None                                      # a value is missing
    got, out = parse(["--in", "a/", "dir"], build=True)
    assert got is None and "unrecognized argument: --in" in out
    got, out = parse(["--in", "a/"], build=False, dedup=True)
    assert got is None and "unrecognized argument: --in" in out


def test_help_texts_and_usage():
    def text(**kw):
        with redirect_stdout(io.StringIO()) as out:
            image_search._help(kw.pop("build", False), dict(threads=4, verbose=1, db=".", dtype="f16", results=5, model="m"), **kw)
        return out.getvalue()

    assert "--in <prefix>" in text() and "repeated" in text()
    assert "image_search update" in text(update=True) and "--db" in text(update=True) and "--in" not in text(update=True)
    assert "--in" not in text(build=True) and "--in" not in text(dedup=True)
    with redirect_stdout(io.StringIO()) as out:
        assert image_search.main([]) == 1
    assert "update" in out.getvalue()
    assert "update" in image_search.__doc__ and "--in PREFIX" in image_search.__doc__
    with redirect_stdout(io.StringIO()) as out:
        assert image_search.main(["update"]) == 1                                        # no dir: the help, not a traceback
    assert "image_search update" in out.getvalue()


def test_reconcile():
    old = ["p/a.png", "p/b.png", "q/c.png", "gone/elsewhere.png", "p/d.png"]
    on_disk = {"p/a.png", "q/c.png", "p/d.png", "p/new1.png", "p/new0.png", "r/new2.png"}
    found = ["p/a.png", "p/d.png", "p/new0.png", "p/new1.png", "r/new2.png", "p/new0.png"]       # scan order; one dir given twice
    kept, removed, to_add = image_search.reconcile(old, found, exists=lambda p: p in on_disk)
    assert kept == [0, 2, 4]                       # q/c.png stays although no given dir holds it
    assert removed == [1, 3]                       # gone/elsewhere.png goes although it lies under no given dir
    assert to_add == ["p/new0.png", "p/new1.png", "r/new2.png"]
    assert image_search.reconcile([], [], exists=lambda p: True) == ([], [], [])
    assert image_search.reconcile(old, [], exists=lambda p: False) == ([], [0, 1, 2, 3, 4], [])
    # a path that vanished and was found again in the same scan cannot happen (found files exist); a kept path is never added twice
    assert image_search.reconcile(["x"], ["x", "x", "y"], exists=lambda p: True) == ([0], [], ["y"])
