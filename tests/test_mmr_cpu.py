"""CPU tier of diversified search (`search --diverse L`): the entry points, the option parsing, the checks that need no device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clip_amd_index_search_mmr", "clip_amd_index_search_mmr_device", "clip_amd_index_search_ids_mmr", "clip_amd_test_index_mmr_route",
       "clip_amd_bench_search_mmr"]


def _parse(argv):
    from clip_cpp_amd import image_search
    return image_search._parse(list(argv), False)


def test_entry_points_are_declared_and_bound(clip_lib):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    L = clip_lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in clip_lib.AMD_SYMBOLS and getattr(L, name).argtypes is not None, name
    assert L.clip_amd_index_search_mmr(None, None, 1, 5, 0.5, 0, None, None, None, None) is False
    assert L.clip_amd_index_search_ids_mmr(None, None, 1, 5, 0.5, 0, 1, None, None, None, None) is False
    assert L.clip_amd_test_index_mmr_route(None, 1) == -1


def test_diverse_parsing(capsys):
    plain = _parse(["a", "cat"])
    assert "diverse" not in plain                                         # a plain search is what it was
    p = _parse(["--diverse", "0.5", "a", "cat"])
    assert p is not None and p.pop("diverse") == 0.5 and p == plain
    p = _parse(["--diverse", "1", "-n", "1024", "--in", "pics/", "--like", "pics/a.png"])
    assert p["diverse"] == 1.0 and p["results"] == 1024 and p["in"] == ["pics/"] and p["like"] == "pics/a.png"
    for bad in (["--diverse"], ["--diverse", "nan", "a cat"], ["--diverse", "1.5", "a cat"], ["--diverse", "-0.1", "a cat"],
                ["--diverse", "much", "a cat"]):
        assert _parse(bad) is None, bad
    capsys.readouterr()
    for extra in (["--distinct", "0.05"], ["--debias"], ["--prob"], ["--and", "a dog"], ["--not", "a dog"], ["-d", "0.2"], ["--offset", "3"],
                  ["-n", "1025"]):
        assert _parse(["--diverse", "0.5"] + extra + ["a cat"]) is None, extra
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "--diverse L re-ranks" in out, (extra, out)
    from clip_cpp_amd import image_search
    for mode in ("dedup", "neighbors", "label"):
        assert image_search._parse(["--diverse", "0.5", "x"], False, **{mode: True}) is None, mode


def test_python_argument_checks_need_no_device(clip_lib):
    ix = clip_lib.Index.__new__(clip_lib.Index)                           # no context, no handle: a check that passed would say "closed"
    ix.dim, ix.handle = 8, None
    q = np.zeros((3, 8), dtype=np.float32)
    for k, lam, pool, word in ((6, 0.5, 5, "k = 6 exceeds pool = 5"), (0, 0.5, 0, "k = 0 outside"), (5, 0.5, 1025, "pool = 1025 outside"),
                               (5, float("nan"), 0, "lambda is NaN"), (5, 1.25, 0, "lambda = 1.25 outside"), (5, -1, 0, "lambda = -1 outside")):
        for call in (lambda: ix.search_mmr(q, k, lam, pool=pool), lambda: ix.search_ids_mmr([0], k, lam, pool=pool),
                     lambda: ix.search_mmr_device(0, 1, k, lam, 0, 0, 0, pool=pool)):
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="queries must be"):
        ix.search_mmr(np.zeros((3, 7), dtype=np.float32), 5, 0.5)
    with pytest.raises(RuntimeError, match="closed"):                     # the checks passed: only the handle is missing
        ix.search_mmr(q, 5, 0.0)
