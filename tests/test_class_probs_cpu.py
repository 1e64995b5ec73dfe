"""CPU tier of the class probabilities (`file --prob`, `audit --prob`): the entry points, the option parsing, the checks that need no device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clip_amd_index_class_probs", "clip_amd_index_class_probs_ids", "clip_amd_index_class_probs_device", "clip_amd_bench_class_probs"]


def _parse(argv, file):
    from clip_cpp_amd import image_search
    return image_search._parse_vote(list(argv), file)


def test_entry_points_are_declared_and_bound(clip_lib):
    header = open(os.path.join(ROOT, "include", "clip_amd.h")).read()
    L = clip_lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in clip_lib.AMD_SYMBOLS and getattr(L, name).argtypes is not None, name
    assert L.clip_amd_index_class_probs(None, None, 1, None, 2, 1, 100.0, None, None, None, None, None) is False
    assert L.clip_amd_index_class_probs_ids(None, None, 1, None, 2, 1, 100.0, 1, None, None, None, None, None) is False
    assert L.clip_amd_index_class_probs_device(None, None, 1, None, 2, 1, 100.0, None, None, None, None, None) is False


def test_prob_parsing(capsys):
    for file, rest in ((True, ["a.png"]), (False, [])):
        plain = _parse(rest, file)
        assert plain is not None and "prob" not in plain and "scale" not in plain      # a plain command is what it was
        p = _parse(["--prob"] + rest, file)
        assert p.pop("prob") is True and p == plain
        p = _parse(["--prob", "--scale", "20", "--in", "pics/"] + rest, file)
        assert p["prob"] is True and p["scale"] == 20.0 and p["in"] == ["pics/"]
        for bad in (["--scale", "20"], ["--prob", "--scale"], ["--prob", "--scale", "nan"], ["--prob", "--scale", "0"], ["--prob", "--scale", "x"]):
            assert _parse(bad + rest, file) is None, bad
        capsys.readouterr()
        assert _parse(["--prob", "-k", "5"] + rest, file) is None
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "--prob cannot be combined with -k" in out, out
    assert _parse(["-k", "5", "-n", "2", "a.png"], True) == dict(threads=4, verbose=1, db=".", model="", k=5, results=2, labels=None, rest=["a.png"],
                                                                 **{"in": []})


def test_python_argument_checks_need_no_device(clip_lib):
    ix = clip_lib.Index.__new__(clip_lib.Index)                           # no context, no handle: a check that passed would say "closed"
    ix.dim, ix.handle = 8, None
    q = np.zeros((3, 8), dtype=np.float32)
    none = np.zeros(0, dtype=np.int32)                                    # (an index without a handle has no rows: n_classes is 1)
    for m, scale, word in ((0, 100.0, "m = 0"), (2, 100.0, "m = 2, n_classes = 1"), (1, float("nan"), "scale is NaN"), (1, 0.0, "scale = 0 is not"),
                           (1, float("inf"), "scale = inf is not")):
        for call in (lambda: ix.class_probs(q, none, m=m, scale=scale), lambda: ix.class_probs_ids([0], none, m=m, scale=scale),
                     lambda: ix.class_probs_device(0, 1, 0, 1, 0, 0, 0, m=m, scale=scale)):
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="n_classes <= 65536, not 65537"):
        ix.class_probs_device(0, 1, 0, 65537, 0, 0, 0)
    with pytest.raises(ValueError, match="one entry per row"):
        ix.class_probs(q, [0, 1])
    with pytest.raises(ValueError, match="queries must be"):
        ix.class_probs(np.zeros((3, 7), dtype=np.float32), none)
    with pytest.raises(RuntimeError, match="closed"):                     # the checks passed: only the handle is missing
        ix.class_probs(q, none, full=True)
