"""CPU tier of the search of one index with the rows of another and of append: the new entry points on NULL arguments, the option parsing
and help texts of `label` and `merge`, `merge`'s refusals (model line, dim, dtype) that run before any model is loaded, and the parse
results of the five older commands, which must be what they were."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def test_new_entry_points_reject_null_arguments(clip_lib, capfd):
    L = clip_lib.lib()
    assert L.clip_amd_index_search_index(None, None, None, 0, 5, None, None, None) is False
    assert L.clip_amd_index_append(None, None, None) == -1
    assert capfd.readouterr().err.count("is NULL") == 2
    assert L.clip_amd_test_index_cross_route(None, 2) == -1
    code = "import clip_cpp_amd as c; print('us', c.bench_cross('f16', 1024, 256, 64, 5, 2, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def _parse(argv, **kw):
    from clip_cpp_amd import image_search
    return image_search._parse(list(argv), kw.pop("build", False), **kw)


def test_label_parsing(capsys):
    p = _parse(["a cat", "a dog"], label=True)
    assert p is not None and p["rest"] == ["a cat", "a dog"] and p["results"] == 1 and p["db"] == "." and p["threads"] == 4
    p = _parse(["-n", "3", "--db", "d", "-v", "0", "-m", "m.gguf", "-t", "2", "cat", "-n", "2", "dog"], label=True)
    assert p["results"] == 2 and p["db"] == "d" and p["verbose"] == 0 and p["model"] == "m.gguf" and p["threads"] == 2
    assert p["rest"] == ["cat", "dog"]                                   # options and labels may alternate, as build's directories
    assert _parse([], label=True) is None                                # no label
    assert _parse(["-n", "2"], label=True) is None
    for bad in (["--in", "pics/", "cat"], ["-d", "0.1", "cat"], ["--dtype", "i8", "cat"], ["--like", "a.png"], ["--from", "d", "cat"], ["cat", "-n"]):
        assert _parse(bad, label=True) is None, bad
    assert "unrecognized argument: --from" in capsys.readouterr().out


def test_merge_parsing(capsys):
    p = _parse(["--db", "a", "--from", "b"], merge=True)
    assert p is not None and p["db"] == "a" and p["from"] == ["b"] and p["max_distance"] is None and p["rest"] == [] and p["model"] == ""
    p = _parse(["--from", "b", "-d", "0.02", "--from", "c", "-m", "m.gguf", "-v", "0"], merge=True)
    assert p["from"] == ["b", "c"] and p["max_distance"] == 0.02 and p["model"] == "m.gguf" and p["verbose"] == 0 and p["db"] == "."
    assert _parse(["--max-distance", "0.5", "--from", "b"], merge=True)["max_distance"] == 0.5
    assert _parse(["--db", "a"], merge=True) is None                     # nothing to merge
    assert _parse(["--db", "a", "--from"], merge=True) is None
    assert _parse(["--from", "b", "-d", "nan"], merge=True) is None
    assert _parse(["--from", "b", "c"], merge=True) is None
    assert "unexpected argument: c" in capsys.readouterr().out
    for bad in (["-n", "3"], ["-t", "2"], ["--in", "pics/"], ["--dtype", "i8"], ["--like", "a.png"]):
        assert _parse(["--from", "b"] + bad, merge=True) is None, bad


def test_help_and_usage_texts(capsys):
    from clip_cpp_amd import image_search
    image_search._help(False, dict(threads=4, verbose=1, db=".", results=1), label=True)
    out = capsys.readouterr().out
    assert "image_search label [options] LABEL [LABEL ...]" in out and "-n N, --results N: Number of labels per image" in out
    assert "Default: 1" in out and "-t N, --threads N" in out and "--from" not in out and "--in" not in out
    image_search._help(False, dict(verbose=1, db="."), merge=True)
    out = capsys.readouterr().out
    assert "image_search merge [options] --db <dir> --from <dir2>" in out and "--from <dir>" in out and "-d R, --max-distance R" in out
    assert "--threads" not in out and "--results" not in out
    for cmd in ("label", "merge"):
        with pytest.raises(SystemExit) as e:
            image_search.main([cmd, "-h"])
        assert e.value.code == 0 and ("image_search %s [options]" % cmd) in capsys.readouterr().out
    assert image_search.main([]) == 1
    out = capsys.readouterr().out
    assert "label [options] LABEL" in out and "merge [options] --db DIR --from DIR2" in out and "{build|search|dedup}" in out
    assert image_search.main(["label"]) == 1 and "image_search label [options]" in capsys.readouterr().out
    assert image_search.main(["merge", "--db", "x"]) == 1 and "image_search merge [options]" in capsys.readouterr().out
    assert "label  [-m MODEL]" in image_search.__doc__ and "merge  [-m MODEL]" in image_search.__doc__


def test_the_five_older_commands_parse_as_before():
    base = dict(threads=4, verbose=1, db=".", dtype="f16", results=5, max_distance=None, model="", rest=[], like=None)
    base["in"] = []
    assert _parse(["pics", "more"], build=True) == dict(base, model="../models/ggml-model-f16.bin", rest=["pics", "more"])
    assert _parse(["--dtype", "i8", "-t", "2", "pics"], build=True) == dict(base, model="../models/ggml-model-f16.bin", rest=["pics"], dtype="i8",
                                                                            threads=2)
    assert _parse(["--db", "d", "pics"], update=True) == dict(base, db="d", rest=["pics"])
    assert _parse(["-n", "3", "--in", "a/", "a", "cat", "-n", "9"]) == dict(base, results=3, rest=["a", "cat", "-n", "9"], **{"in": ["a/"]})
    assert _parse(["-d", "0.25", "x.png"]) == dict(base, max_distance=0.25, rest=["x.png"])
    assert _parse(["--like", "a.png"]) == dict(base, like="a.png")
    assert _parse([], dedup=True) == dict(base, max_distance=0.05)
    assert _parse(["-v", "0", "-d", "0.1"], dedup=True) == dict(base, max_distance=0.1, verbose=0)
    assert _parse(["-n", "7", "-m", "m.gguf"], neighbors=True) == dict(base, results=7, model="m.gguf")
    for mode in ({"build": True}, {"update": True}, {"dedup": True}, {"neighbors": True}, {}):
        assert _parse(["--from", "d", "x"], **mode) is None, mode          # the new flag belongs to merge alone
    assert _parse(["-t", "2"], dedup=True) is None and _parse(["-n", "2"], dedup=True) is None and _parse(["-n", "2", "pics"], update=True) is None


def _database(d, model, dim, dtype, paths):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "images.paths"), "w") as f:
        f.write("".join(p + "\n" for p in [model] + paths))
    with open(os.path.join(d, "images.index"), "wb") as f:                # header only: nothing reads the rows before the checks
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, dim, dtype, len(paths)))


def _merge(*args):
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search", "merge"] + [str(a) for a in args]
    return subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)


def test_merge_refuses_before_any_model_is_loaded(tmp_path):
    """the model of every database here does not exist: a run that got as far as loading it says so on stdout"""
    t, same = tmp_path / "t", tmp_path / "same"
    _database(t, "no/such/model.gguf", 8, 1, ["img/a.png"])
    _database(same, "no/such/model.gguf", 8, 1, ["img/b.png"])
    cases = {
        "model": (("other/model.gguf", 8, 1), "was built with the model other/model.gguf, the target with no/such/model.gguf"),
        "dim": (("no/such/model.gguf", 12, 1), "holds 12-dimensional embeddings, the target 8-dimensional ones"),
        "dtype": (("no/such/model.gguf", 8, 3), "is stored as i8, the target as f16"),
    }
    for name, ((model, dim, dtype), message) in cases.items():
        d = tmp_path / name
        _database(d, model, dim, dtype, ["img/c.png"])
        for order in ((same, d), (d,)):                                    # every source is checked, not only the first
            r = _merge("--db", t, *[x for s in order for x in ("--from", s)])
            assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
            assert message in r.stderr and str(d) in r.stderr, r.stderr
            assert "Unable to load model" not in r.stdout
    # -m: the model lines are not compared (dim and dtype still are); this run gets as far as the model, which does not exist
    r = _merge("--db", t, "--from", tmp_path / "model", "-m", "no/such/model.gguf")
    assert r.returncode == 1 and "main: Unable to load model from no/such/model.gguf" in r.stdout and "was built with" not in r.stderr
    r = _merge("--db", t, "--from", tmp_path / "dim", "-m", "no/such/model.gguf")
    assert r.returncode == 1 and "12-dimensional" in r.stderr and "Unable to load model" not in r.stdout
    # a source that is no database, a target that is none
    r = _merge("--db", t, "--from", tmp_path / "nowhere")
    assert r.returncode == 1 and "no database in" in r.stderr and "Unable to load model" not in r.stdout
    r = _merge("--db", tmp_path / "nowhere", "--from", same)
    assert r.returncode == 1 and "no database in" in r.stderr
    assert (t / "images.paths").read_text() == "no/such/model.gguf\nimg/a.png\n"   # nothing was written
