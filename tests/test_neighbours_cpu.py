"""CPU tier of the searches by stored row and the k-NN graph: the new entry points on NULL arguments, the option parsing and help texts of
`search --like` and `neighbors`, and the database check of `--like` that runs before any model is loaded."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    # no visible device at all, even on a GPU machine (the environment of tests/test_search_cpu.py)
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def test_new_entry_points_reject_null_arguments(clip_lib):
    L = clip_lib.lib()
    assert L.clip_amd_index_search_ids(None, None, 1, 5, 1, None, None, None) is False
    assert L.clip_amd_index_search_ids_device(None, None, 1, 5, 1, None, None, None) is False
    assert L.clip_amd_index_knn_graph(None, 5, None, None) is False
    assert L.clip_amd_test_index_knn_route(None, 2) == -1
    env = _host_only_env()
    code = "import clip_cpp_amd as c; print('us', c.bench_knn('f16', 1024, 64, 5, 2, 1))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("us")[1]) < 0


def _parse(argv, **kw):
    from clip_cpp_amd import image_search
    return image_search._parse(list(argv), kw.pop("build", False), **kw)


def test_like_parsing(capsys):
    p = _parse(["--like", "pics/a.png"])
    assert p is not None and p["like"] == "pics/a.png" and p["rest"] == [] and p["results"] == 5
    p = _parse(["--like", "pics/a.png", "--in", "pics/", "--in", "more/", "-n", "3"])
    assert p["like"] == "pics/a.png" and p["in"] == ["pics/", "more/"] and p["results"] == 3
    assert _parse(["--like", "pics/a.png", "a", "cat"]) is None          # with a positional query
    assert _parse(["a", "cat", "--like", "pics/a.png"])["like"] is None   # (after the query everything is the query, as before)
    assert _parse(["--like", "pics/a.png", "-d", "0.2"]) is None
    assert _parse(["-d", "0.2", "--like", "pics/a.png"]) is None
    assert _parse(["--like"]) is None                                     # without a value
    assert _parse(["--like", "a.png", "--like", "b.png"]) is None         # twice
    for mode in ({"build": True}, {"update": True}, {"dedup": True}):
        assert _parse(["--like", "a.png", "dir"], **mode) is None
    assert "unrecognized argument: --like" in capsys.readouterr().out
    p = _parse(["a", "cat"])                                              # a plain search is what it was
    assert p["rest"] == ["a", "cat"] and p["like"] is None


def test_neighbors_parsing(capsys):
    p = _parse([], neighbors=True)
    assert p is not None and p["results"] == 5 and p["rest"] == []
    p = _parse(["-n", "7", "--db", "d", "-v", "0", "-m", "m.gguf"], neighbors=True)
    assert p["results"] == 7 and p["db"] == "d" and p["verbose"] == 0 and p["model"] == "m.gguf"
    assert _parse(["pics"], neighbors=True) is None
    assert "unexpected argument: pics" in capsys.readouterr().out
    for bad in (["--in", "pics/"], ["-d", "0.1"], ["--dtype", "i8"], ["--like", "a.png"], ["-n"]):
        assert _parse(bad, neighbors=True) is None, bad


def test_help_and_usage_texts(capsys):
    from clip_cpp_amd import image_search
    image_search._help(False, dict(threads=4, verbose=1, db=".", results=5))
    out = capsys.readouterr().out
    assert "--like <path>" in out and "--in <prefix>" in out and "-n N, --results N: Number of results to display. Default: 5" in out
    image_search._help(False, dict(verbose=1, db=".", results=5), neighbors=True)
    out = capsys.readouterr().out
    assert "image_search neighbors [options]" in out and "-n N, --results N" in out and "--in" not in out
    assert image_search.main([]) == 1
    out = capsys.readouterr().out
    assert "neighbors" in out and "update" in out and "{build|search|dedup}" in out
    assert "--like" in image_search.__doc__ and "neighbors" in image_search.__doc__ and "--in PREFIX" in image_search.__doc__


def _database(tmp_path, paths):
    (tmp_path / "images.paths").write_text("".join(p + "\n" for p in ["no/such/model.gguf"] + paths))
    with open(tmp_path / "images.index", "wb") as f:                      # header only: nothing reads the rows before the check
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 4, 1, len(paths)))


@pytest.mark.parametrize("paths", [[], ["img/a.png", "img/b.png"]])
def test_like_of_a_path_that_is_not_indexed_fails_before_the_model(tmp_path, paths):
    _database(tmp_path, paths)
    cmd = [sys.executable, "-m", "clip_cpp_amd.image_search", "search", "--db", str(tmp_path), "--like", "missing.png"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "main: 'missing.png' is not in the database (paths are compared as written in images.paths)" in r.stderr
    assert "Unable to load model" not in r.stdout                         # the model (which does not exist) was never asked for


def test_like_usage_errors_print_the_usage(tmp_path):
    _database(tmp_path, ["img/a.png"])
    for extra in (["--like", "img/a.png", "a", "cat"], ["--like", "img/a.png", "-d", "0.1"], ["--like"], ["--like", "img/a.png", "--like", "img/a.png"]):
        cmd = [sys.executable, "-m", "clip_cpp_amd.image_search", "search", "--db", str(tmp_path)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, env=_host_only_env(), timeout=300, cwd=ROOT)
        assert r.returncode == 1 and "Usage: python -m clip_cpp_amd.image_search search" in r.stdout, extra
