"""CPU tier of the int8 storage mode of the exact index: the host-only context refuses it in create (not in the Python dtype check), the
image-search CLI accepts `--dtype i8` and lists it, and read_index_header reads an i8 (dtype 3) header."""
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_only_env():
    return dict(os.environ, CLIP_AMD_ALLOW_NO_DEVICE="1", HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          env=_host_only_env(), cwd=ROOT, timeout=300)


def test_i8_index_on_host_only_context_fails_in_create(clip_lib, fixture_cache):
    from oracle import fixtures
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    code = ("import clip_cpp_amd as c\n"
            "m = c.Clip(%r, verbosity=0)\n"
            "assert c.lib().clip_amd_ctx_device(m.ctx) == -1\n"
            "assert c.Index.DTYPES['i8'] == 3\n"
            "try:\n"
            "    c.Index(m, 32, 'i8')\n"
            "except RuntimeError as e:\n"
            "    print('raised', e)\n") % model
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_host_only_env(), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "raised clip_amd_index_create failed" in r.stdout
    assert "clip_amd_index_create: host-only context" in r.stderr


def test_build_accepts_i8_and_still_rejects_bf16(tmp_path, fixture_cache):
    from oracle import fixtures
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    (tmp_path / "pics").mkdir()
    r = _cli("build", "-m", model, "--dtype", "i8", "--db", tmp_path / "db", tmp_path / "pics")
    # past argument parsing: the model loads on a host-only context and the index create refuses it
    assert "Usage:" not in r.stdout, r.stdout[-2000:]
    assert "clip_amd_index_create: host-only context" in r.stderr, r.stderr[-2000:]
    r = _cli("build", "-m", model, "--dtype", "bf16", "--db", tmp_path / "db", tmp_path / "pics")
    assert r.returncode != 0 and "Usage:" in r.stdout and "dir/with/pictures" in r.stdout


def test_build_help_lists_i8():
    r = _cli("build", "-h")
    assert r.returncode == 0 and "--dtype f16|f32|i8" in r.stdout


def test_read_index_header_of_an_i8_file(tmp_path):
    from clip_cpp_amd import image_search
    p = tmp_path / "images.index"
    p.write_bytes(b"CLIPIDX1" + struct.pack("<IIIQ", 1, 512, 3, 2) + bytes(2 * 512))
    assert image_search.read_index_header(str(p)) == (1, 512, 3, 2)
