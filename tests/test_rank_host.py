"""The host arithmetic of the rank and count queries (clip_cpp_amd/csrc/rank_host.h: argument checks, blocks, CSR expansion) under the
address and undefined-behaviour sanitizers: tests/rank_host_check.cpp is a stand-alone program with its own main, built and run on the
CPU.  Nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_host_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rank_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "clip_cpp_amd", "csrc"), os.path.join(ROOT, "tests", "rank_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "rank_host_check ok" in r.stdout, r.stderr
