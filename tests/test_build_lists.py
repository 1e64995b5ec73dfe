"""The two build descriptions (Makefile for C / C++ consumers, clip_cpp_amd/build.py for the package) compile the same files with the
same per-file flags: a source added to one list only leaves the other's libclip.so with undefined symbols."""
import os
import re

from clip_cpp_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile():
    return open(os.path.join(ROOT, "Makefile")).read()


def make_list(text, name):
    m = re.search(r"^%s\s*:=(.*)$" % name, text, re.M)
    assert m, "Makefile has no %s := line" % name
    return m.group(1).split()


def stems(files, suffix):
    assert all(f.endswith(suffix) for f in files), files
    return [f[:-len(suffix)] for f in files]


def test_host_sources_match():
    assert make_list(makefile(), "HOST") == stems(B.HOST_SOURCES, ".cpp")


def test_kernel_sources_match():
    assert make_list(makefile(), "KERNELS") == stems(B.HIP_SOURCES, ".hip")


def test_weight_types_match():
    assert [int(w) for w in make_list(makefile(), "WTS")] == B.GEMM_WTYPES


def test_per_file_flags_match():
    m = re.search(r"^(.*):\s*CXXFLAGS\s*\+=\s*-fno-slp-vectorize\s*$", makefile(), re.M)
    assert m, "Makefile gives no file -fno-slp-vectorize"
    objs = m.group(1).split()
    assert all(o.startswith("$(OUT)/") and o.endswith(".o") for o in objs), objs
    assert sorted(o[len("$(OUT)/"):-len(".o")] for o in objs) == sorted(B.EXTRA_FLAGS)
    assert all(flags == ["-fno-slp-vectorize"] for flags in B.EXTRA_FLAGS.values())
