"""The owning buffer type and the corpus column commit (csrc/dev_buf.h) on the host, under sanitizers.

tests/fuzz/dev_buf_check.cpp instantiates dev_buf.h over a counting heap space and checks the
growth policy (max(need, cap * 3 / 2) for the device-like space, exactly `need` for the pinned-like
one), free-before-allocate, the failure path, single ownership through moves and swaps, the
destruction of a struct of twenty buffers, and regrow_columns with every one of eight allocations
refused in turn.  It is compiled with -fsanitize=address,undefined -fno-sanitize-recover=all as a
stand-alone program and run with leak detection on: a leak, a double free, a use after free or UB
fails the run.  CPU only.
"""
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_dev_buf_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "dev_buf_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "fuzz" / "dev_buf_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1:abort_on_error=0",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "dev_buf_check: ok"
