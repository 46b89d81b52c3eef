"""The stream fence and the operation scope (csrc/stream_fence.h) on the host, under sanitizers.

tests/fuzz/stream_fence_check.cpp instantiates stream_fence.h over a stream API that logs every call
and can be told to fail the n-th one.  It checks the call logs of the eager and lazy fence against
literals written down from the code the scope replaced (A, A, B; A, host, B; lazy A, A, A, B; a lazy
record that fails; a host form followed by any stream), the same for the workspaces' hand-off with
its event made on first use, the error exits (the device form leaves the fence on its stream, the
host form synchronises and clears it, the caller's error code and text stay the original ones even
when the clean-up itself fails), a scope that never began (no call at all), and after every
operation the lock released and the device restored.  It is compiled with
-fsanitize=address,undefined -fno-sanitize-recover=all as a stand-alone program and run with leak
detection on.  CPU only.
"""
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_stream_fence_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "stream_fence_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "fuzz" / "stream_fence_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1:abort_on_error=0",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "stream_fence_check: ok"
