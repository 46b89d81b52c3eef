"""The route decision of a query chunk (csrc/knn_plan.h choose_route) on the host, under sanitizers.

tests/fuzz/route_check.cpp evaluates choose_route over a grid that crosses every threshold of the
decision (21 widths x 9 corpus sizes x 15 batch sizes x 8 k x the five search modes x 3 CU counts x
the int8 workgroups-per-CU knob x the int8 tail's knob and the copy's three states: 4.1 M rows) and
compares the route, tail_ok, i8_inst and every Plan field with tests/golden/route_table.bin, which
tools/route_table_gen.py recorded from the former use_* ladder — not from choose_route.  It is
compiled together with knn_plan.cpp by plain g++ (no ROCm include path: the unit is HIP-free) with
-fsanitize=address,undefined -fno-sanitize-recover=all as a stand-alone program.  Any difference
fails, without tolerance.  CPU only.
"""
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_route_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "route_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "fuzz" / "route_check.cpp"),
           str(ROOT / "image_recommender_amd" / "csrc" / "knn_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1:abort_on_error=0",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(exe), str(ROOT / "tests" / "golden" / "route_table.bin")], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "route_check: ok (3780 slices, 2160 rows)"
