"""The joint-row arithmetic of the int8 tail copy on the host (csrc/knn_plan.h i8t_joint_row_bytes,
i8t_tail_stages, i8t_row_stages; DESIGN.md "int8 tail").

A row of the copy is its dpt tail codes, then its first H columns as bf16: dpt + 2 H bytes, whole
128-byte stages, the tail's first.  tests/fuzz/i8joint_check.cpp prints the three functions over a
grid of valid and invalid (H, dpt) pairs; it is compiled with knn_plan.cpp by plain g++ (the unit is
HIP-free) under -fsanitize=address,undefined as a stand-alone program, and every line is compared
with the layout as stated here.  CPU only.
"""
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def _expect(head, dpt):
    ok = head >= 0 and head % 64 == 0 and dpt >= 128 and dpt % 128 == 0
    row = dpt + 2 * head if ok else -1
    return row, dpt // 128, row // 128 if ok else -1


def test_joint_row_arithmetic_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "i8joint_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "fuzz" / "i8joint_check.cpp"),
           str(ROOT / "image_recommender_amd" / "csrc" / "knn_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1:abort_on_error=0",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    table = {}
    for line in r.stdout.splitlines():
        head, dpt, row, nst_t, nst = (int(v) for v in line.split())
        table[head, dpt] = (row, nst_t, nst)
        assert (row, nst_t, nst) == _expect(head, dpt), line
        if row > 0:
            assert row % 128 == 0 and nst == nst_t + head // 64 and nst * 128 == row, line
    assert len(table) == 69 * 67
    # the shapes the design and the GPU tests name: bench config 3 (dpb 1984, H = 192), the two of
    # tests/test_i8joint_gpu.py, and H = 0 (the row is the codes alone)
    assert table[192, 1792] == (2176, 14, 17)
    assert table[192, 640] == (1024, 5, 8)
    assert table[128, 640] == (896, 5, 7)
    assert table[0, 768] == (768, 6, 6)
    assert table[64, 64][0] == -1 and table[32, 640][0] == -1 and table[-64, 640][0] == -1
