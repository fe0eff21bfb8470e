"""The launch rules of the norm kernels (csrc/kernels/norm_plan.h: registers per lane, the backward
row splits, the column-sum tile) are plain C++ with no HIP, so they are pinned here on a CPU:
tests/native/norm_plan_check.cpp holds the cases with literal expectations."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_norm_launch_plan(tmp_path):
    exe = tmp_path / "norm_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tests", "native", "norm_plan_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK" in r.stdout and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
