"""The launch plan of decode_attn_multi (csrc/kernels/decode_attn_plan.h: q_tile and plan_multi) is plain
C++ with no HIP, so it is pinned here on a CPU: tests/native/decode_multi_plan_check.cpp holds the query tiles
and the table of calls with literal expectations."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_decode_multi_launch_plan(tmp_path):
    exe = tmp_path / "decode_multi_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tests", "native", "decode_multi_plan_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK" in r.stdout and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
