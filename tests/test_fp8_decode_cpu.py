"""The weight-only FP8 decode mode (linear="skinny-fp8") on the CPU operators: the dequantised-twin oracle,
the untouched model, argument errors and tools/sample.py."""
import json
import os
import re
import subprocess
import sys

import pytest

import _fp8_decode_cases as qc
import _generate_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = list(gc.MODELS)


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_fp8(kind):
    qc.check_teacher_forced(kind, "cpu")


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_fp8_equals_the_twins_recompute(kind):
    qc.check_greedy(kind, "cpu")


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_model_is_untouched_and_weights_are_reused(kind, monkeypatch):
    qc.check_model_untouched(kind, "cpu", monkeypatch)


def test_argument_errors():
    qc.check_argument_errors("cpu")


def test_sample_tool_takes_skinny_fp8():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--model-name", "qwen3-tiny",
                        "--num-layers", "2", "--prompt-ids", "1,2,3;4,5", "--max-new-tokens", "5", "--device", "cpu",
                        "--linear", "skinny-fp8"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    ids = re.findall(r"^ids\[(\d)\]: ([\d,]+)$", r.stdout, re.M)
    assert [i for i, _ in ids] == ["0", "1"] and all(len(s.split(",")) == 5 for _, s in ids), r.stdout
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["linear"] == "skinny-fp8" and summary["new_tokens"] == 10
