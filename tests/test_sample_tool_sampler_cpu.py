"""tools/sample.py --sampler fused --min-p on the CPU: a tiny random-init config, run in a child process."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sample.py"), "--model-name", "qwen3-tiny",
                           "--num-layers", "2", "--prompt-ids", "1,2,3;4,5", "--max-new-tokens", "5", "--device", "cpu",
                           *args], capture_output=True, text=True, timeout=300, env=env)


def test_sample_tool_fused_sampler_with_min_p():
    r = _run("--temperature", "0.8", "--top-k", "50", "--sampler", "fused", "--min-p", "0.05")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    ids = re.findall(r"^ids\[(\d)\]: ([\d,]+)$", r.stdout, re.M)
    assert [i for i, _ in ids] == ["0", "1"] and all(len(s.split(",")) == 5 for _, s in ids), r.stdout
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["sampler"] == "fused" and summary["new_tokens"] == 10 and summary["tokens_per_s"] > 0


def test_sample_tool_min_p_needs_the_fused_sampler():
    r = _run("--temperature", "0.8", "--min-p", "0.05")
    assert r.returncode != 0 and 'sampler="fused"' in r.stderr
