"""tools/sample.py end to end on the CPU: a tiny random-init config, prompts given as ids, run in a
child process as a user would."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sample.py"), *args], capture_output=True, text=True,
                          timeout=300, env=env)


def test_sample_tool_prints_the_requested_ids():
    r = _run("--model-name", "qwen3-tiny", "--num-layers", "2", "--prompt-ids", "1,2,3;4,5", "--max-new-tokens", "5",
             "--device", "cpu")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    ids = re.findall(r"^ids\[(\d)\]: ([\d,]+)$", r.stdout, re.M)
    assert [i for i, _ in ids] == ["0", "1"], r.stdout
    assert all(len(s.split(",")) == 5 for _, s in ids), r.stdout
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["sequences"] == 2 and summary["new_tokens"] == 10 and summary["tokens_per_s"] > 0


def test_sample_tool_rejects_bad_arguments():
    r = _run("--model-name", "llama-tiny", "--prompt", "hello", "--device", "cpu")
    assert r.returncode != 0 and "--tokenizer" in r.stderr
    r = _run("--model-name", "llama-tiny", "--prompt-ids", "1,2", "--tokenizer", "/nonexistent/dir", "--device", "cpu")
    assert r.returncode != 0 and "not a local directory" in r.stderr
