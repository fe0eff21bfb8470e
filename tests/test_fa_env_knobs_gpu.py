"""The two flash-attention launch paths only the environment selects: DTG_FA_OCC=2 (dQ at two waves
per SIMD at head_dim 128) and DTG_FA_KV_PF=2 (dK/dV with two items staged ahead, 32-row items).
The knobs are read once when the extension loads and `flash_attn_tuning` cannot set them, so one
fresh child process (this file run as a script) loads the extension with both set and checks the
forward and backward against the CPU reference operators, with the comparison and tolerances of
test_kernels_gpu.test_flash_attn_d128_gqa."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQLENS = [64, 1, 129, 130]  # a one-token sequence, a block edge and a ragged tail
OK_LINE = "fa env knobs ok: 4 cases"


@pytest.mark.gpu
def test_flash_attn_env_selected_kernels(cuda):
    env = dict(os.environ, DTG_FA_OCC="2", DTG_FA_KV_PF="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and OK_LINE in r.stdout.splitlines(), (r.stdout + r.stderr)[-3000:]


def _child():
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
    import torch

    from test_kernels_gpu import _attn_case

    assert os.environ.get("DTG_FA_OCC") == "2" and os.environ.get("DTG_FA_KV_PF") == "2"
    cuda = torch.device("cuda:0")
    n = 0
    for causal in (True, False):
        _attn_case(cuda, SEQLENS, hq=4, hkv=2, D=128, causal=causal)
        _attn_case(cuda, SEQLENS, hq=4, hkv=4, D=64, causal=causal)
        n += 2
    torch.cuda.synchronize()
    print(f"fa env knobs ok: {n} cases")


if __name__ == "__main__":
    _child()
