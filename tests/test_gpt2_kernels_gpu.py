"""The GPT-2 streaming kernels (layernorm.hip, gelu.hip) against float64 references at ulp-level
bounds, on the code paths, strides, edge values and empty inputs of tests/_gpt2_cases.py; the same
cases run through the CPU ops in test_gpt2_kernels_cpu.py.

Each assert_within prints the largest error it saw before it asserts; run with -s or -rA to see them.
"""
import pytest
import torch

import _gpt2_cases as C

pytestmark = pytest.mark.gpu
dops = torch.ops.dtg
BF = torch.bfloat16


@pytest.mark.parametrize("H", C.LN_HIDDEN)
def test_layernorm_hidden_sizes(cuda, H):
    C.check_layernorm_hidden(cuda, H)


def test_layernorm_unsupported_hidden_size(cuda):
    x = torch.zeros(5, 16392, dtype=BF, device=cuda)
    w = torch.ones(16392, dtype=BF, device=cuda)
    st = torch.ones(5, device=cuda)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.layernorm_fwd(x, w, w, 1e-5)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.dropout_add_layernorm_fwd(x, x, w, w, 1e-5, 0.0, None)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.layernorm_bwd(x, x, w, st, st, None, 0.0, None)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("T", C.LN_BWD_T)
def test_layernorm_bwd_rows(cuda, T, with_dres):
    C.check_layernorm_bwd_rows(cuda, T, with_dres)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("H", C.LN_BWD_HIDDEN)
def test_layernorm_bwd_hidden_sizes(cuda, H, with_dres):
    C.check_layernorm_bwd_hidden(cuda, H, with_dres)


def test_layernorm_strided_rows(cuda):
    C.check_layernorm_strided(cuda)


def test_layernorm_empty_and_bad_layouts(cuda):
    C.check_layernorm_empty(cuda)
    C.check_layernorm_bad_layouts(cuda, pytest.raises)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_add_layernorm(cuda, p):
    C.check_dropout(cuda, p)


@pytest.mark.parametrize("T,I", [(1, 8), (77, 136)])
def test_gelu(cuda, T, I):
    C.check_gelu(cuda, T, I)


@pytest.mark.parametrize("T,I", [(8, 8), (72, 136), (136, 264)])
def test_gelu_bwd_t(cuda, T, I):
    C.check_gelu_bwd_t(cuda, T, I)


def test_gelu_empty(cuda):
    C.check_gelu_empty(cuda)
