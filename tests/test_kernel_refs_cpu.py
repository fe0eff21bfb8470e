"""The cases of test_kernel_numerics_gpu.py run through the package's f32 CPU ops, against the same
float64 references with the same bounds (tests/_refs.py, tests/_kernel_cases.py).

This shows without a GPU that the references are right, that every f32 term can be met by a correct
f32 implementation, and that the chained-rounding outlier caps hold on these inputs.  No bound is
looser here than on the GPU.
"""
import pytest
import torch

import _kernel_cases as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("H", C.RMS_HIDDEN)
def test_rmsnorm_hidden_sizes(H):
    C.check_rmsnorm_hidden(CPU, H)
    C.check_rmsnorm_bwd_hidden(CPU, H)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("T", C.RMS_BWD_T)
def test_rmsnorm_bwd_rows(T, with_dres):
    C.check_rmsnorm_bwd_rows(CPU, T, with_dres)


def test_rmsnorm_strided_rows():
    C.check_rmsnorm_strided(CPU)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_rmsnorm_eps(eps):
    C.check_rmsnorm_eps(CPU, eps)


@pytest.mark.parametrize("nh", [1, 6])
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("D", [64, 128])
def test_rope(D, T, nh):
    C.check_rope(CPU, D, T, nh)


@pytest.mark.parametrize("T,I", [(1, 8), (77, 136)])
def test_swiglu(T, I):
    C.check_swiglu(CPU, T, I)


@pytest.mark.parametrize("T,I", [(8, 8), (72, 136), (136, 264)])
def test_swiglu_bwd_t(T, I):
    C.check_swiglu_bwd_t(CPU, T, I)


def test_swiglu_bwd_t_refuses_bad_layouts():
    C.check_swiglu_bwd_t_refusals(CPU)


@pytest.mark.parametrize("V", C.CE_VOCABS)
def test_cross_entropy(V):
    C.check_ce(CPU, V)


def test_cross_entropy_vocab_parallel():
    C.check_ce_vocab_parallel(CPU)


@pytest.mark.parametrize("layout", list(C.ADAM_LAYOUTS))
@pytest.mark.parametrize("gdt,sdt,master", C.ADAM_COMBOS, ids=C.ADAM_IDS)
def test_adamw(gdt, sdt, master, layout):
    C.check_adamw_combo(CPU, gdt, sdt, master, layout)


@pytest.mark.parametrize("case", C.ADAM_EDGE_CASES, ids=["wd0", "step100000", "grad_scale0"])
@pytest.mark.parametrize("sdt,master", [(torch.bfloat16, False), (torch.float32, True)], ids=["bf16", "f32_master"])
def test_adamw_edge_values(sdt, master, case):
    C.check_adamw_edges(CPU, sdt, master, **case)


def test_adamw_unrolled_loop_size():
    C.check_adamw_big(CPU)


def test_empty_inputs():
    C.check_rmsnorm_empty(CPU)
    C.check_rope_empty(CPU)
    C.check_swiglu_empty(CPU)
    C.check_ce_empty(CPU)
