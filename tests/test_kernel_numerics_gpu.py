"""The streaming gfx950 kernels (rmsnorm.hip, rope.hip, swiglu.hip, xent.hip, adamw.hip) against
float64 references at ulp-level bounds: |out - ref| <= half a bf16 ulp + the propagated f32 error of
the formula (tests/_refs.py), on the code paths, strides, edge values and empty inputs that
test_kernels_gpu.py does not reach.  The cases live in tests/_kernel_cases.py and also run through
the f32 CPU ops in test_kernel_refs_cpu.py, which shows that the bounds can be met.

Each assert_within prints the largest error it saw (in bf16 ulps and as a share of its bound) before
it asserts; run with -s or -rA to see them.
"""
import pytest
import torch

import _kernel_cases as C

pytestmark = pytest.mark.gpu
dops = torch.ops.dtg
BF = torch.bfloat16


@pytest.mark.parametrize("H", C.RMS_HIDDEN)
def test_rmsnorm_hidden_sizes(cuda, H):
    C.check_rmsnorm_hidden(cuda, H)
    C.check_rmsnorm_bwd_hidden(cuda, H)


def test_rmsnorm_unsupported_hidden_size(cuda):
    x = torch.zeros(5, 16392, dtype=BF, device=cuda)
    w = torch.ones(16392, dtype=BF, device=cuda)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.rmsnorm_fwd(x, w, 1e-5)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.add_rmsnorm_fwd(x, x, w, 1e-5)
    with pytest.raises(RuntimeError, match="unsupported hidden size"):
        dops.rmsnorm_bwd(x, x, w, torch.ones(5, device=cuda), None)


def test_rmsnorm_bwd_refuses_bad_dres_and_rstd(cuda):
    """A dres that is not [T, H] and an rstd the device cannot read are refused on the host (they
    used to go straight into the kernel)."""
    T, H = 5, 64
    x = torch.zeros(T, H, dtype=BF, device=cuda)
    w = torch.ones(H, dtype=BF, device=cuda)
    rstd = torch.ones(T, device=cuda)
    with pytest.raises(RuntimeError, match="dres shape"):
        dops.rmsnorm_bwd(x, x, w, rstd, torch.zeros(T, H + 8, dtype=BF, device=cuda))
    with pytest.raises(RuntimeError, match="dres shape"):
        dops.rmsnorm_bwd(x, x, w, rstd, torch.zeros(T * H, dtype=BF, device=cuda))
    with pytest.raises(RuntimeError, match="rmsnorm_bwd: rstd"):
        dops.rmsnorm_bwd(x, x, w, torch.ones(T), None)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("T", C.RMS_BWD_T)
def test_rmsnorm_bwd_rows(cuda, T, with_dres):
    C.check_rmsnorm_bwd_rows(cuda, T, with_dres)


def test_rmsnorm_strided_rows(cuda):
    C.check_rmsnorm_strided(cuda)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_rmsnorm_eps(cuda, eps):
    C.check_rmsnorm_eps(cuda, eps)


@pytest.mark.parametrize("nh", [1, 6])
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("D", [64, 128])
def test_rope(cuda, D, T, nh):
    C.check_rope(cuda, D, T, nh)


@pytest.mark.parametrize("T,I", [(1, 8), (77, 136)])
def test_swiglu(cuda, T, I):
    C.check_swiglu(cuda, T, I)


@pytest.mark.parametrize("T,I", [(8, 8), (72, 136), (136, 264)])
def test_swiglu_bwd_t(cuda, T, I):
    C.check_swiglu_bwd_t(cuda, T, I)


def test_swiglu_refuses_bad_layouts(cuda):
    """I % 8 != 0 and a non-unit inner stride: refused by the forward and the backward alike (the
    backward used to launch I / 8 vectors per row and leave the rest of dgu unwritten).  The tiled
    backward refuses a gu whose width is no multiple of 16 and a dh that is not 2-D (it used to
    take both and truncate)."""
    C.check_swiglu_bwd_t_refusals(cuda)
    odd = torch.zeros(4, 24, dtype=BF, device=cuda)            # I = 12
    cols = torch.zeros(32, 4, dtype=BF, device=cuda).t()       # [4, 32] with stride(1) == 4
    assert cols.shape == (4, 32) and cols.stride(1) != 1
    for gu in (odd, cols):
        dh = torch.zeros(4, gu.size(1) // 2, dtype=BF, device=cuda)
        with pytest.raises(RuntimeError, match="swiglu"):
            dops.swiglu_fwd(gu)
        with pytest.raises(RuntimeError, match="swiglu_bwd"):
            dops.swiglu_bwd(dh, gu)


@pytest.mark.parametrize("V", C.CE_VOCABS)
def test_cross_entropy(cuda, V):
    C.check_ce(cuda, V)


def test_cross_entropy_vocab_parallel(cuda):
    C.check_ce_vocab_parallel(cuda)


@pytest.mark.parametrize("layout", list(C.ADAM_LAYOUTS))
@pytest.mark.parametrize("gdt,sdt,master", C.ADAM_COMBOS, ids=C.ADAM_IDS)
def test_adamw(cuda, gdt, sdt, master, layout):
    C.check_adamw_combo(cuda, gdt, sdt, master, layout)


@pytest.mark.parametrize("case", C.ADAM_EDGE_CASES, ids=["wd0", "step100000", "grad_scale0"])
@pytest.mark.parametrize("sdt,master", [(torch.bfloat16, False), (torch.float32, True)], ids=["bf16", "f32_master"])
def test_adamw_edge_values(cuda, sdt, master, case):
    C.check_adamw_edges(cuda, sdt, master, **case)


def test_adamw_unrolled_loop_size(cuda):
    """n = 2 * 8388608 + 3 * 2048 + 8: the only size at which the unrolled main loop, the remainder
    loop and lanes with no work all occur (about 135 MB on the device)."""
    C.check_adamw_big(cuda)


def test_empty_inputs(cuda):
    C.check_rmsnorm_empty(cuda)
    C.check_rope_empty(cuda)
    C.check_swiglu_empty(cuda)
    C.check_ce_empty(cuda)
