"""ops.skinny_linear_fp8 on the gfx950 kernel (csrc/kernels/skinny_gemm.hip): every e4m3 code bit for bit,
the f64 bound at every edge of the tiling, the SwiGLU epilogue against swiglu_fwd bit for bit, row invariance,
unread memory, refusals and the composed path; ops.quantize_fp8_rows on the device against the CPU."""
import pytest
import torch

import _skinny_fp8_cases as fc

pytestmark = pytest.mark.gpu


def test_every_code_bitwise(cuda):
    fc.check_every_code(cuda)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(cuda, shape, bias):
    fc.check_accuracy(*shape, cuda, bias, pow2=fc.POW2[shape])


def test_accuracy_strided_rows(cuda):
    fc.check_accuracy(8, 1024, 1040, cuda, True, strided=True)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", fc.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(cuda, shape, bias):
    fc.check_swiglu(*shape, cuda, bias)


@pytest.mark.parametrize("K", fc.INVARIANCE_K)
def test_row_invariance(cuda, K):
    fc.check_row_invariance(K, cuda)


def test_unread_rows_stay_unread(cuda):
    fc.check_unread(cuda)


def test_refusals(cuda):
    fc.check_refusals(cuda)


def test_composed_path_within_the_bound(cuda, monkeypatch):
    fc.check_composed(cuda, monkeypatch)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
def test_quantiser(cuda, pow2, dtype):
    fc.check_quantiser(cuda, pow2, dtype)


def test_quantiser_equals_the_cpu_bitwise(cuda):
    fc.check_quantiser_devices_agree(cuda)
