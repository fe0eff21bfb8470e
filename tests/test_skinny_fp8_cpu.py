"""ops.skinny_linear_fp8 on the CPU operator and ops.quantize_fp8_rows on the CPU: every e4m3 code, the f64
bound, the SwiGLU epilogue, row invariance, refusals, and the quantiser's rules."""
import pytest
import torch

import _skinny_fp8_cases as fc


def test_every_code_bitwise():
    fc.check_every_code("cpu")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape, bias):
    fc.check_accuracy(*shape, "cpu", bias, pow2=fc.POW2[shape])


def test_accuracy_strided_rows():
    fc.check_accuracy(8, 1024, 1040, "cpu", True, strided=True)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", fc.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(shape, bias):
    fc.check_swiglu(*shape, "cpu", bias)


@pytest.mark.parametrize("K", fc.INVARIANCE_K)
def test_row_invariance(K):
    fc.check_row_invariance(K, "cpu")


def test_unread_rows_stay_unread():
    fc.check_unread("cpu")


def test_refusals():
    fc.check_refusals("cpu")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
def test_quantiser(pow2, dtype):
    fc.check_quantiser("cpu", pow2, dtype)


def test_quantiser_refusals():
    fc.check_quantiser_refusals()
