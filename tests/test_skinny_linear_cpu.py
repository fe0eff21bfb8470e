"""ops.skinny_linear on the CPU operator: the f64 bound, the SwiGLU epilogue, row invariance, refusals."""
import pytest

import _skinny_cases as sc


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape, bias):
    sc.check_accuracy(*shape, "cpu", bias)


def test_accuracy_strided_rows():
    sc.check_accuracy(8, 1024, 520, "cpu", True, strided=True)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", sc.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(shape, bias):
    sc.check_swiglu(*shape, "cpu", bias)


@pytest.mark.parametrize("K", sc.INVARIANCE_K)
def test_row_invariance(K):
    sc.check_row_invariance(K, "cpu")


def test_unread_rows_stay_unread():
    sc.check_unread("cpu")


def test_refusals():
    sc.check_refusals("cpu")
