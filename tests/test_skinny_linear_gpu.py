"""ops.skinny_linear on the gfx950 kernel (csrc/kernels/skinny_gemm.hip): the f64 bound at every edge of the
tiling, the SwiGLU epilogue against swiglu_fwd bit for bit, row invariance, unread memory, refusals and
the composed hipBLASLt path."""
import pytest

import _skinny_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(cuda, shape, bias):
    sc.check_accuracy(*shape, cuda, bias)


def test_accuracy_strided_rows(cuda):
    sc.check_accuracy(8, 1024, 520, cuda, True, strided=True)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", sc.SWIGLU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(cuda, shape, bias):
    sc.check_swiglu(*shape, cuda, bias)


@pytest.mark.parametrize("K", sc.INVARIANCE_K)
def test_row_invariance(cuda, K):
    sc.check_row_invariance(K, cuda)


def test_unread_rows_stay_unread(cuda):
    sc.check_unread(cuda)


def test_refusals(cuda):
    sc.check_refusals(cuda)


def test_composed_path_within_the_bound(cuda, monkeypatch):
    sc.check_composed(cuda, monkeypatch)
