"""The weight-only FP8 decode mode (linear="skinny-fp8") on the GPU: ops.skinny_linear_fp8 in the decode step
against the dequantised twin, and the HIP-graph decode loop against the eager loop bit for bit."""
import pytest

import _fp8_decode_cases as qc
import _generate_cases as gc

pytestmark = pytest.mark.gpu
KINDS = list(gc.MODELS)


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_fp8(cuda, kind):
    qc.check_teacher_forced(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_fp8_equals_the_twins_recompute(cuda, kind):
    qc.check_greedy(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_captured_loop_equals_eager_bitwise(cuda, kind):
    qc.check_graph_bitwise(kind, cuda)


def test_model_is_untouched_and_weights_are_reused(cuda, monkeypatch):
    qc.check_model_untouched("qwen2", cuda, monkeypatch)


def test_argument_errors(cuda):
    qc.check_argument_errors(cuda)
