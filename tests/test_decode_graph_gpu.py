"""The decode step through ops.skinny_linear and the HIP-graph decode loop on the GPU."""
import pytest

import _decode_graph_cases as dc
import _generate_cases as gc

pytestmark = pytest.mark.gpu
KINDS = list(gc.MODELS)


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_skinny(cuda, kind):
    dc.check_teacher_forced_skinny(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_captured_loop_equals_eager_bitwise(cuda, kind):
    dc.check_graph_bitwise(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_captured_loop_blas_agrees_where_sure(cuda, kind):
    dc.check_graph_blas(kind, cuda)


def test_one_graph_object_serves_a_second_call(cuda):
    dc.check_graph_reuse("llama", cuda)
