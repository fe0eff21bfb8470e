"""generate(..., sampler="fused" | "torch") on the GPU (the fused sampling kernel)."""
import pytest

import _generate_sampler_cases as gs

pytestmark = pytest.mark.gpu


def test_fused_seeds(cuda):
    gs.check_fused_seeds(cuda)


def test_fused_per_prompt_greedy_row(cuda):
    gs.check_fused_per_prompt_greedy(cuda)


def test_fused_eos_prefix(cuda):
    gs.check_fused_eos(cuda)


def test_torch_sampler_is_unchanged(cuda):
    gs.check_torch_sampler_unchanged(cuda)


def test_bad_arguments(cuda):
    gs.check_errors(cuda)
