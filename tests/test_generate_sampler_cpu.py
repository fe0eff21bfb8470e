"""generate(..., sampler="fused" | "torch") on the CPU (the f64 sampling operator)."""
import torch

import _generate_sampler_cases as gs

DEV = torch.device("cpu")


def test_fused_seeds():
    gs.check_fused_seeds(DEV)


def test_fused_per_prompt_greedy_row():
    gs.check_fused_per_prompt_greedy(DEV)


def test_fused_eos_prefix():
    gs.check_fused_eos(DEV)


def test_torch_sampler_is_unchanged():
    gs.check_torch_sampler_unchanged(DEV)


def test_bad_arguments():
    gs.check_errors(DEV)
