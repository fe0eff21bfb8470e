"""The shared argument checks of the RoPE-taking operators (csrc/kernels/rope_common.h): every
perturbation of tests/_rope_arg_cases.py is refused by every operator's host wrapper, by name, with the
activation and the caches left as they were.  Host-side only: nothing is launched on bad arguments."""
import re

import pytest
import torch

import _rope_arg_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("bad", C.PERTURBATIONS)
@pytest.mark.parametrize("op", C.OPERATORS)
def test_bad_arguments_are_refused_by_name(cuda, op, bad, D):
    args = C.valid_args(D, cuda)
    args.update(C.PERTURBATIONS[bad](args))
    watched = [args[k] for k in ("qkv", "kc", "vc")]
    before = [C.storage_bits(t) for t in watched]
    with pytest.raises(RuntimeError, match=re.escape(f"dtg: {op}: ")):
        C.OPERATORS[op](args)
    for t, b in zip(watched, before):
        assert torch.equal(C.storage_bits(t), b), f"{op} wrote to its arguments before refusing {bad}"


@pytest.mark.parametrize("D", C.DIMS)
@pytest.mark.parametrize("op", C.OPERATORS)
def test_unperturbed_arguments_are_accepted(cuda, op, D):
    """The perturbation, not the base case, is what the wrappers refuse."""
    C.OPERATORS[op](C.valid_args(D, cuda))
    torch.cuda.synchronize()
