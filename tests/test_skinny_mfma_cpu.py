"""ops.skinny_linear_mfma on the CPU operator (the f64 bound, its refusals) and the row limits of
linear="skinny-mfma" (64) beside those of linear="skinny" (16, message unchanged)."""
import pytest
import torch

import _generate_cases as gc
import _refs
import _skinny_cases as sc
from dtg import ops
from dtg.models import Speculative
from dtg.models.generation import generate
from dtg.models.speculative import check_speculate
from _skinny_mfma_cases import SHAPES, prompts, raw_refusals


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape, bias):
    x, w, b = sc.inputs(*shape, "cpu", bias)
    _refs.assert_within(ops.skinny_linear_mfma(x, w, b), *sc.reference(x, w, b), f"skinny_linear_mfma cpu {shape}")
    if shape[1] % 2 == 0:
        assert torch.equal(ops.skinny_linear_mfma(x, w, b, act="swiglu"), ops.swiglu(ops.skinny_linear_mfma(x, w, b)))


@pytest.mark.parametrize("what", list(raw_refusals("cpu")))
def test_refusals(what):
    with pytest.raises(RuntimeError, match="dtg: "):
        raw_refusals("cpu")[what]()
    with pytest.raises(ValueError, match="64"):
        ops.skinny_linear_mfma(torch.zeros(65, 64, dtype=torch.bfloat16), torch.zeros(10, 64, dtype=torch.bfloat16))


def test_generate_row_limits():
    model, _ = gc.models("llama", "cpu")
    assert [len(o) for o in generate(model, prompts(17), 2, linear="skinny-mfma")] == [2] * 17
    with pytest.raises(ValueError, match='linear="skinny-mfma" decodes at most 64 sequences per step, got 65'):
        generate(model, prompts(65), 2, linear="skinny-mfma")
    with pytest.raises(ValueError, match='linear="skinny" decodes at most 16 sequences per step, got 17'):
        generate(model, prompts(17), 2, linear="skinny")


def test_check_speculate_row_limits():
    check_speculate(Speculative(k=4), 8, "skinny-mfma", False, "torch", 0.0)
    with pytest.raises(ValueError, match="17 x 4 = 68 rows per step, over the skinny limit of 64"):
        check_speculate(Speculative(k=4), 17, "skinny-mfma", False, "torch", 0.0)
