"""The host side of the captured decode loop and the skinny decode step on the CPU operators."""
import pytest
import torch

import _decode_graph_cases as dc
import _generate_cases as gc
from dtg.models.generation import KVCache, decode_step, generate, prefill


def test_decode_bucket_properties():
    dc.bucket_properties()


def test_graph_needs_a_gpu():
    model, _ = gc.models("llama", "cpu")
    with pytest.raises(ValueError, match="GPU"):
        generate(model, [torch.arange(4)], 4, decode="graph")


def test_graph_with_the_torch_sampler_is_refused():
    model, _ = gc.models("llama", "cpu")
    with pytest.raises(ValueError, match='sampler="fused"'):
        generate(model, [torch.arange(4)], 4, decode="graph", temperature=1.0)


def test_bad_arguments():
    model, _ = gc.models("llama", "cpu")
    with pytest.raises(ValueError, match="linear"):
        generate(model, [torch.arange(4)], 4, linear="cublas")
    with pytest.raises(ValueError, match="decode"):
        generate(model, [torch.arange(4)], 4, decode="captured")


def test_bad_plan_len():
    model, _ = gc.models("llama", "cpu")
    cache = KVCache(model.config, 1, 32, device="cpu")
    prefill(model, [torch.arange(5)], cache)
    for plan_len in (5, 33, 0):
        with pytest.raises(ValueError, match="plan_len"):
            decode_step(model, torch.tensor([1]), cache, plan_len=plan_len)
    assert cache.max_len == 5
    a = decode_step(model, torch.tensor([1]), cache, plan_len=32)
    cache2 = KVCache(model.config, 1, 32, device="cpu")
    prefill(model, [torch.arange(5)], cache2)
    assert torch.equal(a, decode_step(model, torch.tensor([1]), cache2))


def test_seventeen_prompts_with_skinny_are_refused():
    model, _ = gc.models("llama", "cpu")
    with pytest.raises(ValueError, match="16"):
        generate(model, [torch.arange(3)] * 17, 2, linear="skinny")
    cache = KVCache(model.config, 17, 8, device="cpu")
    prefill(model, [torch.arange(3)] * 17, cache)
    with pytest.raises(ValueError, match="16"):
        decode_step(model, torch.zeros(17, dtype=torch.long), cache, linear="skinny")


@pytest.mark.parametrize("kind", list(gc.MODELS))
def test_generate_skinny_runs_on_the_cpu_ops(kind):
    model, _ = gc.models(kind, "cpu")
    prompts = [s[:p] for s, p in zip(gc.sequences(kind), (gc.PREFIX, gc.PREFIX - gc.SHORTER))]
    out = generate(model, prompts, 8, linear="skinny")
    assert all(o.shape == (8,) for o in out)
    assert all(torch.equal(a, b) for a, b in zip(out, generate(model, prompts, 8, linear="skinny", bucketed=True)))


def test_defaults_are_blas_eager():
    model, _ = gc.models("qwen2", "cpu")
    prompts = [s[:p] for s, p in zip(gc.sequences("qwen2"), (gc.PREFIX, gc.PREFIX - gc.SHORTER))]
    a = generate(model, prompts, 12)
    b = generate(model, prompts, 12, linear="blas", decode="eager")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_teacher_forced_skinny_cpu():
    dc.check_teacher_forced_skinny("qwen2", "cpu")


@pytest.mark.parametrize("kind", list(gc.MODELS))
def test_reference_gaps_hold_at_long_prompts(kind):
    dc.check_reference_gaps(kind)
