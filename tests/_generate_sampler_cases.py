"""generate(..., sampler=...) on the tiny models of _generate_cases.py, shared by
test_generate_sampler_cpu.py and test_generate_sampler_gpu.py."""
import pytest
import torch

from _generate_cases import SAMPLE_T, VOCAB, models, sequences
from dtg.models.generation import KVCache, decode_step, generate, prefill, sample_next

KIND = "qwen3"


def _prompts():
    return [s[:n] for s, n in zip(sequences(KIND), (6, 4))]


def check_fused_seeds(dev):
    model, _ = models(KIND, dev)
    kw = dict(temperature=SAMPLE_T, top_k=50, top_p=0.95, min_p=0.001, sampler="fused")
    a = generate(model, _prompts(), 12, seed=1, **kw)
    b = generate(model, _prompts(), 12, seed=1, **kw)
    c = generate(model, _prompts(), 12, seed=2, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "same seed, different ids"
    assert any(not torch.equal(x, y) for x, y in zip(a, c)), "different seeds, same ids"
    assert all(x.shape == (12,) and 0 <= int(t) < VOCAB for x in a for t in x)


def check_fused_per_prompt_greedy(dev):
    model, _ = models(KIND, dev)
    greedy = generate(model, _prompts(), 12, temperature=0.0, sampler="fused")
    mixed = generate(model, _prompts(), 12, temperature=[0.0, SAMPLE_T], top_k=[0, 50], seed=3, sampler="fused")
    assert torch.equal(mixed[0], greedy[0]), "the greedy row of a mixed batch differs from a greedy run"
    assert not torch.equal(mixed[1], greedy[1]), "the sampled row of the mixed batch is greedy"
    assert torch.equal(greedy[0], generate(model, _prompts(), 12, temperature=0.0)[0])  # argmax either way


def check_fused_eos(dev):
    model, _ = models(KIND, dev)
    n = 40
    free = generate(model, _prompts(), n, temperature=SAMPLE_T, seed=5, sampler="fused")

    def first(seq, tok):
        hit = (seq == tok).nonzero()
        return int(hit[0]) + 1 if len(hit) else n

    eos = next((int(t) for t in free[0][:-1] if first(free[0], t) != first(free[1], t)), None)
    assert eos is not None, "no id stops the two sequences at different steps"
    got = generate(model, _prompts(), n, temperature=SAMPLE_T, seed=5, eos_token_id=eos, sampler="fused")
    for f, g in zip(free, got):
        assert torch.equal(g, f[:first(f, eos)]), (g.tolist(), f.tolist())


def check_torch_sampler_unchanged(dev):
    """sampler="torch" is the loop generate() has always run: prefill, then sample_next on one generator."""
    model, _ = models(KIND, dev)
    n, kw = 10, dict(temperature=SAMPLE_T, top_k=50, top_p=0.95)
    got = generate(model, _prompts(), n, seed=7, **kw)
    assert all(torch.equal(x, y) for x, y in zip(got, generate(model, _prompts(), n, seed=7, sampler="torch", **kw)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cache = KVCache(model.config, 2, 6 + n, device=dev, dtype=model.embed_tokens.weight.dtype)
    logits = prefill(model, _prompts(), cache)
    ids = []
    for step in range(n):
        nxt = sample_next(logits, SAMPLE_T, 50, 0.95, gen)
        ids.append(nxt.cpu())
        if step + 1 < n:
            logits = decode_step(model, nxt, cache)
    assert torch.equal(torch.stack(got), torch.stack(ids, 1))


def check_errors(dev):
    model, _ = models(KIND, dev)
    p = _prompts()
    for kw in (dict(min_p=0.05), dict(temperature=[0.0, 1.0]), dict(top_k=[1, 2]), dict(top_p=(0.5, 0.9))):
        with pytest.raises(ValueError, match='sampler="fused"'):
            generate(model, p, 4, **kw)
    for kw in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1), dict(min_p=1.5),
               dict(temperature=[1.0, -1.0]), dict(min_p=[0.0, 2.0]), dict(top_k=[1, 2, 3])):
        with pytest.raises(ValueError):
            generate(model, p, 4, sampler="fused", **kw)
    for kw in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(min_p=1.5), dict(sampler="other")):
        with pytest.raises(ValueError):
            generate(model, p, 4, **kw)
