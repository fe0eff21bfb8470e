"""KV-cache generation (dtg.models.generation) on the CPU operators: teacher-forced equivalence with
the existing full forward, greedy equality, EOS stopping, seeded sampling and the unsupported cases."""
import pytest
import torch

import _generate_cases as G
from dtg.models import build_model, resolve_config
from dtg.models.generation import KVCache, decode_step, generate, prefill, sample_next

CPU = torch.device("cpu")
KINDS = list(G.MODELS)


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_logits_match_full_forward(kind):
    G.check_teacher_forced(kind, CPU)


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_ids_match_full_recompute(kind):
    G.check_greedy(kind, CPU)


def test_eos_stops_each_sequence_at_its_own_step():
    G.check_eos("llama", CPU)


def test_sampling_is_seeded():
    G.check_sampling_seeds("qwen3", CPU)


def test_top_k_and_top_p_restrict_the_support():
    logits = torch.tensor([[4.0, 3.0, 2.0, 1.0, 0.0]]).repeat(64, 1)
    g = torch.Generator().manual_seed(0)
    assert set(sample_next(logits, 1.0, top_k=2, generator=g).tolist()) <= {0, 1}
    assert set(sample_next(logits, 1.0, top_p=0.5, generator=g).tolist()) == {0}       # p0 = 0.64 alone reaches 0.5
    assert set(sample_next(logits, 1.0, top_p=0.7, generator=g).tolist()) <= {0, 1}
    assert sample_next(logits, 0.0).tolist() == [0] * 64


def test_gpt2_is_rejected():
    m = build_model("gpt2-tiny", dtype=torch.float32)
    with pytest.raises(ValueError, match="GPT-2"):
        generate(m, [torch.tensor([1, 2, 3])], 4)


def test_tp_model_is_rejected(tmp_path):
    import torch.distributed as dist

    mine = not dist.is_initialized()
    if mine:
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        m = build_model(G.config("llama"), dtype=torch.float32, tp_group=dist.group.WORLD)
        with pytest.raises(ValueError, match="parallel group"):
            generate(m, [torch.tensor([1, 2, 3])], 4)
    finally:
        if mine:
            dist.destroy_process_group()


def test_length_beyond_the_cache_is_rejected():
    m, _ = G.models("llama", CPU)
    with pytest.raises(ValueError, match="exceeds S_max"):
        generate(m, [torch.arange(10), torch.arange(4)], 8, s_max=17)
    assert [len(o) for o in generate(m, [torch.arange(10), torch.arange(4)], 8, s_max=18)] == [8, 8]
    cache = KVCache(m.config, 1, 4)
    with pytest.raises(ValueError, match="does not fit"):
        prefill(m, [torch.arange(5)], cache)
    prefill(m, [torch.arange(4)], cache)
    with pytest.raises(ValueError, match="cache is full"):
        decode_step(m, torch.tensor([1]), cache)


def test_generate_is_exported_at_the_top_level():
    import dtg

    assert dtg.generate is generate
