"""KV-cache generation (dtg.models.generation) through the gfx950 kernels: the checks of
tests/_generate_cases.py that test_generate_cpu.py runs on the CPU operators."""
import pytest
import torch

import _generate_cases as G

pytestmark = pytest.mark.gpu
KINDS = list(G.MODELS)


@pytest.mark.parametrize("kind", KINDS)
def test_teacher_forced_logits_match_full_forward(cuda, kind):
    G.check_teacher_forced(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_ids_match_full_recompute(cuda, kind):
    G.check_greedy(kind, cuda)


def test_eos_stops_each_sequence_at_its_own_step(cuda):
    G.check_eos("llama", cuda)


def test_sampling_is_seeded(cuda):
    G.check_sampling_seeds("qwen3", cuda)


def test_composed_path_generates_the_same_logits_within_tolerance(cuda, monkeypatch):
    """DTG_DECODE_FUSED=0 end to end: the same teacher-forced bound."""
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", False)
    G.check_teacher_forced("mistral", cuda)
