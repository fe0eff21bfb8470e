"""Speculative decoding on the GPU: with the skinny kernels the ids are the plain loop's bit for bit, whatever
the drafter proposes (tests/_spec_cases.py); Mistral's sliding window moves the verify kernel's tile origin, so
it is held to the gap rule instead."""
import pytest

import _spec_cases as sc

pytestmark = pytest.mark.gpu

BITWISE = [("llama", "skinny"), ("qwen2", "skinny"), ("qwen3", "skinny"), ("llama", "skinny-fp8")]
IDS = [f"{k}-{l}" for k, l in BITWISE]


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_oracle_drafter_bitwise(cuda, kind, linear):
    sc.check_oracle(kind, cuda, linear)


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_wrong_drafts_bitwise(cuda, kind, linear):
    sc.check_wrong(kind, cuda, linear)


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_other_draft_lengths_bitwise(cuda, kind, linear, k):
    sc.check_oracle(kind, cuda, linear, k=k)
    sc.check_wrong(kind, cuda, linear, k=k)


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_odd_budget_in_an_exact_cache_bitwise(cuda, kind, linear):
    tight = max(sc.dc.PROMPT_LENS) + sc.ODD_NEW
    sc.check_oracle(kind, cuda, linear, new=sc.ODD_NEW, s_max=tight)
    sc.check_wrong(kind, cuda, linear, new=sc.ODD_NEW, s_max=tight)


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_fused_sampler_greedy_and_sampled_rows_bitwise(cuda, kind, linear):
    sc.check_oracle(kind, cuda, linear, sampling=sc.MIXED)
    sc.check_wrong(kind, cuda, linear, sampling=sc.MIXED)


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_eos_stops_rows_apart_bitwise(cuda, kind, linear):
    sc.check_eos(kind, cuda, linear)


@pytest.mark.parametrize("kind,linear", BITWISE, ids=IDS)
def test_ngram_drafter_bitwise(cuda, kind, linear):
    sc.check_ngram(kind, cuda, linear)


def test_mistral_window_agrees_where_sure(cuda):
    sc.check_up_to_gaps("mistral", cuda, "skinny")


def test_errors_and_none(cuda):
    sc.check_errors(cuda)
    sc.check_none_is_the_plain_loop(cuda)
