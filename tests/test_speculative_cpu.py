"""Speculative decoding on the CPU operators: the loop's bookkeeping (acceptance, budgets, EOS, the drafters),
its errors, and the ids against the plain loop up to the gap rule (the CPU GEMMs promise no row independence,
so no bitwise claim here; test_speculative_gpu.py makes it for the skinny kernels)."""
import pytest
import torch

import _generate_cases as gc
import _spec_cases as sc

CPU = torch.device("cpu")


@pytest.mark.parametrize("kind", list(gc.MODELS))
def test_speculative_ids_agree_with_the_plain_loop_where_sure(kind):
    sc.check_up_to_gaps(kind, CPU)


def test_errors():
    sc.check_errors(CPU)


def test_speculate_none_is_the_plain_loop():
    sc.check_none_is_the_plain_loop(CPU)


def test_ngram_drafter():
    sc.check_ngram_drafter()


def test_budget_and_cache_edge():
    """max_new_tokens no multiple of k and s_max exactly prompt + budget: every row gets exactly its budget, and
    the always-wrong drafter costs one pass per id."""
    import _decode_graph_cases as dc

    ref = sc.reference("llama", CPU, "blas", sc.ODD_NEW, max(dc.PROMPT_LENS) + sc.ODD_NEW)
    spec = sc.Speculative(sc.Oracle(ref, dc.long_prompts("llama"), wrong_at=0), k=4)
    got = sc._spec_run("llama", CPU, "blas", spec, sc.ODD_NEW, max(dc.PROMPT_LENS) + sc.ODD_NEW)
    assert [len(g) for g in got] == [sc.ODD_NEW] * 2
    assert spec.stats["accepted"] == 0 and spec.stats["steps"] == sc.ODD_NEW - 1
