"""The cases of test_gpt2_kernels_gpu.py run through the package's CPU ops, against the same float64
references with the same bounds (tests/_gpt2_cases.py): the references are right, every f32 term can
be met by a correct f32 implementation, and the LayerNorm bound tells a two-pass variance from a
one-pass one.
"""
import pytest
import torch

import _gpt2_cases as C
import _refs as R

CPU = torch.device("cpu")


@pytest.mark.parametrize("H", C.LN_HIDDEN)
def test_layernorm_hidden_sizes(H):
    C.check_layernorm_hidden(CPU, H)


@pytest.mark.parametrize("H", C.LN_HIDDEN)
def test_rstd_bound_passes_f64(H):
    x, _, w, b, _, _ = C.ln_inputs(5, H, seed=H)
    _, _, rstd_r, _, _ = C.ln_ref(R.f64(x), w, b, C.EPS)
    R.assert_within(rstd_r.float(), rstd_r, C.ln_terms(R.f64(x), w, b, C.EPS)["rstd"], "f64 rstd as f32")


@pytest.mark.parametrize("H", [1600, 2048])
def test_rstd_bound_rejects_one_pass_variance(H):
    """The f32 E[x^2] - mean^2 form is outside the bound on the offset row (see ln_terms for why,
    and for why these two sizes)."""
    x, _, w, b, _, _ = C.ln_inputs(5, H, seed=H)
    _, _, rstd_r, _, _ = C.ln_ref(R.f64(x), w, b, C.EPS)
    t = C.ln_terms(R.f64(x), w, b, C.EPS)
    R.assert_within(rstd_r.float(), rstd_r, t["rstd"], "f64 rstd as f32")
    row = slice(C.OFFSET_ROW, C.OFFSET_ROW + 1)
    with pytest.raises(AssertionError):
        R.assert_within(C.one_pass_rstd(x, C.EPS)[row], rstd_r[row], t["rstd"][row], "one-pass rstd (offset row)")


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("T", C.LN_BWD_T)
def test_layernorm_bwd_rows(T, with_dres):
    C.check_layernorm_bwd_rows(CPU, T, with_dres)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("H", C.LN_BWD_HIDDEN)
def test_layernorm_bwd_hidden_sizes(H, with_dres):
    C.check_layernorm_bwd_hidden(CPU, H, with_dres)


def test_layernorm_strided_rows():
    C.check_layernorm_strided(CPU)


def test_layernorm_empty_and_bad_layouts():
    C.check_layernorm_empty(CPU)
    C.check_layernorm_bad_layouts(CPU, pytest.raises)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_add_layernorm(p):
    C.check_dropout(CPU, p)


@pytest.mark.parametrize("T,I", [(1, 8), (77, 136)])
def test_gelu(T, I):
    C.check_gelu(CPU, T, I)


@pytest.mark.parametrize("T,I", [(8, 8), (72, 136), (136, 264)])
def test_gelu_bwd_t(T, I):
    C.check_gelu_bwd_t(CPU, T, I)


def test_gelu_empty():
    C.check_gelu_empty(CPU)
