"""The CPU operator decode_attn_multi (dtg.ops._cpu) and ops.decode_attention_multi built on it, through the
cases, float64 references and bounds of tests/_decode_multi_cases.py (the ones test_decode_attn_multi_gpu.py
runs through the gfx950 kernel)."""
import pytest
import torch

import _decode_multi_cases as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_cpu_multi_matches_f64(run):
    C.check_multi(C.make_case(run[0]), CPU, run[1])


@pytest.mark.parametrize("name", ["straddle", "inactive", "Q1_G4_D64", "Q5_G4_D64", "row_indirection"])
def test_cpu_multi_equals_decode_attn_per_token(name):
    C.check_bitwise(C.make_case(name), CPU, 0)


@pytest.mark.parametrize("fused", [True, False], ids=["op", "composed"])
@pytest.mark.parametrize("name", C.PUBLIC_CASES)
def test_public_op_and_composition_within_bounds(name, fused, monkeypatch):
    C.check_public(C.make_case(name), CPU, fused, 0, monkeypatch)


def test_public_op_validates_on_the_host():
    C.check_public_errors(CPU)


def test_zero_sequences():
    c = C.make_case("straddle")
    e = torch.empty(0, dtype=torch.int32)
    out = torch.ops.dtg.decode_attn_multi(c["qkv"][:0], c["kc"], c["vc"], e, e, c["Q"], c["nq"], c["nkv"], c["D"],
                                          c["scale"], 0, 0, 0)
    assert out.shape == (0, c["nq"] * c["D"])
