"""The gfx950 kernel behind decode_attn_multi (csrc/kernels/decode_attn.hip, the query-tiled form of the
decode attention) against the float64 references and bounds of tests/_decode_multi_cases.py, and bit for bit
against decode_attn on every token alone."""
import pytest
import torch

import _decode_multi_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_multi_kernel_matches_f64(cuda, run):
    C.check_multi(C.make_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("run", C.BITWISE_RUNS, ids=C.run_id)
def test_multi_kernel_equals_decode_attn_per_token_bitwise(cuda, run):
    C.check_bitwise(C.make_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", C.PUBLIC_CASES)
def test_public_op_fused_and_composed_within_bounds(cuda, name, fused, monkeypatch):
    C.check_public(C.make_case(name), cuda, fused, 3 if fused else 0, monkeypatch)


def test_public_op_validates_on_the_host(cuda):
    C.check_public_errors(cuda)


def test_raw_op_checks_and_zero_sequences(cuda):
    c = C.make_case("straddle")
    qkv, kc, vc, rows, lens = (c[k].to(cuda) for k in ("qkv", "kc", "vc", "rows", "lens"))
    a = (c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"], 0, 0)
    with pytest.raises(RuntimeError, match="q_len"):
        torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows, lens, 5, *a)
    with pytest.raises(RuntimeError, match="one entry per sequence"):
        torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows[:-1], lens, c["Q"], *a)
    with pytest.raises(RuntimeError, match="one entry per token"):
        torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows, lens[:-1], c["Q"], *a)
    with pytest.raises(RuntimeError, match="max_len"):
        torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows, lens, c["Q"], c["nq"], c["nkv"], c["D"], c["scale"],
                                        kc.shape[2] + 1, 0, 0)
    e = torch.empty(0, dtype=torch.int32, device=cuda)
    out = torch.ops.dtg.decode_attn_multi(qkv[:0], kc, vc, e, e, c["Q"], *a)
    assert out.shape == (0, c["nq"] * c["D"]) and out.is_cuda
