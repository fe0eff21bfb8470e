"""The FP8 KV cache on the gfx950 kernels of csrc/kernels/decode_attn.hip (the e4m3 cache format of the append
and of the decode attention) and through the models: the checks of tests/_kv_fp8_cases.py."""
import pytest

import _decode_cases as C
import _kv_fp8_cases as F

pytestmark = pytest.mark.gpu

KINDS = ["llama", "qwen2", "qwen3", "mistral"]


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_kernel_bit_for_bit(cuda, D, rope):
    F.check_append(D, cuda, rope)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_out_of_range_writes_nothing(cuda, D, rope):
    F.check_append_out_of_range(D, cuda, rope)


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_decode_kernel_matches_f64(cuda, run):
    F.check_decode(F.make_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_decode_kernel_equals_bf16_kernel(cuda, run):
    F.check_decode_bitwise(F.make_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("run", F.MULTI_RUNS, ids=C.run_id)
def test_multi_kernel_equals_bf16_kernel(cuda, run):
    F.check_multi_bitwise(F.make_multi_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", F.PUBLIC_CASES)
def test_public_decode_fused_and_composed(cuda, name, fused, monkeypatch):
    F.check_public(F.make_case(name), cuda, fused, 3 if fused else 0, monkeypatch)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_public_multi_and_append_fused_and_composed(cuda, fused, monkeypatch):
    F.check_public_multi(cuda, fused, monkeypatch)
    F.check_public_append(cuda, fused, monkeypatch)


def test_public_errors(cuda):
    F.check_public_errors(cuda)


def test_zero_sequences_launch_nothing(cuda):
    F.check_zero_sequences(cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_wiring_oracle_bit_for_bit(cuda, kind):
    F.check_wiring(kind, cuda, "skinny", exact=True)


def test_wiring_oracle_blas(cuda):
    F.check_wiring("llama", cuda, "blas", exact=False)


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_captured_loop_bitwise(cuda, kind):
    F.check_graph_bitwise(kind, cuda)


def test_captured_loop_bitwise_fp8_weights(cuda):
    F.check_graph_bitwise("llama", cuda, "skinny-fp8")


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_speculative_bitwise(cuda, kind):
    F.check_speculative(kind, cuda, "skinny")


def test_arguments(cuda):
    F.check_arguments(cuda)
