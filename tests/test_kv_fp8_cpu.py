"""The FP8 KV cache on the CPU operators (dtg.ops._cpu) and the CPU plumbing of the models: the checks of
tests/_kv_fp8_cases.py that test_kv_fp8_gpu.py runs on the gfx950 kernels."""
import pytest

import _decode_cases as C
import _kv_fp8_cases as F

CPU = "cpu"


def test_scale_rule_on_boundary_vectors():
    F.check_scale_rule()


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_bit_for_bit(D, rope):
    F.check_append(D, CPU, rope)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_out_of_range_writes_nothing(D, rope):
    F.check_append_out_of_range(D, CPU, rope)


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_decode_matches_f64(run):
    F.check_decode(F.make_case(run[0]), CPU, run[1])


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_decode_equals_bf16_op_on_dequantised_cache(run):
    F.check_decode_bitwise(F.make_case(run[0]), CPU, run[1])


@pytest.mark.parametrize("run", F.MULTI_RUNS, ids=C.run_id)
def test_multi_equals_bf16_op_on_dequantised_cache(run):
    F.check_multi_bitwise(F.make_multi_case(run[0]), CPU, run[1])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", F.PUBLIC_CASES)
def test_public_decode_fused_and_composed(name, fused, monkeypatch):
    F.check_public(F.make_case(name), CPU, fused, 3 if fused else 0, monkeypatch)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_public_multi_and_append_fused_and_composed(fused, monkeypatch):
    F.check_public_multi(CPU, fused, monkeypatch)
    F.check_public_append(CPU, fused, monkeypatch)


def test_public_errors():
    F.check_public_errors(CPU)


def test_zero_sequences():
    F.check_zero_sequences(CPU)


@pytest.mark.parametrize("kind", ["llama", "qwen2", "qwen3", "mistral"])
def test_wiring_oracle(kind):
    F.check_wiring(kind, CPU, "blas", exact=False)


def test_speculative_on_fp8_cache():
    F.check_speculative("llama", CPU, "blas")


def test_arguments():
    F.check_arguments(CPU)
