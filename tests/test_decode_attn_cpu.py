"""The CPU operators kv_cache_append_ / decode_attn (dtg.ops._cpu) and the public ops built on them,
through the cases, float64 references and bounds of tests/_decode_cases.py (the ones
test_decode_attn_gpu.py runs through the gfx950 kernels)."""
import pytest
import torch

import _decode_cases as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_cpu_decode_matches_f64(run):
    C.check_decode(C.make_case(run[0]), CPU, run[1])


@pytest.mark.parametrize("fused", [True, False], ids=["op", "composed"])
@pytest.mark.parametrize("name", ["boundaries", "window", "poisoned_window", "row_indirection", "G7_D64"])
def test_public_decode_op_and_composition_within_bounds(name, fused, monkeypatch):
    C.check_public_decode(C.make_case(name), CPU, fused, 0, monkeypatch)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_cpu_append(D, rope):
    C.check_append(D, CPU, rope)
    C.check_append_out_of_range(D, CPU, rope)


@pytest.mark.parametrize("fused", [True, False], ids=["op", "composed"])
def test_public_append_matches_raw_op(fused, monkeypatch):
    """ops.kv_cache_append (either path) leaves qkv and the caches as the raw operator does."""
    from dtg import ops
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    D = 64
    cos, sin = C.tables(D)
    x = C.append_inputs(D, 6, 1)
    pos, rows = torch.tensor(C.PREFILL["pos"]), torch.tensor(C.PREFILL["rows"], dtype=torch.int32)
    kc, vc = C.fresh_caches(D, CPU)
    want = x.clone()
    torch.ops.dtg.kv_cache_append_(want, kc, vc, cos, sin, pos, rows, C.NQ, C.NKV, D)
    kc2, vc2 = C.fresh_caches(D, CPU)
    got = ops.kv_cache_append(x.clone(), kc2, vc2, pos, rows, C.NQ, C.NKV, D, cos, sin)
    for a, b in ((got, want), (kc2, kc), (vc2, vc)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_zero_sequences():
    c = C.make_case("single_key")
    e = torch.empty(0, dtype=torch.int32)
    out = torch.ops.dtg.decode_attn(c["qkv"][:0], c["kc"], c["vc"], e, e, c["nq"], c["nkv"], c["D"], c["scale"], 0, 0, 0)
    assert out.shape == (0, c["nq"] * c["D"])


def test_public_ops_validate_on_the_host():
    from dtg import ops

    c = C.make_case("single_key")
    a = (c["qkv"], c["kc"], c["vc"], c["rows"], c["lens"], c["nq"], c["nkv"], c["D"])
    with pytest.raises(ValueError, match="max_len"):
        ops.decode_attention(*a, c["kc"].shape[2] + 1)
    with pytest.raises(ValueError, match="caches must be"):
        ops.decode_attention(c["qkv"], c["kc"][:, :1], c["vc"], *a[3:], 1)
    with pytest.raises(ValueError, match="integer tensor"):
        ops.decode_attention(c["qkv"], c["kc"], c["vc"], c["rows"].float(), *a[4:], 1)
    with pytest.raises(ValueError, match="qkv must be"):
        ops.kv_cache_append(c["qkv"][:, :-8], c["kc"], c["vc"], c["lens"].long(), c["rows"], c["nq"], c["nkv"], c["D"])
    pos, rows = c["lens"].long(), c["rows"]
    with pytest.raises(ValueError, match="outside the cache"):
        ops.kv_cache_append(c["qkv"].clone(), c["kc"].clone(), c["vc"].clone(), pos, rows, c["nq"], c["nkv"], c["D"],
                            pos_max=c["kc"].shape[2])
    with pytest.raises(ValueError, match="cache row"):
        ops.kv_cache_append(c["qkv"].clone(), c["kc"].clone(), c["vc"].clone(), pos, rows, c["nq"], c["nkv"], c["D"],
                            row_max=c["kc"].shape[0])
