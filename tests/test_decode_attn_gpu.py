"""The gfx950 kernels of csrc/kernels/decode_attn.hip against the float64 references and bounds of
tests/_decode_cases.py (the cases test_decode_attn_cpu.py runs through the CPU operators)."""
import pytest
import torch

import _decode_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_decode_kernel_matches_f64(cuda, run):
    C.check_decode(C.make_case(run[0]), cuda, run[1])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", ["boundaries", "window", "poisoned_window", "row_indirection", "G7_D64", "logit_range"])
def test_public_op_fused_and_composed_within_bounds(cuda, name, fused, monkeypatch):
    C.check_public_decode(C.make_case(name), cuda, fused, 3 if fused else 0, monkeypatch)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_kernel(cuda, D, rope):
    C.check_append(D, cuda, rope)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "copy_only"])
@pytest.mark.parametrize("D", C.APPEND_DIMS)
def test_append_out_of_range_writes_nothing(cuda, D, rope):
    C.check_append_out_of_range(D, cuda, rope)


def test_zero_sequences_launch_nothing(cuda):
    c = C.make_case("single_key")
    e = torch.empty(0, dtype=torch.int32, device=cuda)
    out = torch.ops.dtg.decode_attn(c["qkv"][:0].to(cuda), c["kc"].to(cuda), c["vc"].to(cuda), e, e, c["nq"], c["nkv"],
                                    c["D"], c["scale"], 0, 0, 0)
    assert out.shape == (0, c["nq"] * c["D"]) and out.is_cuda
    qkv = torch.empty(0, (C.NQ + 2 * C.NKV) * 64, dtype=torch.bfloat16, device=cuda)
    kc, vc = C.fresh_caches(64, cuda)
    torch.ops.dtg.kv_cache_append_(qkv, kc, vc, torch.empty(0, device=cuda), torch.empty(0, device=cuda),
                                   torch.empty(0, dtype=torch.long, device=cuda), e, C.NQ, C.NKV, 64)
    assert (kc.view(torch.int16) == C.SENTINEL).all()


def test_unsupported_shapes_are_rejected_and_compose(cuda):
    """The kernels exist for D = 64 / 128 and G in {1, 2, 3, 4, 7, 8, 16}: the raw operator says so, the
    public op composes the result from torch ops."""
    from dtg import ops

    for D, nq, nkv, msg in ((96, 4, 2, "head_dim must be 64 or 128"), (64, 5, 1, "query heads per kv head")):
        g = torch.Generator().manual_seed(D + nq)
        lens = [9, 70]
        qkv = torch.randn(2, (nq + 2 * nkv) * D, generator=g).to(torch.bfloat16).to(cuda)
        kc = torch.randn(2, nkv, 72, D, generator=g).to(torch.bfloat16).to(cuda)
        vc = torch.randn(2, nkv, 72, D, generator=g).to(torch.bfloat16).to(cuda)
        rows = torch.arange(2, dtype=torch.int32, device=cuda)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=cuda)
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.dtg.decode_attn(qkv, kc, vc, rows, lens_t, nq, nkv, D, D ** -0.5, 70, 0, 0)
        out = ops.decode_attention(qkv, kc, vc, rows, lens_t, nq, nkv, D, 70)
        for b, n in enumerate(lens):
            q = qkv[b, : nq * D].double().reshape(nkv, nq // nkv, D)
            p = torch.softmax(torch.einsum("hgd,hnd->hgn", q, kc[b, :, :n].double()) * D ** -0.5, -1)
            ref = torch.einsum("hgn,hnd->hgd", p, vc[b, :, :n].double()).reshape(-1)
            torch.testing.assert_close(out[b].double(), ref, rtol=2 ** -8, atol=2e-3)
    # the append at D = 96: raw op refuses, public op composes
    D, nq, nkv = 96, 2, 1
    qkv = torch.randn(3, (nq + 2 * nkv) * D).to(torch.bfloat16).to(cuda)
    kc = torch.zeros(2, nkv, 8, D, dtype=torch.bfloat16, device=cuda)
    vc = torch.zeros_like(kc)
    pos, rows = torch.tensor([0, 1, 0], device=cuda), torch.tensor([0, 0, 1], dtype=torch.int32, device=cuda)
    e = torch.empty(0, device=cuda)
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        torch.ops.dtg.kv_cache_append_(qkv.clone(), kc, vc, e, e, pos, rows, nq, nkv, D)
    ops.kv_cache_append(qkv, kc, vc, pos, rows, nq, nkv, D)
    assert torch.equal(kc[0, 0, 1], qkv[1, nq * D:(nq + nkv) * D]) and torch.equal(vc[1, 0, 0], qkv[2, (nq + nkv) * D:])


def test_other_dtypes_compose(cuda):
    """The kernels are bf16; a float32 activation and cache on the GPU take the composition."""
    from dtg import ops

    D, nq, nkv, lens = 64, 4, 2, [9, 33]
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(2, (nq + 2 * nkv) * D, generator=g).to(cuda)
    kc, vc = torch.zeros(2, nkv, 40, D, device=cuda), torch.zeros(2, nkv, 40, D, device=cuda)
    src = torch.randn(sum(lens), (nq + 2 * nkv) * D, generator=g).to(cuda)
    pos = torch.cat([torch.arange(n) for n in lens]).to(cuda)
    rows = torch.repeat_interleave(torch.arange(2), torch.tensor(lens)).to(cuda)
    ops.kv_cache_append(src, kc, vc, pos, rows, nq, nkv, D, pos_max=max(lens) - 1, row_max=1)
    out = ops.decode_attention(qkv, kc, vc, torch.arange(2, device=cuda), torch.tensor(lens, device=cuda), nq, nkv, D, 33)
    off = 0
    for b, n in enumerate(lens):
        k = src[off:off + n, nq * D:(nq + nkv) * D].reshape(n, nkv, D).transpose(0, 1).double()
        v = src[off:off + n, (nq + nkv) * D:].reshape(n, nkv, D).transpose(0, 1).double()
        q = qkv[b, : nq * D].double().reshape(nkv, nq // nkv, D)
        p = torch.softmax(torch.einsum("hgd,hnd->hgn", q, k) * D ** -0.5, -1)
        torch.testing.assert_close(out[b].double(), torch.einsum("hgn,hnd->hgd", p, v).reshape(-1), rtol=1e-4, atol=1e-5)
        off += n
