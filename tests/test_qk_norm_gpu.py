"""The gfx950 kernels of csrc/kernels/qk_norm.hip against the float64 references and bounds of
tests/_qknorm_cases.py (the cases test_qk_norm_cpu.py runs through the CPU operators).
"""
import pytest
import torch

import _qknorm_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_kernels_match_f64(cuda, case):
    C.check_ops(C.make_case(*case), cuda)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("case", [c for c in C.CASES if c[3] == 65], ids=C.case_id)
def test_public_op_fused_and_composed_within_bounds(cuda, case, fused, monkeypatch):
    C.check_public_op(C.make_case(*case), cuda, fused, monkeypatch)


@pytest.mark.parametrize("rope", [True, False])
def test_zero_tokens_launch_nothing(cuda, rope):
    ops = torch.ops.dtg
    D, nq, nkv = 128, 3, 1
    qkv = torch.empty(0, (nq + 2 * nkv) * D, dtype=torch.bfloat16, device=cuda)
    w = torch.ones(D, dtype=torch.bfloat16, device=cuda)
    cos, sin = (t.to(cuda) for t in C.tables(D)) if rope else (torch.empty(0, device=cuda), torch.empty(0, device=cuda))
    pos = torch.empty(0, dtype=torch.long, device=cuda)
    xqk, rstd = ops.qk_norm_rope_fwd_(qkv, w, w, cos, sin, pos, nq, nkv, D, C.EPS)
    assert xqk.shape == (0, (nq + nkv) * D) and rstd.shape == (0, nq + nkv)
    dwq, dwk = ops.qk_norm_rope_bwd_(qkv.clone(), xqk, rstd, w, w, cos, sin, pos, nq, nkv, D)
    assert dwq.shape == (D,) and not dwq.any() and not dwk.any()


def test_other_head_dims_are_rejected_and_fall_back(cuda, monkeypatch):
    """The kernels exist for D = 64 and 128; the raw operator says so, the public op composes."""
    from dtg import ops

    D, nq, nkv, T = 96, 2, 1, 5
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(T, (nq + 2 * nkv) * D, generator=g).to(torch.bfloat16).to(cuda)
    w = torch.ones(D, dtype=torch.bfloat16, device=cuda)
    e = torch.empty(0, device=cuda)
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        torch.ops.dtg.qk_norm_rope_fwd_(qkv.clone(), w, w, e, e, torch.empty(0, dtype=torch.long, device=cuda), nq, nkv,
                                        D, C.EPS)
    y = ops.qk_norm_rope(qkv.clone(), w, w, C.EPS, nq, nkv, D)
    x = qkv[:, : (nq + nkv) * D].double().reshape(T, nq + nkv, D)
    ref = (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + C.EPS)).reshape(T, -1)
    torch.testing.assert_close(y[:, : (nq + nkv) * D].double(), ref, rtol=2 ** -8, atol=1e-6)
    assert torch.equal(y[:, (nq + nkv) * D:], qkv[:, (nq + nkv) * D:])
