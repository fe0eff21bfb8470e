"""The CPU implementations of qk_norm_rope_fwd_ / qk_norm_rope_bwd_ (dtg.ops._cpu) against the float64
references and bounds of tests/_qknorm_cases.py -- the cases test_qk_norm_gpu.py runs through the HIP
kernels -- and the autograd node against the composed path.
"""
import pytest
import torch

import _qknorm_cases as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_ops_match_f64(case):
    C.check_ops(C.make_case(*case), CPU)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("case", [c for c in C.CASES if c[3] == 65], ids=C.case_id)
def test_public_op_fused_and_composed_within_bounds(case, fused, monkeypatch):
    C.check_public_op(C.make_case(*case), CPU, fused, monkeypatch)


@pytest.mark.parametrize("rope", [True, False])
def test_zero_tokens(rope):
    ops = torch.ops.dtg
    D, nq, nkv = 64, 3, 1
    qkv = torch.empty(0, (nq + 2 * nkv) * D, dtype=torch.bfloat16)
    w = torch.ones(D, dtype=torch.bfloat16)
    cos, sin = C.tables(D) if rope else (torch.empty(0), torch.empty(0))
    pos = torch.empty(0, dtype=torch.long)
    xqk, rstd = ops.qk_norm_rope_fwd_(qkv, w, w, cos, sin, pos, nq, nkv, D, C.EPS)
    assert xqk.shape == (0, (nq + nkv) * D) and rstd.shape == (0, nq + nkv)
    dwq, dwk = ops.qk_norm_rope_bwd_(qkv.clone(), xqk, rstd, w, w, cos, sin, pos, nq, nkv, D)
    assert dwq.shape == (D,) and not dwq.any() and not dwk.any()


def test_autograd_with_attention_matches_composed_f32(monkeypatch):
    """ops.qk_norm_rope + ops.attention (no RoPE in the attention node) in f32 on the CPU: the fused
    node's hand-written backward against autograd through the composed path."""
    from dtg import ops
    from dtg.ops import functional

    D, nq, nkv, T = 64, 4, 2, 48
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(T, (nq + 2 * nkv) * D, generator=g)
    wq0, wk0 = 1 + 0.3 * torch.randn(D, generator=g), 1 + 0.3 * torch.randn(D, generator=g)
    do = torch.randn(T, nq * D, generator=g)
    cos, sin = C.tables(D)
    pos = torch.cat([torch.arange(20), torch.arange(28)])
    cu = torch.tensor([0, 20, 48], dtype=torch.int32)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(functional, "_QKNORM_FUSED", fused)
        x, wq, wk = (t.clone().requires_grad_() for t in (x0, wq0, wk0))
        y = ops.qk_norm_rope(x * 1.0, wq, wk, C.EPS, nq, nkv, D, cos, sin, pos, grad_inplace=fused)
        o = ops.attention(y, nq, nkv, D, cu, 28)
        o.backward(do)
        res[fused] = (o.detach(), x.grad, wq.grad, wk.grad)
    for a, b, n in zip(res[True], res[False], ("o", "dx", "dwq", "dwk")):
        torch.testing.assert_close(a, b, rtol=1.3e-6 * 50, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
    assert res[True][2].abs().max() > 1e-3  # the weights do receive gradient


def test_weight_grads_are_routed_into_main_grad(monkeypatch):
    """Both paths hand dwq / dwk to grad_routing.route_param_grad (the flat-buffer engines' entry)."""
    from dtg import ops
    from dtg.ops import functional, grad_routing

    D, nq, nkv, T = 64, 3, 1, 9
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(T, (nq + 2 * nkv) * D, generator=g)
    w0 = 1 + 0.3 * torch.randn(2, D, generator=g)
    dy = torch.randn_like(x0)
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(functional, "_QKNORM_FUSED", fused)
        wq, wk = (t.clone().requires_grad_() for t in w0)
        for p in (wq, wk):
            p.main_grad = torch.full((D,), 7.0)
        x = x0.clone().requires_grad_()
        ops.qk_norm_rope(x, wq, wk, C.EPS, nq, nkv, D).backward(dy)
        assert wq.grad is None and wk.grad is None
        got[fused] = (wq.main_grad.clone(), wk.main_grad.clone())
        grad_routing.reset_grad_state([wq, wk])
    for a, b in zip(got[True], got[False]):
        assert not torch.equal(a, torch.full((D,), 7.0))
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
