"""The weight gradients of the norm kernels promise "fixed order, bitwise reproducible".  With
T <= 512 every backward workgroup owns one row, so the f32 partial matrix is known exactly and the
column sum of csrc/kernels/norm_common.h can be replayed on the CPU addition by addition: lane
group g of 16 adds rows g, g + 16, g + 32, ... in order starting from 0, group 0 then adds the 16
group sums in order 0..15 starting from 0, and the result is rounded to bf16 once.

T = 40, H = 24: two column-sum workgroups, the second half full; the lane groups hold 3 or 2 rows.
"""
import pytest
import torch

from dtg import ops  # noqa: F401  (registers torch.ops.dtg)

pytestmark = pytest.mark.gpu
dops = torch.ops.dtg
BF = torch.bfloat16
T, H = 40, 24
GROUPS = 16


def fixed_order_colsum(part):
    """part: f32 [nrows, W] on the CPU.  Every addition is one explicit f32 row addition."""
    nrows, W = part.shape
    t = torch.zeros(W, dtype=torch.float32)
    for g in range(GROUPS):
        s = torch.zeros(W, dtype=torch.float32)
        for r in range(g, nrows, GROUPS):
            s = s + part[r]
        t = t + s
    return t.to(BF)


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).to(BF)
    dy = torch.randn(T, H, generator=g).to(BF)
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    b = (0.1 * torch.randn(H, generator=g)).to(BF)
    return x, dy, w, b


def test_rmsnorm_dw_summation_order(cuda):
    x, dy, w, _ = _inputs(40)
    _, rstd = dops.rmsnorm_fwd(x.to(cuda), w.to(cuda), 1e-5)
    _, dw = dops.rmsnorm_bwd(dy.to(cuda), x.to(cuda), w.to(cuda), rstd, None)
    # a one-row block's partial is 0 + dy * bf16(x * rstd); the product of two bf16 values is exact
    # in f32, so contraction into an FMA cannot change it
    p = dy.float() * (x.float() * rstd.cpu()[:, None]).to(BF).float()
    assert p.dtype == torch.float32
    assert torch.equal(dw.cpu(), fixed_order_colsum(p))


def test_layernorm_db_summation_order(cuda):
    """db's partial of a one-row block is dy itself: matrix 1 of the shared column sum."""
    h, dy, w, b = _inputs(41)
    _, mean, rstd = dops.layernorm_fwd(h.to(cuda), w.to(cuda), b.to(cuda), 1e-5)
    _, _, _, db = dops.layernorm_bwd(dy.to(cuda), h.to(cuda), w.to(cuda), mean, rstd, None, 0.0, None)
    assert torch.equal(db.cpu(), fixed_order_colsum(dy.float()))


def test_layernorm_db_order_decides_the_result(cuda):
    """The one bf16 rounding hides most reorderings of random inputs.  Here every column holds
    +2^30 and -2^30 in two random rows and integers in [-8, 8] elsewhere: what is added while a sum
    stands at 2^30 is lost (the f32 ulp there is 128), so the result depends on which rows meet in
    which lane group and in what order, and only the kernel's order gives the expected integers."""
    h, _, w, b = _inputs(42)
    g = torch.Generator().manual_seed(43)
    dy = torch.randint(-8, 9, (T, H), generator=g).float()
    for c in range(H):
        r_pos, r_neg = torch.randperm(T, generator=g)[:2]
        dy[r_pos, c], dy[r_neg, c] = 2.0 ** 30, -(2.0 ** 30)
    dy = dy.to(BF)
    expected = fixed_order_colsum(dy.float())
    in_row_order = torch.zeros(H)
    for r in range(T):
        in_row_order = in_row_order + dy.float()[r]
    assert (expected != in_row_order.to(BF)).sum() > H // 2, "the case does not tell the orders apart"
    _, mean, rstd = dops.layernorm_fwd(h.to(cuda), w.to(cuda), b.to(cuda), 1e-5)
    _, _, _, db = dops.layernorm_bwd(dy.to(cuda), h.to(cuda), w.to(cuda), mean, rstd, None, 0.0, None)
    assert torch.equal(db.cpu(), expected)
