"""Shapes, the f64 reference and the checks of ops.skinny_linear shared by test_skinny_linear_cpu.py and
test_skinny_linear_gpu.py.

Reference: y = sum_k x_k w_k (+ b) in float64 from the bf16 inputs.  Bound (tests/_refs.py): half a bf16
ulp of the reference for the one rounding on store, plus the f32 term of a K-term reduction of products,
K_ * U * (K + 1) * (sum_k |x_k w_k| + |b|): one roundoff per product and one per addition on the
magnitude summed so far (at most the whole sum of magnitudes, K times), one more for the bias, times the
file's factor 8 for the summation order.  It holds for any order of the K terms, so the kernel, the CPU
operator (an f32 matmul) and hipBLASLt (DTG_SKINNY_FUSED=0) are all held to it, with no outliers."""
import pytest
import torch

import _refs
from dtg import ops
from dtg.ops import functional as F_

# (M, N, K): one chunk; N and K off every tile (N % 4, K % 512 partial pass) at M = 1; fewer columns than
# a workgroup's 16 with exactly one pass; several workgroups with a partial second pass at M = 8 (the
# 2-deep unroll); M = 16 with N % 16 = 2 and 8 full passes + 1 chunk; two columns of a long K (28 passes).
SHAPES = [(1, 1, 8), (1, 67, 264), (3, 5, 512), (8, 1024, 520), (16, 130, 4104), (16, 2, 14336)]
SWIGLU_SHAPES = [(1, 2, 8), (5, 134, 264), (16, 1024, 512)]
INVARIANCE_K = [264, 4104]


def inputs(M, N, K, dev, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * M + 13 * N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if bias else None
    return x, w, b


def reference(x, w, b):
    xd, wd = _refs.f64(x), _refs.f64(w)
    ref = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if b is not None:
        ref = ref + _refs.f64(b)
        mag = mag + _refs.f64(b).abs()
    return ref, _refs.K * _refs.U * (x.shape[1] + 1) * mag


def check_accuracy(M, N, K, dev, bias, strided=False):
    x, w, b = inputs(M, N, K, dev, bias)
    if strided:  # rows of a wider buffer: row stride K + 16
        buf = torch.zeros(M, K + 16, dtype=x.dtype, device=dev)
        buf[:, :K] = x
        x = buf[:, :K]
        assert not x.is_contiguous() or M == 1
    ref, term = reference(x, w, b)
    out = ops.skinny_linear(x, w, b)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _refs.assert_within(out, ref, term, f"skinny_linear {M}x{N}x{K}{' +b' if bias else ''}{' strided' if strided else ''}")


def swiglu_any_width(gu):
    """ops.swiglu of a [M, 2 I] gate|up row for any I: the kernel takes I % 8 == 0, so the halves are laid
    into a zero-padded buffer of the next such width and the result is cut back (element-wise op)."""
    M, inter = gu.shape[0], gu.shape[1] // 2
    ip = (inter + 7) // 8 * 8
    if ip == inter:
        return ops.swiglu(gu)
    pad = torch.zeros(M, 2 * ip, dtype=gu.dtype, device=gu.device)
    pad[:, :inter] = gu[:, :inter]
    pad[:, ip:ip + inter] = gu[:, inter:]
    return ops.swiglu(pad)[:, :inter]


def check_swiglu(M, N, K, dev, bias):
    x, w, b = inputs(M, N, K, dev, bias, seed=1)
    fused = ops.skinny_linear(x, w, b, act="swiglu")
    assert fused.shape == (M, N // 2)
    two = swiglu_any_width(ops.skinny_linear(x, w, b, act=None))
    assert torch.equal(fused, two), f"epilogue differs from swiglu(skinny_linear) at {(fused != two).nonzero()[:4].tolist()}"
    assert torch.equal(fused, ops.skinny_linear(x, w, b, act=1))


def check_row_invariance(K, dev):
    x, w, b = inputs(16, 37, K, dev, True, seed=2)
    full = ops.skinny_linear(x, w, b)
    assert torch.equal(full, ops.skinny_linear(x, w, b)), "two identical calls differ"
    for m in range(16):
        assert torch.equal(ops.skinny_linear(x[m:m + 1], w, b)[0], full[m]), f"row {m} alone differs from the batch"
    assert torch.equal(ops.skinny_linear(x[3:10], w, b), full[3:10])


def check_unread(dev):
    """x as a window of a NaN-filled buffer: rows above and below and the columns beside it are never read."""
    M, N, K = 5, 21, 264
    x, w, b = inputs(M, N, K, dev, True, seed=3)
    want = ops.skinny_linear(x, w, b)
    buf = torch.full((M + 4, K + 24), float("nan"), dtype=x.dtype, device=dev)
    buf[2:2 + M, 8:8 + K] = x
    got = ops.skinny_linear(buf[2:2 + M, 8:8 + K], w, b)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


def check_refusals(dev):
    x, w, b = inputs(4, 10, 64, dev)
    op = torch.ops.dtg.skinny_linear
    bad = {
        "M = 0": lambda: op(x[:0], w, b, 0),
        "M > 16": lambda: op(torch.zeros(17, 64, dtype=x.dtype, device=dev), w, b, 0),
        "K % 8": lambda: op(x[:, :60].contiguous(), w[:, :60].contiguous(), b, 0),
        "f32 x": lambda: op(x.float(), w, b, 0),
        "f32 w": lambda: op(x, w.float(), b, 0),
        "non-contiguous w": lambda: op(x, torch.zeros(64, 10, dtype=x.dtype, device=dev).t(), b, 0),
        "misaligned x": lambda: op(torch.zeros(4, 72, dtype=x.dtype, device=dev)[:, 1:65], w, b, 0),
        "row stride % 8": lambda: op(torch.zeros(4, 68, dtype=x.dtype, device=dev)[:, :64], w, b, 0),
        "odd N with act": lambda: op(x, w[:9].contiguous(), None, 1),
        "bias length": lambda: op(x, w, b[:9].contiguous(), 0),
        "act = 2": lambda: op(x, w, b, 2),
    }
    for what, call in bad.items():
        with pytest.raises(RuntimeError, match="dtg: "):
            call()
            pytest.fail(f"{what} was accepted")
    with pytest.raises(ValueError, match="16"):
        ops.skinny_linear(torch.zeros(17, 64, dtype=x.dtype, device=dev), w, b)
    with pytest.raises(ValueError, match="even N"):
        ops.skinny_linear(x, w[:9].contiguous(), None, act="swiglu")
    with pytest.raises(ValueError, match="act"):
        ops.skinny_linear(x, w, b, act="gelu")


def check_composed(dev, monkeypatch):
    """DTG_SKINNY_FUSED=0 (torch.mm / addmm / ops.swiglu) within the kernel's bound."""
    monkeypatch.setattr(F_, "_SKINNY_FUSED", False)
    for M, N, K in SHAPES:
        for bias in (False, True):
            x, w, b = inputs(M, N, K, dev, bias)
            ref, term = reference(x, w, b)
            _refs.assert_within(ops.skinny_linear(x, w, b), ref, term, f"skinny_linear composed {M}x{N}x{K}")
    x, w, b = inputs(16, 1024, 512, dev, True, seed=1)
    assert torch.equal(ops.skinny_linear(x, w, b, act="swiglu"), ops.swiglu(ops.skinny_linear(x, w, b)))
