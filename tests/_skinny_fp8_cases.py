"""Shapes, the f64 reference and the checks of ops.skinny_linear_fp8 and ops.quantize_fp8_rows shared by
test_skinny_fp8_cpu.py and test_skinny_fp8_gpu.py.

Reference: y = (sum_k x_k q_k) * scale (+ b) in float64 from the bf16 x, the e4m3 codes widened by torch on
the CPU (q) and the f32 scale.  Bound (tests/_refs.py): half a bf16 ulp of the reference for the one
rounding on store, plus K_ * U * (K + 2) * (sum_k |x_k q_k| * |scale| + |b|): the K-term reduction and the
products as in tests/_skinny_cases.py, and one more operation for the multiply by the scale.  It holds for
any order of the K terms, so the kernel, the CPU operator and the composed path (DTG_SKINNY_FUSED=0) are all
held to it, with no outliers.

The quantiser's bound: e4m3 has 3 stored significand bits, so rounding to it moves a normal value by at
most 2^-4 of its magnitude, and its subnormals are spaced 2^-9 apart, half of that 2^-10 -- both in units of
the row's scale.  With pow2=False the division by the scale rounds once more in f32 (and the quotient of
the largest element may be clamped back by one f32 ulp): 2 U |w|."""
import pytest
import torch

import _refs
import _skinny_cases as sc
from dtg import ops
from dtg.ops import functional as F_

FP8 = torch.float8_e4m3fn
# (M, N, K).  A lane takes 16-element chunks l, l + 64, ...; the loop issues kUnroll * 64 chunks per iteration,
# kUnroll = 4 for M <= 4, 2 for M <= 8, 1 above.
#   (1, 1, 16)       one chunk, one column
#   (1, 67, 272)     N % 4 != 0 (clamped rows in the last wave) and 17 chunks: a partial pass
#   (3, 5, 1024)     fewer columns than a workgroup's 16, exactly 64 chunks: one full pass of the lanes
#   (2, 9, 4368)     273 chunks at the 4-deep unroll: one full iteration and a partial second one
#   (8, 1024, 1040)  several workgroups, 65 chunks: a partial second pass of the 2-deep unroll
#   (16, 130, 8208)  M = 16 (1-deep), N % 16 = 2, 513 chunks: 8 full passes plus one chunk
#   (16, 2, 14336)   two columns of the longest K in use, 14 passes
SHAPES = [(1, 1, 16), (1, 67, 272), (3, 5, 1024), (2, 9, 4368), (8, 1024, 1040), (16, 130, 8208), (16, 2, 14336)]
POW2 = {s: i % 2 == 0 for i, s in enumerate(SHAPES)}  # every other shape takes amax / 448 scales
SWIGLU_SHAPES = [(1, 2, 16), (5, 134, 272), (16, 1024, 512)]
INVARIANCE_K = [272, 8208]


def inputs(M, N, K, dev, bias=True, seed=0, pow2=True):
    g = torch.Generator().manual_seed(seed + 7 * M + 13 * N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    wq, scale = ops.quantize_fp8_rows(w, pow2=pow2)  # on the CPU; the quantiser has its own checks below
    b = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if bias else None
    return x, wq.to(dev), scale.to(dev), b


def reference(x, wq, scale, b):
    xd, qd, sd = _refs.f64(x), _refs.f64(wq.cpu().float()), _refs.f64(scale)
    ref = (xd @ qd.t()) * sd
    mag = (xd.abs() @ qd.abs().t()) * sd.abs()
    if b is not None:
        ref = ref + _refs.f64(b)
        mag = mag + _refs.f64(b).abs()
    return ref, _refs.K * _refs.U * (x.shape[1] + 2) * mag


def check_every_code(dev):
    """All 256 byte codes (the two NaN codes replaced by 0) through an identity x: the kernel's widening is
    torch's e4m3fn -- not fnuz, no byte or word of the packed conversion out of order, subnormals right."""
    codes = torch.arange(256, dtype=torch.int32)
    codes[0x7F] = codes[0xFF] = 0
    wq = codes.to(torch.uint8).view(16, 16).contiguous().view(FP8)
    scale = torch.tensor([2.0 ** (n - 8) for n in range(16)], dtype=torch.float32)
    want = (wq.float() * scale[:, None]).t().to(torch.bfloat16)
    assert want.float().abs().max() == 448 * 2.0 ** 7 and torch.isfinite(want.float()).all()
    x = torch.eye(16, dtype=torch.bfloat16, device=dev)
    got = ops.skinny_linear_fp8(x, wq.to(dev), scale.to(dev))
    bad = (got.cpu() != want).nonzero()
    assert torch.equal(got.cpu(), want), f"codes {[(int(n) * 16 + int(m)) for m, n in bad[:8]]} widen differently"


def check_accuracy(M, N, K, dev, bias, strided=False, pow2=True):
    x, wq, scale, b = inputs(M, N, K, dev, bias, pow2=pow2)
    if strided:  # rows of a wider buffer: row stride K + 16
        buf = torch.zeros(M, K + 16, dtype=x.dtype, device=dev)
        buf[:, :K] = x
        x = buf[:, :K]
        assert not x.is_contiguous() or M == 1
    ref, term = reference(x, wq, scale, b)
    out = ops.skinny_linear_fp8(x, wq, scale, b)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _refs.assert_within(out, ref, term, f"skinny_linear_fp8 {M}x{N}x{K}{' +b' if bias else ''}"
                        f"{'' if pow2 else ' amax/448'}{' strided' if strided else ''}")


def check_swiglu(M, N, K, dev, bias):
    x, wq, scale, b = inputs(M, N, K, dev, bias, seed=1, pow2=(M != 5))
    fused = ops.skinny_linear_fp8(x, wq, scale, b, act="swiglu")
    assert fused.shape == (M, N // 2)
    two = sc.swiglu_any_width(ops.skinny_linear_fp8(x, wq, scale, b, act=None))
    assert torch.equal(fused, two), f"epilogue differs from swiglu(skinny_linear_fp8) at {(fused != two).nonzero()[:4].tolist()}"
    assert torch.equal(fused, ops.skinny_linear_fp8(x, wq, scale, b, act=1))


def check_row_invariance(K, dev):
    x, wq, scale, b = inputs(16, 37, K, dev, True, seed=2)
    full = ops.skinny_linear_fp8(x, wq, scale, b)
    assert torch.equal(full, ops.skinny_linear_fp8(x, wq, scale, b)), "two identical calls differ"
    for m in range(16):
        assert torch.equal(ops.skinny_linear_fp8(x[m:m + 1], wq, scale, b)[0], full[m]), f"row {m} alone differs from the batch"
    assert torch.equal(ops.skinny_linear_fp8(x[3:10], wq, scale, b), full[3:10])


def check_unread(dev):
    """x as a window of a NaN-filled buffer: rows above and below and the columns beside it are never read."""
    M, N, K = 5, 21, 272
    x, wq, scale, b = inputs(M, N, K, dev, True, seed=3)
    want = ops.skinny_linear_fp8(x, wq, scale, b)
    buf = torch.full((M + 4, K + 24), float("nan"), dtype=x.dtype, device=dev)
    buf[2:2 + M, 8:8 + K] = x
    got = ops.skinny_linear_fp8(buf[2:2 + M, 8:8 + K], wq, scale, b)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


def check_refusals(dev):
    x, wq, scale, b = inputs(4, 10, 64, dev)
    op = torch.ops.dtg.skinny_linear_fp8
    z = lambda *shape, dtype=x.dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    off_by_one = torch.zeros(10 * 64 + 16, dtype=torch.uint8, device=dev)[1:1 + 10 * 64].view(FP8).view(10, 64)
    assert off_by_one.is_contiguous() and off_by_one.data_ptr() % 16
    bad = {
        "M = 0": lambda: op(x[:0], wq, scale, b, 0),
        "M > 16": lambda: op(z(17, 64), wq, scale, b, 0),
        "K % 16": lambda: op(x[:, :56].contiguous(), wq[:, :56].contiguous(), scale, b, 0),
        "f32 x": lambda: op(x.float(), wq, scale, b, 0),
        "bf16 wq": lambda: op(x, wq.to(torch.bfloat16), scale, b, 0),
        "e5m2 wq": lambda: op(x, wq.view(torch.float8_e5m2), scale, b, 0),
        "fnuz wq": lambda: op(x, wq.view(torch.float8_e4m3fnuz), scale, b, 0),
        "f64 scale": lambda: op(x, wq, scale.double(), b, 0),
        "bf16 scale": lambda: op(x, wq, scale.to(torch.bfloat16), b, 0),
        "scale length": lambda: op(x, wq, scale[:9].contiguous(), b, 0),
        "scale [N, 1]": lambda: op(x, wq, scale[:, None], b, 0),
        "strided scale": lambda: op(x, wq, z(20, dtype=torch.float32)[::2], b, 0),
        "non-contiguous wq": lambda: op(x, z(64, 10).to(FP8).t(), scale, b, 0),
        "misaligned wq": lambda: op(x, off_by_one, scale, b, 0),
        "misaligned x": lambda: op(z(4, 72)[:, 1:65], wq, scale, b, 0),
        "row stride % 8": lambda: op(z(4, 68)[:, :64], wq, scale, b, 0),
        "odd N with act": lambda: op(x, wq[:9].contiguous(), scale[:9].contiguous(), None, 1),
        "bias length": lambda: op(x, wq, scale, b[:9].contiguous(), 0),
        "f32 bias": lambda: op(x, wq, scale, b.float(), 0),
        "act = 2": lambda: op(x, wq, scale, b, 2),
    }
    if torch.device(dev).type != "cpu":
        bad["scale on the CPU"] = lambda: op(x, wq, scale.cpu(), b, 0)
    for what, call in bad.items():
        with pytest.raises(RuntimeError, match="dtg: "):
            call()
            pytest.fail(f"{what} was accepted")
    with pytest.raises(ValueError, match="16"):
        ops.skinny_linear_fp8(z(17, 64), wq, scale, b)
    with pytest.raises(ValueError, match="even N"):
        ops.skinny_linear_fp8(x, wq[:9].contiguous(), scale[:9].contiguous(), None, act="swiglu")
    with pytest.raises(ValueError, match="act"):
        ops.skinny_linear_fp8(x, wq, scale, b, act="gelu")
    with pytest.raises(ValueError, match="do not match"):
        ops.skinny_linear_fp8(x[:, :32], wq, scale, b)
    with pytest.raises(ValueError, match="scale"):
        ops.skinny_linear_fp8(x, wq, scale[:9], b)


def check_composed(dev, monkeypatch):
    """DTG_SKINNY_FUSED=0 (an f32 torch.mm, the scale, the bias, one rounding, ops.swiglu) within the kernel's
    bound."""
    monkeypatch.setattr(F_, "_SKINNY_FUSED", False)
    for M, N, K in SHAPES:
        for bias in (False, True):
            x, wq, scale, b = inputs(M, N, K, dev, bias, pow2=POW2[(M, N, K)])
            ref, term = reference(x, wq, scale, b)
            _refs.assert_within(ops.skinny_linear_fp8(x, wq, scale, b), ref, term, f"skinny_linear_fp8 composed {M}x{N}x{K}")
    x, wq, scale, b = inputs(16, 1024, 512, dev, True, seed=1)
    assert torch.equal(ops.skinny_linear_fp8(x, wq, scale, b, act="swiglu"), ops.swiglu(ops.skinny_linear_fp8(x, wq, scale, b)))


# ------------------------------------------------------------------------------------------ the quantiser
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def quantiser_matrix(dtype):
    """[40, 272]: random rows at magnitudes 2^-60 ... 2^57, then the special rows."""
    g = torch.Generator().manual_seed(11)
    w = torch.randn(40, 272, generator=g) / 272 ** 0.5
    w[:32] *= torch.ldexp(torch.ones(32), torch.arange(32) * 4 - 64)[:, None] * (1 + torch.rand(32, 1, generator=g))
    w[32] = 0                                   # an all-zero row
    w[33, 5] = BF16_MAX                         # the bf16 maximum (the rest of the row underflows to 0)
    w[34, 7] = -BF16_MAX
    w[35] = w[35].clamp(-0.2, 0.2)
    w[35, 3] = 448 * 2.0 ** -11                 # largest magnitude exactly 448 * 2^k: the quotient is 448 itself
    w[36] = w[36].clamp(-0.2, 0.2)
    w[36, 9] = -224 * 2.0 ** -9                 # exactly 224 * 2^k: the interval is open there, the quotient is 448
    w[37] = w[37] * 2.0 ** -120                 # below the scale's floor: everything rounds to 0
    w[38] = 465.0 / 448 * w[38].abs().max()     # a constant row
    w[39, 0] = 2.0 ** -126                      # a lone tiny value among larger ones
    return w.to(dtype)


def check_quantiser(dev, pow2, dtype=torch.bfloat16):
    w = quantiser_matrix(dtype)
    wq, scale = ops.quantize_fp8_rows(w.to(dev), pow2=pow2)
    assert wq.dtype == FP8 and wq.shape == w.shape and wq.is_contiguous() and wq.device == torch.device(dev)
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],) and scale.is_contiguous()
    wq, scale = wq.cpu(), scale.cpu()
    codes = wq.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any(), "a NaN code was emitted"
    wd, sd = w.double(), scale.double()
    deq = wq.float().double() * sd[:, None]
    bound = 2.0 ** -4 * wd.abs() + 2.0 ** -10 * sd[:, None] + (0 if pow2 else 2 * _refs.U * wd.abs())
    ratio = ((wd - deq).abs() / bound).max().item()
    print(f"[fp8] quantiser {dtype} pow2={pow2} on {dev}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert scale[32] == 1 and (codes[32] & 0x7F == 0).all(), "an all-zero row must give zeros with scale 1"
    assert torch.isfinite(scale).all() and (scale >= 2.0 ** -100).all()
    assert torch.isfinite(wq[33:35].float()).all() and wq[33].float().abs().max() > 224
    assert scale[37] == 2.0 ** -100 and (codes[37] & 0x7F == 0).all()
    amax = wd.abs().amax(1)
    top = amax / sd
    live = (amax > 0) & (scale > 2.0 ** -100)
    if pow2:
        m, _ = torch.frexp(scale)
        assert (m == 0.5).all(), "a scale is no power of two"
        assert ((top > 224) & (top <= 448))[live].all(), f"quotients {top[live & ~((top > 224) & (top <= 448))].tolist()} outside (224, 448]"
        assert top[35] == 448 and top[36] == 448
        d32 = wq.float() * scale[:, None]
        assert torch.equal(d32.to(torch.bfloat16).float(), d32), "q * scale is not exactly a bf16 value"
    else:
        assert ((top - 448).abs() <= 448 * 2 * _refs.U)[live].all()
    return wq, scale


def check_quantiser_devices_agree(dev):
    for dtype in (torch.bfloat16, torch.float32):
        w = quantiser_matrix(dtype)
        q0, s0 = ops.quantize_fp8_rows(w, pow2=True)
        q1, s1 = ops.quantize_fp8_rows(w.to(dev), pow2=True)
        assert torch.equal(s0, s1.cpu()), "scales differ between the CPU and the device"
        assert torch.equal(q0.view(torch.uint8), q1.cpu().view(torch.uint8)), "codes differ between the CPU and the device"


def check_quantiser_refusals():
    with pytest.raises(ValueError, match="bf16 or f32"):
        ops.quantize_fp8_rows(torch.zeros(4, 16, dtype=torch.float16))
    with pytest.raises(ValueError, match="N, K"):
        ops.quantize_fp8_rows(torch.zeros(16))
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_fp8_rows(torch.full((2, 16), float("inf")))
