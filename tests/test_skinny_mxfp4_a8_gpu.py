"""W4A8 on the gfx950 kernels of csrc/kernels/skinny_mfma.hip: ops.quantize_mxfp8_rows bit for bit against the torch
rule, the operand layout of v_mfma_scale_f32_16x16x128_f8f6f4 exactly, ops.skinny_linear_mxfp4_a8 within the f64 bound
of _skinny_cases.reference on the two dequantised matrices (no outliers), row invariance and the SwiGLU epilogue bit for
bit, refusals, and linear="skinny-mxfp4-a8" against its graph, its speculative loop and the cost of 4-bit weights.

The bound: an e2m1 code times an e4m3 code times two powers of two is exact in f32, so what the kernel adds to the exact
product of the dequantised matrices is a K-term f32 sum in some order and one bf16 rounding, which is the bound of
_skinny_cases.reference (it also allows one roundoff per product, which is not used here)."""
import copy

import pytest
import torch

import _generate_cases as gc
import _refs
import _skinny_cases as sc
import _spec_cases as sp
from _skinny_mfma_cases import prompts
from dtg import ops
from dtg.models import Mxfp4DecodeWeights, Speculative, build_model
from dtg.models.decode_graph import GraphedDecode
from dtg.models.generation import KVCache, decode_step, generate, prefill

pytestmark = pytest.mark.gpu

W, U = 8, 2  # the kernel's waves per workgroup and units (128 of K) per pass (DTG_MXFP4_A8_UNROLL)
# one block; one unit and a 17th row; a 17th column, one full pass + one block; partial both ways; two full passes; long K
SHAPES = [(1, 1, 32), (17, 16, 128), (16, 17, 128 * W * U + 32), (33, 67, 4128), (64, 130, 4096), (48, 2, 14336)]
raw = torch.ops.dtg.skinny_linear_mxfp4_a8


def quantized(M, N, K, dev, bias=True, seed=0):
    x, w, b = sc.inputs(M, N, K, dev, bias, seed)
    return (x, *ops.quantize_mxfp8_rows(x), *ops.quantize_mxfp4_rows(w), b)


@pytest.mark.parametrize("shape", [(1, 32), (17, 160), (64, 4128), (17, 160, "strided")], ids=lambda s: "x".join(map(str, s)))
def test_quantizer_bitwise(cuda, shape):
    """Blocks spanning 2^-20..2^20; the last blocks are all zero, amax = 448 * 2^3 and 224 * 2^-5 (the two ends of the
    scale's interval) and one value below the scale floor."""
    M, K = shape[:2]
    g = torch.Generator().manual_seed(M + K)
    nb = M * K // 32
    xb = torch.randn(nb, 32, generator=g) * torch.exp2(torch.randint(-20, 21, (nb, 1), generator=g).float())
    planted = torch.randn(4, 32, generator=g) * 0.01
    planted[0] = 0.0
    planted[1, 5], planted[2, 31], planted[3] = 448.0 * 8, -224.0 / 32, 0.0
    planted[3, 7] = 2.0 ** -110
    if nb > 1:
        k = min(4, nb - 1)
        xb[nb - k:] = planted[:k]
    x = xb.reshape(M, K).to(torch.bfloat16)
    want_q, want_s = ops.quantize_fp8_rows(x.reshape(-1, 32), pow2=True)
    xd = x.to(cuda)
    if len(shape) == 3:  # a window of a NaN buffer: row stride K + 24
        buf = torch.full((M + 4, K + 24), float("nan"), dtype=x.dtype, device=cuda)
        buf[2:2 + M, 8:8 + K] = xd
        xd = buf[2:2 + M, 8:8 + K]
    xq, xs = ops.quantize_mxfp8_rows(xd)
    assert xq.dtype == torch.float8_e4m3fn and xq.shape == (M, K) and xq.is_contiguous()
    assert xs.dtype == torch.uint8 and xs.shape == (M, K // 32) and xs.is_contiguous()
    assert torch.equal(xs.cpu().reshape(-1).int(), want_s.view(torch.int32) >> 23) and xs.min() > 0 and xs.max() < 255
    got, want = xq.cpu().view(torch.uint8).reshape(-1, 32), want_q.view(torch.uint8)
    assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()
    assert torch.equal(ops.dequantize_mxfp8(xq, xs).cpu(), (want_q.float() * want_s[:, None]).reshape(M, K).to(torch.bfloat16))


@pytest.mark.parametrize("third", [0, 1, 2])
def test_layout_exact(cuda, third):
    """K = 160: a full unit and one block.  Weight codes differ within and across blocks, every block has its own scale.
    xq row m is the one code 1.5 at k_m, with a scale byte per (row, block), so y[m, n] is the one product
    1.5 * 2^(xs[m, k_m / 32] - 127) * deq[n, k_m], exact in bf16: a permuted k or a swapped scale shows."""
    N, K = 18, 160
    n, k = torch.arange(N)[:, None], torch.arange(K)[None]
    codes = ((k % 32 + 5 * (k % 32 // 16) + n) % 16).to(torch.uint8)
    wq = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(cuda)
    scales = (118 + 3 * torch.arange(K // 32)[None] + n % 3 + 7 * (n // 9)).to(torch.uint8).to(cuda)
    at = torch.randperm(K, generator=torch.Generator().manual_seed(6))[(torch.arange(64) + 64 * third) % K]  # 3 runs: all 160 k
    xq = torch.zeros(64, K, dtype=torch.uint8)
    xq[torch.arange(64), at] = 0x3C  # e4m3 1.5
    xs = (124 + torch.arange(K // 32)[None] + torch.arange(64)[:, None] % 3).to(torch.uint8)
    xval = 1.5 * torch.exp2(xs[torch.arange(64), at // 32].float() - 127)
    want = (ops.dequantize_mxfp4(wq, scales)[:, at.to(cuda)].t().float() * xval.to(cuda)[:, None]).to(torch.bfloat16)
    got = raw(xq.view(torch.float8_e4m3fn).to(cuda), xs.to(cuda), wq, scales, None, 0)
    assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(33, 67, 4128, "strided")], ids=lambda s: "x".join(map(str, s)))
def test_accuracy(cuda, shape, bias):
    M, N, K = shape[:3]
    _, xq, xs, wq, scales, b = quantized(M, N, K, cuda, bias)
    if len(shape) == 4:  # rows of a wider buffer: row stride K + 16
        xq = torch.cat([xq.view(torch.uint8), torch.zeros(M, 16, dtype=torch.uint8, device=cuda)], 1)[:, :K].view(xq.dtype)
    out = raw(xq, xs, wq, scales, b, 0)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _refs.assert_within(out, *sc.reference(ops.dequantize_mxfp8(xq, xs), ops.dequantize_mxfp4(wq, scales), b),
                        f"skinny_linear_mxfp4_a8 {shape}{' +b' if bias else ''}")


@pytest.mark.parametrize("K", [160, 4128])
def test_row_invariance(cuda, K):
    """Through the bf16 wrapper: the quantiser's rows are held to it too."""
    x, _, _, wq, scales, b = quantized(64, 37, K, cuda, seed=2)
    full = ops.skinny_linear_mxfp4_a8(x, wq, scales, b)
    assert torch.equal(full, ops.skinny_linear_mxfp4_a8(x, wq, scales, b)), "two identical calls differ"
    for m in (0, 15, 16, 63):
        assert torch.equal(ops.skinny_linear_mxfp4_a8(x[m:m + 1], wq, scales, b)[0], full[m]), f"row {m} alone differs from the batch"
    assert torch.equal(ops.skinny_linear_mxfp4_a8(x[13:35], wq, scales, b), full[13:35])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 32), (37, 134, 288), (64, 1024, 512)], ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(cuda, shape, bias):
    x, _, _, wq, scales, b = quantized(*shape, cuda, bias, seed=1)
    fused = ops.skinny_linear_mxfp4_a8(x, wq, scales, b, act="swiglu")
    two = sc.swiglu_any_width(ops.skinny_linear_mxfp4_a8(x, wq, scales, b))
    assert fused.shape == (shape[0], shape[1] // 2) and torch.equal(fused, two), (fused != two).nonzero()[:4].tolist()


def raw_refusals(dev):
    _, xq, xs, wq, s, b = quantized(4, 10, 64, dev)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)  # noqa: E731
    return {
        "M = 0": lambda: raw(xq[:0], xs[:0], wq, s, b, 0),
        "M = 65": lambda: raw(z(65, 64), xs[:1].expand(65, 2).contiguous(), wq, s, b, 0),
        "K % 32": lambda: raw(xq[:, :48].contiguous(), xs[:, :1].contiguous(), wq[:, :24].contiguous(), s[:, :1].contiguous(), b, 0),
        "bf16 xq": lambda: raw(xq.to(torch.bfloat16), xs, wq, s, b, 0),
        "xs shape": lambda: raw(xq, xs[:, :1].contiguous(), wq, s, b, 0),
        "wq width": lambda: raw(xq, xs, torch.cat([wq, wq], 1), s, b, 0),
        "misaligned xq": lambda: raw(z(4, 80)[:, 1:65], xs, wq, s, b, 0),
        "odd N with act": lambda: raw(xq, xs, wq[:9].contiguous(), s[:9].contiguous(), None, 1),
        "bias length": lambda: raw(xq, xs, wq, s, b[:9].contiguous(), 0),
        "act = 2": lambda: raw(xq, xs, wq, s, b, 2),
    }


@pytest.mark.parametrize("what", list(raw_refusals("cpu")))
def test_refusals(cuda, what):
    with pytest.raises(RuntimeError, match="dtg: skinny_linear_mxfp4_a8: "):
        raw_refusals(cuda)[what]()


def test_graph_24_rows_and_speculative_32_rows_return_the_eager_ids(cuda):
    model, _ = gc.models("llama", cuda)
    kw = dict(s_max=256, linear="skinny-mxfp4-a8", mxfp4=Mxfp4DecodeWeights(model))
    gd = GraphedDecode(model, 24, **kw)
    graph = generate(model, prompts(24), 12, decode=gd, **kw)
    eager = generate(model, prompts(24), 12, decode="eager", bucketed=True, **kw)
    assert gd.replays >= 8 and gd.mxfp4 is kw["mxfp4"] and all(torch.equal(g, e) for g, e in zip(graph, eager)), (graph, eager)
    plain = generate(model, prompts(8), 16, bucketed=True, **kw)
    spec = Speculative(sp.Oracle(torch.stack(plain), prompts(8), wrong_at=1), k=4)  # its second draft is wrong
    got = generate(model, prompts(8), 16, speculate=spec, **kw)
    assert all(torch.equal(g, p) for g, p in zip(got, plain)) and 0 < spec.stats["accepted"] < spec.stats["proposed"], (got, plain)


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_teacher_forced_within_the_cost_of_4_bit_weights(cuda, kind):
    """e_a8: prefill + decode_step(linear="skinny-mxfp4-a8") against the f32 upcast of the dequantised twin.  e_w4: that f32
    twin against the f32 unquantised model on the same positions, what 4-bit weights already cost.  No margin: e4m3's
    relative step is 2^-4 against e2m1's 2^-2."""
    model, _ = gc.models(kind, cuda)
    mx = Mxfp4DecodeWeights(model)
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for name in mx.names():
            twin.get_submodule(name).weight.copy_(mx.dequantized(name))
    ref, full = (build_model(gc.config(kind), dtype=torch.float32, init=False) for _ in range(2))
    ref.load_state_dict({k: v.float().cpu() for k, v in twin.state_dict().items()})
    full.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    seqs, pre = gc.sequences(kind), [gc.PREFIX, gc.PREFIX - gc.SHORTER]
    cache = KVCache(model.config, 2, gc.SEQ, device=cuda)
    got = [prefill(model, [s[:p] for s, p in zip(seqs, pre)], cache, mxfp4=mx).float().cpu()]
    for t in range(gc.STEPS):
        tok = torch.stack([s[p + t] for s, p in zip(seqs, pre)])
        got.append(decode_step(model, tok, cache, linear="skinny-mxfp4-a8", mxfp4=mx).float().cpu())
    e_w4 = e_a8 = 0.0
    for i, (s, p) in enumerate(zip(seqs, pre)):
        r = gc.full_logits(ref.eval(), s)[p - 1: p + gc.STEPS]
        e_w4 = max(e_w4, (gc.full_logits(full.eval(), s)[p - 1: p + gc.STEPS] - r).abs().max().item())
        e_a8 = max(e_a8, (torch.stack([g[i] for g in got]) - r).abs().max().item())
    print(f"[mxfp4-a8-decode] {kind} teacher-forced: e_a8 {e_a8:.5f}, e_w4 {e_w4:.5f}")
    assert 0 < e_a8 <= e_w4, f"{kind}: skinny-mxfp4-a8 error {e_a8} against the f32 twin > the 4-bit weights' own {e_w4}"
