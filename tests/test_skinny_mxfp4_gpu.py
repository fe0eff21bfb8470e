"""ops.skinny_linear_mxfp4 on the gfx950 kernel (csrc/kernels/skinny_mfma.hip) and linear="skinny-mxfp4": the operand
layout exactly, the f64 bound of _skinny_cases.reference on the dequantised weights (no outliers), row invariance and
the SwiGLU epilogue bit for bit, unread memory, refusals, and the decode mode against its dequantised twin."""
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

W, U = 8, 2  # the kernel's waves per workgroup and super-slabs (128 of K) per pass
# one block; one super-slab and a 17th row; a 17th column, one full pass + one block; partial both ways; two full passes; long K
SHAPES = [(1, 1, 32), (17, 16, 128), (16, 17, 128 * W * U + 32), (33, 67, 4128), (64, 130, 4096), (48, 2, 14336)]


def quantized(M, N, K, dev, bias=True, seed=0):
    x, w, b = sc.inputs(M, N, K, dev, bias, seed)
    return (x, *ops.quantize_mxfp4_rows(w), b)


@pytest.mark.parametrize("third", [0, 1, 2])
def test_layout_exact(cuda, third):
    """K = 160: a full super-slab and one block.  Each half of a block holds 16 different codes, the halves differ, every
    block has its own scale.  x row m is one-hot at k_m, so y[m, n] is the one product 1 * deq[n, k_m], exact in bf16."""
    N, K = 18, 160
    n, k = torch.arange(N)[:, None], torch.arange(K)[None]
    codes = ((k % 32 + 5 * (k % 32 // 16) + n) % 16).to(torch.uint8)
    wq = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(cuda)
    scales = (118 + 3 * torch.arange(K // 32)[None] + n % 3 + 7 * (n // 9)).to(torch.uint8).to(cuda)
    at = torch.randperm(K, generator=torch.Generator().manual_seed(6))[(torch.arange(64) + 64 * third) % K]  # 3 runs: all 160 k
    x = torch.zeros(64, K, dtype=torch.bfloat16, device=cuda)
    x[torch.arange(64), at] = 1.0
    want = ops.dequantize_mxfp4(wq, scales)[:, at.to(cuda)].t()
    got = ops.skinny_linear_mxfp4(x, wq, scales)
    assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(33, 67, 4128, "strided")], ids=lambda s: "x".join(map(str, s)))
def test_accuracy(cuda, shape, bias):
    M, N, K = shape[:3]
    x, wq, scales, b = quantized(M, N, K, cuda, bias)
    if len(shape) == 4:  # rows of a wider buffer: row stride K + 16
        x = torch.cat([x, torch.zeros(M, 16, dtype=x.dtype, device=cuda)], 1)[:, :K]
    out = ops.skinny_linear_mxfp4(x, wq, scales, b)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _refs.assert_within(out, *sc.reference(x, ops.dequantize_mxfp4(wq, scales), b), f"skinny_linear_mxfp4 {shape}{' +b' if bias else ''}")


@pytest.mark.parametrize("K", [160, 4128])
def test_row_invariance(cuda, K):
    x, wq, scales, b = quantized(64, 37, K, cuda, seed=2)
    full = ops.skinny_linear_mxfp4(x, wq, scales, b)
    assert torch.equal(full, ops.skinny_linear_mxfp4(x, wq, scales, b)), "two identical calls differ"
    for m in (0, 15, 16, 63):
        assert torch.equal(ops.skinny_linear_mxfp4(x[m:m + 1], wq, scales, b)[0], full[m]), f"row {m} alone differs from the batch"
    assert torch.equal(ops.skinny_linear_mxfp4(x[13:35], wq, scales, b), full[13:35])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 32), (37, 134, 288), (64, 1024, 512)], ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(cuda, shape, bias):
    x, wq, scales, b = quantized(*shape, cuda, bias, seed=1)
    fused = ops.skinny_linear_mxfp4(x, wq, scales, b, act="swiglu")
    two = sc.swiglu_any_width(ops.skinny_linear_mxfp4(x, wq, scales, b))
    assert fused.shape == (shape[0], shape[1] // 2) and torch.equal(fused, two), (fused != two).nonzero()[:4].tolist()


def test_unread_rows_stay_unread(cuda):
    M, N, K = 21, 21, 288
    x, wq, scales, b = quantized(M, N, K, cuda, seed=3)
    buf = torch.full((M + 4, K + 24), float("nan"), dtype=x.dtype, device=cuda)
    buf[2:2 + M, 8:8 + K] = x
    got = ops.skinny_linear_mxfp4(buf[2:2 + M, 8:8 + K], wq, scales, b)
    assert torch.isfinite(got.float()).all() and torch.equal(got, ops.skinny_linear_mxfp4(x, wq, scales, b))


def raw_refusals(dev):
    (x, wq, s, b), op, z = quantized(4, 10, 64, dev), torch.ops.dtg.skinny_linear_mxfp4, lambda *sh: torch.zeros(*sh, dtype=torch.bfloat16, device=dev)
    return {
        "M = 0": lambda: op(x[:0], wq, s, b, 0),
        "M = 65": lambda: op(z(65, 64), wq, s, b, 0),
        "K % 32": lambda: op(x[:, :48].contiguous(), wq[:, :24].contiguous(), s[:, :1].contiguous(), b, 0),
        "f32 x": lambda: op(x.float(), wq, s, b, 0),
        "int8 wq": lambda: op(x, wq.view(torch.int8), s, b, 0),
        "wq width": lambda: op(x, torch.cat([wq, wq], 1), s, b, 0),
        "scales shape": lambda: op(x, wq, s[:, :1].contiguous(), b, 0),
        "misaligned x": lambda: op(z(4, 72)[:, 1:65], wq, s, b, 0),
        "odd N with act": lambda: op(x, wq[:9].contiguous(), s[:9].contiguous(), None, 1),
        "bias length": lambda: op(x, wq, s, b[:9].contiguous(), 0),
        "act = 2": lambda: op(x, wq, s, b, 2),
    }


@pytest.mark.parametrize("what", list(raw_refusals("cpu")))
def test_refusals(cuda, what):
    with pytest.raises(RuntimeError, match="dtg: skinny_linear_mxfp4: "):
        raw_refusals(cuda)[what]()


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_teacher_forced_against_the_dequantised_twin(cuda, kind):
    """The twin is the bf16 model with dequantized(name) for matrices; e_full its own error against its f32 upcast."""
    model, _ = gc.models(kind, cuda)
    mx = Mxfp4DecodeWeights(model)
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for name in mx.names():
            twin.get_submodule(name).weight.copy_(mx.dequantized(name))
    ref = build_model(gc.config(kind), dtype=torch.float32, init=False)
    ref.load_state_dict({k: v.float().cpu() for k, v in twin.state_dict().items()})
    seqs, pre = gc.sequences(kind), [gc.PREFIX, gc.PREFIX - gc.SHORTER]
    cache = KVCache(model.config, 2, gc.SEQ, device=cuda)
    got = [prefill(model, [s[:p] for s, p in zip(seqs, pre)], cache, mxfp4=mx).float().cpu()]
    for t in range(gc.STEPS):
        tok = torch.stack([s[p + t] for s, p in zip(seqs, pre)])
        got.append(decode_step(model, tok, cache, linear="skinny-mxfp4", mxfp4=mx).float().cpu())
    e_full = e_cached = 0.0
    for i, (s, p) in enumerate(zip(seqs, pre)):
        r = gc.full_logits(ref.eval(), s)[p - 1: p + gc.STEPS]
        e_full = max(e_full, (gc.full_logits(twin.eval(), s)[p - 1: p + gc.STEPS] - r).abs().max().item())
        e_cached = max(e_cached, (torch.stack([g[i] for g in got]) - r).abs().max().item())
    print(f"[mxfp4-decode] {kind} teacher-forced: e_full {e_full:.5f}, e_cached {e_cached:.5f} (allowed {2 * e_full:.5f})")
    assert 0 < e_cached <= 2 * e_full, f"{kind}: skinny-mxfp4 cached path error {e_cached} > 2 * {e_full}"


def test_graph_24_rows_and_speculative_32_rows_return_the_eager_ids(cuda):
    model, _ = gc.models("llama", cuda)
    kw = dict(s_max=256, linear="skinny-mxfp4", mxfp4=Mxfp4DecodeWeights(model))
    gd = GraphedDecode(model, 24, **kw)
    graph = generate(model, prompts(24), 12, decode=gd, **kw)
    eager = generate(model, prompts(24), 12, decode="eager", bucketed=True, **kw)
    assert gd.replays >= 8 and gd.mxfp4 is kw["mxfp4"] and all(torch.equal(g, e) for g, e in zip(graph, eager)), (graph, eager)
    plain = generate(model, prompts(8), 16, bucketed=True, **kw)
    spec = Speculative(sp.Oracle(torch.stack(plain), prompts(8), wrong_at=1), k=4)  # its second draft is wrong
    got = generate(model, prompts(8), 16, speculate=spec, **kw)
    assert all(torch.equal(g, p) for g, p in zip(got, plain)) and 0 < spec.stats["accepted"] < spec.stats["proposed"], (got, plain)
