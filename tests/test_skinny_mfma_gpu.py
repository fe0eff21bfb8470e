"""ops.skinny_linear_mfma on the gfx950 kernel (csrc/kernels/skinny_mfma.hip) and linear="skinny-mfma": the f64
bound of _skinny_cases.reference (derived for any order of an f32 K-term sum, no outliers), row invariance and
the SwiGLU epilogue bit for bit, unread memory, refusals, and the two loops that need more than 16 rows."""
import pytest
import torch

import _generate_cases as gc
import _refs
import _skinny_cases as sc
import _spec_cases as sp
from _skinny_mfma_cases import SHAPES, prompts, raw_refusals
from dtg import ops
from dtg.models import Speculative
from dtg.models.decode_graph import GraphedDecode
from dtg.models.generation import generate

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(33, 67, 4128, "strided")], ids=lambda s: "x".join(map(str, s)))
def test_accuracy(cuda, shape, bias):
    M, N, K = shape[:3]
    x, w, b = sc.inputs(M, N, K, cuda, bias)
    if len(shape) == 4:  # rows of a wider buffer: row stride K + 16
        x = torch.cat([x, torch.zeros(M, 16, dtype=x.dtype, device=cuda)], 1)[:, :K]
        assert x.stride(0) == K + 16
    out = ops.skinny_linear_mfma(x, w, b)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _refs.assert_within(out, *sc.reference(x, w, b), f"skinny_linear_mfma {shape}{' +b' if bias else ''}")


@pytest.mark.parametrize("K", [288, 4128])
def test_row_invariance(cuda, K):
    x, w, b = sc.inputs(64, 37, K, cuda, True, seed=2)
    full = ops.skinny_linear_mfma(x, w, b)
    assert torch.equal(full, ops.skinny_linear_mfma(x, w, b)), "two identical calls differ"
    for m in (0, 15, 16, 63):
        assert torch.equal(ops.skinny_linear_mfma(x[m:m + 1], w, b)[0], full[m]), f"row {m} alone differs from the batch"
    assert torch.equal(ops.skinny_linear_mfma(x[13:35], w, b), full[13:35])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 32), (37, 134, 288), (64, 1024, 512)], ids=lambda s: "x".join(map(str, s)))
def test_swiglu_epilogue_bitwise(cuda, shape, bias):
    x, w, b = sc.inputs(*shape, cuda, bias, seed=1)
    fused = ops.skinny_linear_mfma(x, w, b, act="swiglu")
    two = sc.swiglu_any_width(ops.skinny_linear_mfma(x, w, b))
    assert fused.shape == two.shape == (shape[0], shape[1] // 2)
    assert torch.equal(fused, two), f"epilogue differs from swiglu(skinny_linear_mfma) at {(fused != two).nonzero()[:4].tolist()}"


def test_unread_rows_stay_unread(cuda):
    M, N, K = 21, 21, 288
    x, w, b = sc.inputs(M, N, K, cuda, True, seed=3)
    buf = torch.full((M + 4, K + 24), float("nan"), dtype=x.dtype, device=cuda)
    buf[2:2 + M, 8:8 + K] = x
    got = ops.skinny_linear_mfma(buf[2:2 + M, 8:8 + K], w, b)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, ops.skinny_linear_mfma(x, w, b))


@pytest.mark.parametrize("what", list(raw_refusals("cpu")))
def test_refusals(cuda, what):
    with pytest.raises(RuntimeError, match="dtg: "):
        raw_refusals(cuda)[what]()


def test_speculative_32_rows_returns_the_plain_loops_ids(cuda):
    """8 prompts x k = 4: one verify pass is 32 rows.  The drafter always proposes and its second draft is wrong."""
    model, _ = gc.models("llama", cuda)
    kw = dict(s_max=256, linear="skinny-mfma")
    plain = generate(model, prompts(8), 16, bucketed=True, **kw)
    spec = Speculative(sp.Oracle(torch.stack(plain), prompts(8), wrong_at=1), k=4)
    got = generate(model, prompts(8), 16, speculate=spec, **kw)
    assert all(torch.equal(g, p) for g, p in zip(got, plain)), (got, plain)
    assert 0 < spec.stats["accepted"] < spec.stats["proposed"], spec.stats


def test_graphed_decode_24_rows_returns_the_eager_ids(cuda):
    model, _ = gc.models("llama", cuda)
    kw = dict(s_max=256, linear="skinny-mfma")
    gd = GraphedDecode(model, 24, **kw)
    graph = generate(model, prompts(24), 12, decode=gd, **kw)
    eager = generate(model, prompts(24), 12, decode="eager", bucketed=True, **kw)
    assert gd.replays >= 8
    assert all(torch.equal(g, e) for g, e in zip(graph, eager)), (graph, eager)
