"""W4A8 on the CPU: the operator pair against the f64 bound of _skinny_cases.reference on the two dequantised matrices,
the MXFP8 round trip, and the limits and errors of linear="skinny-mxfp4-a8"."""
import pytest
import torch

import _generate_cases as gc
import _refs
import _skinny_cases as sc
import dtg
from dtg import ops
from dtg.models.generation import KVCache, decode_step, generate, prefill
from _skinny_mfma_cases import prompts


@pytest.mark.parametrize("shape", [(17, 16, 160), (64, 67, 4128)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_operator(shape):
    x, w, b = sc.inputs(*shape, "cpu")
    (xq, xs), (wq, scales) = ops.quantize_mxfp8_rows(x), ops.quantize_mxfp4_rows(w)
    out = ops.skinny_linear_mxfp4_a8(x, wq, scales, b)
    assert torch.equal(out, torch.ops.dtg.skinny_linear_mxfp4_a8(xq, xs, wq, scales, b, 0))
    _refs.assert_within(out, *sc.reference(ops.dequantize_mxfp8(xq, xs), ops.dequantize_mxfp4(wq, scales), b),
                        f"skinny_linear_mxfp4_a8 cpu {shape}")


def test_mxfp8_round_trip():
    """Quantising the dequantised matrix returns the same matrix, and the same codes and scale bytes wherever the block's
    largest code lies inside (224, 448]; one that was rounded down to 224 is renormalised (the codes doubled)."""
    x = (torch.randn(9, 160, generator=torch.Generator().manual_seed(8)) * torch.logspace(-6, 6, 9, base=2.0)[:, None]).to(torch.bfloat16)
    x[3, 32:64] = 0.0
    xq, xs = ops.quantize_mxfp8_rows(x)
    assert xq.dtype == torch.float8_e4m3fn and xs.dtype == torch.uint8 and xs[3, 1] == 127 and 0 < xs.min() and xs.max() < 255
    deq = ops.dequantize_mxfp8(xq, xs)
    assert deq.dtype == torch.bfloat16 and (deq.float() - x.float()).abs().max() <= x.float().abs().max() / 16
    xq2, xs2 = ops.quantize_mxfp8_rows(deq)
    assert torch.equal(ops.dequantize_mxfp8(xq2, xs2), deq)
    kept = (xq.float().abs().reshape(9, 5, 32).amax(-1) > 224) | (xs == 127)
    assert kept.sum() > 30 and torch.equal(xs2[kept], xs[kept])
    assert torch.equal(xq2.view(torch.uint8).reshape(9, 5, 32)[kept], xq.view(torch.uint8).reshape(9, 5, 32)[kept])


def test_mode_limits_and_argument_errors():
    model, _ = gc.models("llama", "cpu")
    mx, fp8 = dtg.Mxfp4DecodeWeights(model), dtg.Fp8DecodeWeights(model)
    one = [torch.arange(3)]  # mxfp4=None quantises for the call
    a8 = generate(model, one, 4, linear="skinny-mxfp4-a8", mxfp4=mx)[0]
    assert len(a8) == 4 and torch.equal(a8, generate(model, one, 4, linear="skinny-mxfp4-a8")[0])
    with pytest.raises(ValueError, match='linear="skinny-mxfp4-a8" decodes at most 64 sequences per step, got 65'):
        generate(model, prompts(65), 2, linear="skinny-mxfp4-a8", mxfp4=mx)
    with pytest.raises(ValueError, match="skinny-fp8"):
        generate(model, one, 2, linear="skinny-mxfp4-a8", fp8=fp8)
    with pytest.raises(ValueError, match="Mxfp4DecodeWeights"):
        generate(model, one, 2, linear="skinny-mxfp4-a8", mxfp4=fp8)
    cache = KVCache(model.config, 2, 8, device="cpu")
    prefill(model, [torch.arange(3), torch.arange(2)], cache, mxfp4=mx)
    with pytest.raises(ValueError, match="mxfp4=Mxfp4DecodeWeights"):  # a step does not quantise for itself
        decode_step(model, torch.zeros(2, dtype=torch.long), cache, linear="skinny-mxfp4-a8")
    assert decode_step(model, torch.zeros(2, dtype=torch.long), cache, linear="skinny-mxfp4-a8", mxfp4=mx).shape[0] == 2
