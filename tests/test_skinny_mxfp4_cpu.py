"""MXFP4 on the CPU: the quantiser against a plain f64 form of the OCP MX v1.0 rule written here, the CPU operator
against the f64 bound of _skinny_cases.reference on the dequantised weights, the limits and errors of the mode."""
import pytest
import torch

import _generate_cases as gc
import _refs
import _skinny_cases as sc
import dtg
from dtg import ops
from dtg.models.generation import KVCache, decode_step, generate, prefill
from _skinny_mfma_cases import prompts

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def ref_quantize(w):
    """(codes [N, K], k [N, K / 32]) in f64; of two nearest grid values the one with the even code, saturating at 6."""
    v = w.double().reshape(w.shape[0], -1, 32)
    amax = v.abs().amax(-1)
    k = torch.where(amax > 0, torch.floor(torch.log2(amax)) - 2, torch.full_like(amax, -100.0)).clamp(-100, 125)
    q = v / 2.0 ** k[..., None]
    d = (q.abs().clamp(max=6.0)[..., None] - GRID).abs()
    lo, hi = d.argmin(-1), 7 - d.flip(-1).argmin(-1)  # the first and the last nearest grid value
    codes = torch.where(lo % 2 == 0, lo, hi) + 8 * torch.signbit(q)
    return codes.reshape(w.shape).to(torch.uint8), k.long()


def unpack(wq):
    return torch.stack([wq & 15, wq >> 4], -1).reshape(wq.shape[0], -1)


BLOCKS = {  # name -> (leading elements of a 32-element block, zero after them; expected k; expected leading codes)
    "zeros": ([0.0], -100, [0]),
    "amax a power of two": ([4.0, -2.0, 1.0, 0.5], 0, [6, 12, 2, 1]),
    "ties to even": ([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, -3.5], 0, [6, 0, 2, 2, 4, 4, 14]),
    "saturation": ([7.5, -7.0, 6.5, 5.0], 0, [7, 15, 7, 6]),
    "floor of the scale": ([2.0 ** -110], -100, [0]),
}


@pytest.mark.parametrize("what", list(BLOCKS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantizer_block(what, dtype):
    lead, k, codes = BLOCKS[what]
    w = torch.zeros(1, 32, dtype=dtype)
    w[0, : len(lead)] = torch.tensor(lead, dtype=dtype)
    wq, scales = ops.quantize_mxfp4_rows(w)
    assert wq.dtype == scales.dtype == torch.uint8 and wq.shape == (1, 16) and scales.shape == (1, 1)
    ref_codes, ref_k = ref_quantize(w)
    assert torch.equal(unpack(wq), ref_codes) and ref_k.item() == k == scales.item() - 127
    assert ref_codes[0, : len(codes)].tolist() == codes


def test_quantizer_random_matches_the_f64_rule():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(5, 96, generator=g) * torch.tensor([1e-3, 0.02, 1.0, 37.0, 5e4])[:, None]
    wq, scales = ops.quantize_mxfp4_rows(w)
    codes, k = ref_quantize(w)
    assert torch.equal(scales.long() - 127, k) and torch.equal(unpack(wq), codes)
    assert torch.equal(wq & 15, codes[:, 0::2]) and torch.equal(wq >> 4, codes[:, 1::2])  # element 2 j: low nibble
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_mxfp4_rows(torch.full((1, 32), float("inf")))


def test_dequantize_is_exact():
    table, wq = GRID.tolist() + (-GRID).tolist(), (torch.arange(16, dtype=torch.uint8) * 17).reshape(1, 16)  # byte j: code j twice
    got = ops.dequantize_mxfp4(wq, torch.tensor([[127]], dtype=torch.uint8))
    assert got.dtype == torch.bfloat16 and got[0, 0::2].tolist() == table and got[0, 1::2].tolist() == table
    g = torch.Generator().manual_seed(5)
    wq = torch.randint(0, 256, (7, 64), generator=g, dtype=torch.uint8)
    scales = torch.randint(27, 253, (7, 4), generator=g, dtype=torch.uint8)
    w = ops.dequantize_mxfp4(wq, scales)  # a matrix on the grid, the sign of its zeros included
    again = ops.dequantize_mxfp4(*ops.quantize_mxfp4_rows(w))
    assert torch.equal(again.view(torch.int16), w.view(torch.int16))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 32), (17, 16, 128), (16, 18, 4128), (64, 67, 160)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_operator(shape, bias):
    x, w, b = sc.inputs(*shape, "cpu", bias)
    wq, scales = ops.quantize_mxfp4_rows(w)
    out = ops.skinny_linear_mxfp4(x, wq, scales, b)
    _refs.assert_within(out, *sc.reference(x, ops.dequantize_mxfp4(wq, scales), b), f"skinny_linear_mxfp4 cpu {shape}")
    if shape[1] % 2 == 0:
        assert torch.equal(ops.skinny_linear_mxfp4(x, wq, scales, b, act="swiglu"), sc.swiglu_any_width(out))


def test_limits_and_argument_errors():
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    wq, scales = ops.quantize_mxfp4_rows(z(10, 64))
    assert ops.skinny_linear_mxfp4(z(64, 64), wq, scales).shape == (64, 10)
    with pytest.raises(RuntimeError, match="dtg: skinny_linear_mxfp4: x must be .* 1 <= M <= 64"):
        torch.ops.dtg.skinny_linear_mxfp4(z(65, 64), wq, scales, None, 0)
    with pytest.raises(RuntimeError, match="dtg: skinny_linear_mxfp4: K must be a multiple of 32"):
        torch.ops.dtg.skinny_linear_mxfp4(z(4, 48), wq[:, :24].contiguous(), scales[:, :1].contiguous(), None, 0)
    model, _ = gc.models("llama", "cpu")
    mx, fp8 = dtg.Mxfp4DecodeWeights(model), dtg.Fp8DecodeWeights(model)
    assert [len(o) for o in generate(model, prompts(17), 2, linear="skinny-mxfp4", mxfp4=mx)] == [2] * 17
    with pytest.raises(ValueError, match='linear="skinny-mxfp4" decodes at most 64 sequences per step, got 65'):
        generate(model, prompts(65), 2, linear="skinny-mxfp4", mxfp4=mx)
    one = [torch.arange(3)]  # mxfp4=None quantises for the call
    assert torch.equal(generate(model, one, 4, linear="skinny-mxfp4")[0], generate(model, one, 4, linear="skinny-mxfp4", mxfp4=mx)[0])
    for kw, message in ((dict(linear="skinny-mxfp4", mxfp4=mx, fp8=fp8), "both"),
                        (dict(linear="skinny-mxfp4", fp8=fp8), "skinny-fp8"),
                        (dict(linear="skinny-fp8", mxfp4=mx), "skinny-mxfp4"),
                        (dict(linear="blas", mxfp4=mx), "skinny-mxfp4"),
                        (dict(linear="skinny-mxfp4", mxfp4=fp8), "Mxfp4DecodeWeights")):
        with pytest.raises(ValueError, match=message):
            generate(model, one, 2, **kw)
    cache = KVCache(model.config, 2, 8, device="cpu")
    prefill(model, [torch.arange(3), torch.arange(2)], cache, mxfp4=mx)
    with pytest.raises(ValueError, match="mxfp4=Mxfp4DecodeWeights"):  # a step does not quantise for itself
        decode_step(model, torch.zeros(2, dtype=torch.long), cache, linear="skinny-mxfp4")
