"""Cases and checks of the FP8 (e4m3) KV cache: the operators kv_cache_append_fp8_ and decode_attn_fp8
(csrc/kernels/decode_attn.hip, dtg.ops._cpu), the k_scale / v_scale arguments of the public ops, and
KVCache(kv_cache="fp8") through prefill, decode_step, generate, the captured loop and speculative decoding.
Shared by test_kv_fp8_cpu.py and test_kv_fp8_gpu.py.

The format has an exact oracle.  A key vector's scale is the power of two that puts its amax into (224, 448]
(ops.quantize_fp8_rows(pow2=True) of the D-vector), so float(code) * scale is exactly a bf16 value and the FP8
cache is exactly some bf16 cache.  Hence
  * the append is compared bit for bit with quantize_fp8_rows of the (roped) vectors;
  * the attention on (codes, scales) is held to the float64 reference and bound of tests/_decode_cases.py,
    recomputed on the dequantised values with the same formulas (widening e4m3 and multiplying by a power of two
    add no error), and compared bit for bit with the bf16 operator on the dequantised cache;
  * a model run on an FP8 cache is compared with the same decoder stack around an attention built here from
    the bf16 ops alone, which fake-quantises what it appends.
Cases, inputs and models are those of _decode_cases, _decode_multi_cases and _generate_cases, imported.  Nothing
here comes from a run of the code under test."""
import functools

import pytest
import torch

import _decode_cases as C
import _decode_graph_cases as dc
import _decode_multi_cases as M
import _generate_cases as gc
import _spec_cases as sc
from _refs import K, U, assert_within, f64
from dtg import ops
from dtg.models import Speculative
from dtg.models import generation as G
from dtg.models.generation import KVCache, decode_bucket, decode_step, generate, prefill

FP8 = torch.float8_e4m3fn
SENT_CODE = 0x4B          # the byte the append tests fill the caches with
SENT_SCALE = 12345.0      # ... and the scales
NAN_CODE = 0x7F


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def quantize_vectors(x):
    """x bf16 [..., D] (CPU) -> (codes float8 [..., D], scale f32 [...]): quantize_fp8_rows per D-vector."""
    codes, scale = ops.quantize_fp8_rows(x.reshape(-1, x.shape[-1]))
    return codes.reshape(x.shape), scale.reshape(x.shape[:-1])


def dequantize(codes, scale, dtype=torch.bfloat16):
    return (codes.float() * scale[..., None]).to(dtype)


def quantize_cache(kc):
    """A bf16 cache [rows, nkv, S, D] -> (codes, scales, the dequantised bf16 cache).  A poisoned (all-NaN)
    key vector becomes NaN codes under a NaN scale."""
    bad = torch.isnan(kc).any(-1)
    codes, scale = quantize_vectors(torch.where(bad[..., None], torch.zeros_like(kc), kc))
    codes = torch.where(bad[..., None], torch.full_like(_bytes(codes), NAN_CODE), _bytes(codes)).view(FP8)
    scale = torch.where(bad, torch.full_like(scale, float("nan")), scale)
    return codes, scale, dequantize(codes, scale)


# ---------------------------------------------------------------------------------------------
# the scale rule on the boundary vectors the append tests plant
# ---------------------------------------------------------------------------------------------
def special_vectors(D):
    """name -> (bf16 [D], expected scale, expected code byte of the largest element or None)."""
    g = torch.Generator().manual_seed(11 + D)
    small = (torch.rand(D, generator=g) * 0.5 + 0.25)  # in [0.25, 0.75)
    out = {"zero": (torch.zeros(D), 1.0, 0x00)}
    v = small * 448.0 * 8.0 * 0.9
    v[5] = -448.0 * 8.0            # amax exactly 448 * 2^3: stays at scale 2^3, code -448
    out["amax_448"] = (v, 8.0, 0xFE)
    v = small * 224.0 * 0.25 * 0.9
    v[D - 3] = 224.0 * 0.25        # amax exactly 224 * 2^-2: the next scale down, 2^-3, code 448
    out["amax_224"] = (v, 0.125, 0x7E)
    v = small.clone()
    v[D // 2 + 1] = 0.5 * 4096.0   # one element 2^12 times the rest: 2048 = 256 * 2^3
    out["spike"] = (v, 8.0, 0x78)  # 256 = 1.0 * 2^8: exponent field 15, mantissa 0
    return {k: (a.to(torch.bfloat16), s, c) for k, (a, s, c) in out.items()}


def check_scale_rule():
    """quantize_fp8_rows puts the boundary vectors where the rule says; they are exact in bf16."""
    for D in C.APPEND_DIMS:
        for name, (v, want_scale, want_code) in special_vectors(D).items():
            codes, scale = quantize_vectors(v[None])
            assert scale.item() == want_scale, (name, D, scale.item())
            i = int(v.float().abs().argmax())
            assert _bytes(codes)[0, i].item() == want_code, (name, D, hex(_bytes(codes)[0, i].item()))
            top = v.float().abs().max().item() / scale.item()
            assert top == 0 or 224 < top <= 448, (name, top)
            if name in ("amax_448", "amax_224"):
                assert abs(dequantize(codes, scale)[0, i].float().item()) == v.float().abs().max().item()
            if name == "spike":  # the rest, 2^-12 of the spike, lands below 2^-3: the lowest three binades or under
                rest = torch.cat([_bytes(codes)[0, :i], _bytes(codes)[0, i + 1:]]) & 0x7F
                assert (rest < 0x20).all() and (rest > 0).any(), name


# ---------------------------------------------------------------------------------------------
# kv_cache_append_fp8_
# ---------------------------------------------------------------------------------------------
NQ, NKV = C.NQ, C.NKV


def fresh_fp8_caches(D, dev):
    shape = (C.ROWS_MAX, NKV, C.S_MAX, D)
    kc = torch.full(shape, SENT_CODE, dtype=torch.uint8).view(FP8).to(dev)
    ks = torch.full(shape[:3], SENT_SCALE, dtype=torch.float32).to(dev)
    return kc, kc.clone(), ks, ks.clone()


def planted_inputs(D, T, seed):
    """_decode_cases.append_inputs with the boundary vectors in some k and v heads."""
    x = C.append_inputs(D, T, seed).clone()
    sp = special_vectors(D)
    k0, v0 = NQ * D, (NQ + NKV) * D
    plant = [(0, k0, "zero"), (0, v0 + D, "zero"), (1 % T, v0, "amax_448"), (1 % T, k0 + D, "amax_448")]
    if T > 3:
        plant += [(2, v0 + D, "amax_224"), (2, k0, "amax_224"), (3, v0, "spike"), (3, k0 + D, "spike")]
    for t, c0, name in plant:
        x[t, c0:c0 + D] = sp[name][0]
    return x


def _expect(cache, scales, written, what):
    """`written`: {(row, pos): (codes [nkv, D], scale [nkv])}; everything else still holds the sentinels."""
    exp_c = torch.full(cache.shape, SENT_CODE, dtype=torch.uint8)
    exp_s = torch.full(scales.shape, SENT_SCALE, dtype=torch.float32)
    for (r, p), (c, s) in written.items():
        exp_c[r, :, p] = _bytes(c)
        exp_s[r, :, p] = s
    assert torch.equal(_bytes(cache), exp_c), f"{what}: codes differ from the addressed writes over the sentinel"
    assert torch.equal(scales.cpu().view(torch.int32), exp_s.view(torch.int32)), f"{what}: scales differ"


def _append_once(D, dev, rope, x, pos, rows, caches, written):
    """One append of `x` (all tokens in range unless listed in `skip`); checks qkv and records the writes."""
    cos, sin = (t.to(dev) for t in C.tables(D)) if rope else (torch.empty(0, device=dev), torch.empty(0, device=dev))
    T, nqk = x.shape[0], (NQ + NKV) * D
    kc, vc, ks, vs = caches
    qkv = x.clone().to(dev)
    torch.ops.dtg.kv_cache_append_fp8_(qkv, kc, vc, ks, vs, cos, sin, pos.to(dev), rows.to(dev), NQ, NKV, D)
    live = ((pos >= 0) & (pos < C.S_MAX) & (rows >= 0) & (rows < C.ROWS_MAX)).tolist()
    want = x.clone().to(dev)
    if rope:  # rope_'s bits on the same device; the tokens out of range keep theirs
        idx = torch.tensor([t for t in range(T) if live[t]])
        sel = want[idx.to(dev)]
        torch.ops.dtg.rope_(sel, cos, sin, pos[idx].to(dev), NQ + NKV, D, False)
        want[idx.to(dev)] = sel
    want = want.cpu()
    got = qkv.cpu()
    assert torch.equal(_bits(got[:, : NQ * D]), _bits(want[:, : NQ * D])), "roped q differs from rope_"
    for name, c0, written_to in (("k", NQ * D, written[0]), ("v", nqk, written[1])):
        src = want[:, c0:c0 + NKV * D].reshape(T, NKV, D)  # the roped k / the v
        codes, scale = quantize_vectors(src)
        deq = dequantize(codes, scale)
        for t in range(T):
            cols = got[t, c0:c0 + NKV * D].reshape(NKV, D)
            if live[t]:
                assert torch.equal(_bits(cols), _bits(deq[t])), f"{name} of token {t}: qkv is not code * scale of the roped value"
                written_to[(int(rows[t]), int(pos[t]))] = (codes[t], scale[t])
            else:
                assert torch.equal(_bits(cols), _bits(x[t, c0:c0 + NKV * D].reshape(NKV, D))), f"token {t} was modified"
    for t in range(T):
        if not live[t]:
            assert torch.equal(_bits(got[t]), _bits(x[t])), f"out-of-range token {t} was modified"
    _expect(kc, ks, written[0], f"k D{D}")
    _expect(vc, vs, written[1], f"v D{D}")


def check_append(D, dev, rope):
    """The packed prefill, then the decode step, on one set of caches: codes and scales equal
    quantize_fp8_rows of the roped k / the v bit for bit, qkv holds rope_'s q and the dequantised k / v."""
    caches, written = fresh_fp8_caches(D, dev), ({}, {})
    for seed, batch in ((1, C.PREFILL), (2, C.STEP)):
        T = len(batch["pos"])
        _append_once(D, dev, rope, planted_inputs(D, T, seed), torch.tensor(batch["pos"], dtype=torch.long),
                     torch.tensor(batch["rows"], dtype=torch.int32), caches, written)
    assert len(written[0]) == 8


def check_append_out_of_range(D, dev, rope):
    """The five tokens of _decode_cases.check_append_out_of_range: four write nothing and stay as they were
    (neither roped nor written back), the fifth is handled as usual."""
    pos = torch.tensor([C.S_MAX, -1, 2, 0, 3], dtype=torch.long)
    rows = torch.tensor([0, 1, C.ROWS_MAX, -1, 2], dtype=torch.int32)
    written = ({}, {})
    _append_once(D, dev, rope, planted_inputs(D, 5, 3), pos, rows, fresh_fp8_caches(D, dev), written)
    assert list(written[0]) == [(2, 3)] and list(written[1]) == [(2, 3)]


# ---------------------------------------------------------------------------------------------
# decode_attn_fp8, q_len = 1
# ---------------------------------------------------------------------------------------------
def _reference(qkv, kc, vc, rows, token_lens, nq, nkv, D, window, scale):
    """ref and term of _decode_cases.make_case (the same formulas), one query row per entry of token_lens."""
    G_ = nq // nkv
    n_tok = len(token_lens)
    ref = torch.zeros(n_tok, nq * D, dtype=torch.float64)
    term = torch.zeros(n_tok, nq * D, dtype=torch.float64)
    for i, (r, n1) in enumerate(zip(rows, token_lens)):
        n0 = max(0, n1 - window) if window else 0
        n = n1 - n0
        if n <= 0 or r is None:
            continue
        q = f64(qkv)[i, : nq * D].reshape(nkv, G_, D)
        k, v = f64(kc)[r, :, n0:n1], f64(vc)[r, :, n0:n1]
        s = scale * torch.einsum("hgd,hnd->hgn", q, k)
        e = (D + 2) * scale * torch.einsum("hgd,hnd->hgn", q.abs(), k.abs())
        m = s.amax(-1, keepdim=True)
        p = torch.softmax(s, -1)
        rel = e + 2 * (s - m).abs() + 2
        o = torch.einsum("hgn,hnd->hgd", p, v)
        num = torch.einsum("hgn,hnd->hgd", p * (rel + n + 1), v.abs())
        den = (p * rel).sum(-1, keepdim=True) + n + 1
        ref[i] = o.reshape(-1)
        term[i] = (K * U * (num + o.abs() * den)).reshape(-1)
    return ref, term


def _quantized(c, ref_rows, token_lens):
    kq, ks, kd = quantize_cache(c["kc"])
    vq, vs, vd = quantize_cache(c["vc"])
    ref, term = _reference(c["qkv"], kd, vd, ref_rows, token_lens, c["nq"], c["nkv"], c["D"], c["window"], c["scale"])
    return dict(c, kq=kq, ks=ks, vq=vq, vs=vs, kc=kd, vc=vd, ref=ref, term=term)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """_decode_cases.make_case(name) with the caches quantised per key vector: kq / vq / ks / vs, kc / vc the
    dequantised bf16 caches, ref / term recomputed on them."""
    c = C.make_case(name)
    q = _quantized(c, c["rows"].tolist(), c["lens"].tolist())
    if C.CASES[name][9]:  # poisoned: everything outside the attended ranges is a NaN code under a NaN scale
        window = c["window"]
        keep = torch.zeros(c["kc"].shape[0], c["kc"].shape[2], dtype=torch.bool)
        for r, n in zip(c["rows"].tolist(), c["lens"].tolist()):
            keep[r, (max(0, n - window) if window else 0): n] = True
        out = ~keep[:, None, :].expand(-1, c["nkv"], -1)
        for codes, scales in ((q["kq"], q["ks"]), (q["vq"], q["vs"])):
            assert (_bytes(codes)[out] == NAN_CODE).all() and torch.isnan(scales[out]).all()
            assert not torch.isnan(scales[~out]).any()
    return q


def _fp8_args(c, dev):
    return tuple(c[k].to(dev) for k in ("qkv", "kq", "vq", "ks", "vs", "rows", "lens"))


def check_decode(c, dev, splits):
    """decode_attn_fp8 at q_len 1 against the f64 reference on the dequantised values, the bound unchanged;
    twice, bitwise equal."""
    args = _fp8_args(c, dev)
    runs = [torch.ops.dtg.decode_attn_fp8(*args, 1, c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"], c["window"],
                                          splits) for _ in range(2)]
    assert runs[0].shape == (c["B"], c["nq"] * c["D"]) and runs[0].dtype == torch.bfloat16
    assert_within(runs[0], c["ref"], c["term"], f"decode_attn_fp8 {c['name']} splits {splits}")
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "not reproducible"
    assert torch.equal(_bits(args[0]), _bits(c["qkv"])), "qkv was written"


def check_decode_bitwise(c, dev, splits):
    """decode_attn_fp8(codes, scales) equals decode_attn(dequantised bf16 caches) on the same device with the
    same max_len, window and splits, bit for bit.  Cache values are randn-sized: the claim is made for scales
    whose products stay in the normal f32 range."""
    args = _fp8_args(c, dev)
    tail = (c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"], c["window"], splits)
    got = torch.ops.dtg.decode_attn_fp8(*args, 1, *tail)
    want = torch.ops.dtg.decode_attn(args[0], c["kc"].to(dev), c["vc"].to(dev), args[5], args[6], *tail)
    assert torch.equal(_bits(got), _bits(want)), f"{c['name']} splits {splits}: differs from decode_attn on the dequantised cache"


# ---------------------------------------------------------------------------------------------
# decode_attn_fp8, q_len > 1
# ---------------------------------------------------------------------------------------------
# query tiles of 8 (G 1, 2), 4 (G 3, 4), 2 (G 7, 8) and 1 (G 16) tokens; one and several splits; a planned split;
# window, poisoned, inactive and indirect-row cases
MULTI_CASES = ["straddle", "straddle_d64", "planned_split", "planned_split_g4", "window", "poisoned", "poisoned_window",
               "inactive", "row_indirection", "Q16_G4_D64", "Q8_G2_D128", "G1_D128", "G3_D64", "G7_D64", "G8_D128",
               "G16_D64", "G16_D128"]
MULTI_RUNS = [(n, s) for n in MULTI_CASES for s in M.CASES[n]["splits"]]


@functools.lru_cache(maxsize=None)
def make_multi_case(name):
    c = M.make_case(name)
    Q = c["Q"]
    rows = [r if 0 <= r < c["kc"].shape[0] else None for r in c["rows"].tolist() for _ in range(Q)]
    return _quantized(c, rows, c["lens"].tolist())


def check_multi_bitwise(c, dev, splits):
    """decode_attn_fp8 at q_len > 1 equals decode_attn_multi on the dequantised bf16 caches bit for bit (window
    cases too: the comparison is within one template), and stays within the f64 bound.  Cache values are
    randn-sized: the claim is made for scales whose products stay in the normal f32 range."""
    args = _fp8_args(c, dev)
    tail = (c["Q"], c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"], c["window"], splits)
    got = torch.ops.dtg.decode_attn_fp8(*args, *tail)
    want = torch.ops.dtg.decode_attn_multi(args[0], c["kc"].to(dev), c["vc"].to(dev), args[5], args[6], *tail)
    assert got.shape == (c["B"] * c["Q"], c["nq"] * c["D"])
    assert torch.equal(_bits(got), _bits(want)), f"{c['name']} splits {splits}: differs from decode_attn_multi"
    assert_within(got, c["ref"], c["term"], f"decode_attn_fp8 multi {c['name']} splits {splits}")
    assert (_bits(got)[c["zero"]] == 0).all(), "an inactive token's output row is not exact zeros"


# ---------------------------------------------------------------------------------------------
# public ops
# ---------------------------------------------------------------------------------------------
PUBLIC_CASES = ["boundaries", "window", "poisoned_window", "row_indirection", "G7_D64", "logit_range"]


def check_public(c, dev, fused, splits, monkeypatch):
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    qkv, kq, vq, ks, vs, rows, lens = _fp8_args(c, dev)
    out = ops.decode_attention(qkv, kq, vq, rows.long(), lens, c["nq"], c["nkv"], c["D"], c["max_len"],
                               window=c["window"], splits=splits, k_scale=ks, v_scale=vs)
    assert_within(out, c["ref"], c["term"], f"decode_attention fp8 {c['name']} {'fused' if fused else 'composed'}")


def check_public_multi(dev, fused, monkeypatch):
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    c = make_multi_case("straddle")
    qkv, kq, vq, ks, vs, rows, lens = _fp8_args(c, dev)
    out = ops.decode_attention_multi(qkv, kq, vq, rows.long(), lens, c["Q"], c["nq"], c["nkv"], c["D"], c["max_len"],
                                     splits=2 if fused else 0, k_scale=ks, v_scale=vs)
    assert_within(out, c["ref"], c["term"], f"decode_attention_multi fp8 {'fused' if fused else 'composed'}")


def check_public_append(dev, fused, monkeypatch):
    """ops.kv_cache_append with scales, fused and composed: quantize_fp8_rows' codes and scales, qkv written back."""
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    D = 64
    kc, vc, ks, vs = fresh_fp8_caches(D, dev)
    x = planted_inputs(D, 6, 1)
    pos, rows = torch.tensor(C.PREFILL["pos"]), torch.tensor(C.PREFILL["rows"])
    cos, sin = (t.to(dev) for t in C.tables(D))
    qkv = ops.kv_cache_append(x.clone().to(dev), kc, vc, pos.to(dev), rows.to(dev), NQ, NKV, D, cos, sin, pos_max=4,
                              row_max=3, k_scale=ks, v_scale=vs)
    want = x.clone().to(dev)
    torch.ops.dtg.rope_(want, cos, sin, pos.to(dev), NQ + NKV, D, False)
    want = want.cpu()
    wk, wv = {}, {}
    for c0, written in ((NQ * D, wk), ((NQ + NKV) * D, wv)):
        codes, scale = quantize_vectors(want[:, c0:c0 + NKV * D].reshape(6, NKV, D))
        assert torch.equal(_bits(qkv[:, c0:c0 + NKV * D]), _bits(dequantize(codes, scale).reshape(6, NKV * D)))
        for t in range(6):
            written[(int(rows[t]), int(pos[t]))] = (codes[t], scale[t])
    _expect(kc, ks, wk, "k")
    _expect(vc, vs, wv, "v")


def check_public_errors(dev):
    c = make_case("boundaries")
    qkv, kq, vq, ks, vs, rows, lens = _fp8_args(c, dev)
    a = (rows, lens, c["nq"], c["nkv"], c["D"], c["max_len"])
    with pytest.raises(ValueError, match="k_scale / v_scale were given"):
        ops.decode_attention(qkv, c["kc"].to(dev), c["vc"].to(dev), *a, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        ops.decode_attention(qkv, kq, vq, *a)
    with pytest.raises(ValueError, match="k_scale must be"):
        ops.decode_attention(qkv, kq, vq, *a, k_scale=ks[:, :, :-1].contiguous(), v_scale=vs)
    with pytest.raises(ValueError, match="v_scale must be"):
        ops.decode_attention(qkv, kq, vq, *a, k_scale=ks, v_scale=vs.double())
    with pytest.raises(ValueError, match="both k_scale and v_scale"):
        ops.decode_attention(qkv, kq, vq, *a, k_scale=ks)
    pos = torch.zeros(qkv.shape[0], dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        ops.kv_cache_append(qkv.clone(), kq, vq, pos, rows, c["nq"], c["nkv"], c["D"])
    m = make_multi_case("straddle")
    qkv, kq, vq, ks, vs, rows, lens = _fp8_args(m, dev)
    with pytest.raises(ValueError, match="k_scale / v_scale were given"):
        ops.decode_attention_multi(qkv, m["kc"].to(dev), m["vc"].to(dev), rows, lens, m["Q"], m["nq"], m["nkv"], m["D"],
                                   m["max_len"], k_scale=ks, v_scale=vs)


def check_zero_sequences(dev):
    c = make_case("single_key")
    e = torch.empty(0, dtype=torch.int32, device=dev)
    _, kq, vq, ks, vs, _, _ = _fp8_args(c, dev)
    out = torch.ops.dtg.decode_attn_fp8(c["qkv"][:0].to(dev), kq, vq, ks, vs, e, e, 1, c["nq"], c["nkv"], c["D"], c["scale"],
                                        0, 0, 0)
    assert out.shape == (0, c["nq"] * c["D"]) and out.device.type == torch.device(dev).type
    qkv = torch.empty(0, (NQ + 2 * NKV) * 64, dtype=torch.bfloat16, device=dev)
    kc, vc, ks, vs = fresh_fp8_caches(64, dev)
    z = torch.empty(0, device=dev)
    torch.ops.dtg.kv_cache_append_fp8_(qkv, kc, vc, ks, vs, z, z, torch.empty(0, dtype=torch.long, device=dev), e, NQ, NKV, 64)
    assert (_bytes(kc) == SENT_CODE).all() and (ks == SENT_SCALE).all()


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------
WIRING_STEPS = 8
PRE = (gc.PREFIX, gc.PREFIX - gc.SHORTER)  # 8 / 5 tokens


def _fake_quantize(cache_t, qkv, c0, rows, pos, nkv, d):
    """Quantise the slots (rows, pos) of the bf16 cache in place and copy them into qkv's columns from c0."""
    r, p = rows.long(), pos.long()
    x = cache_t[r, :, p]
    codes, scale = ops.quantize_fp8_rows(x.reshape(-1, d))
    deq = (codes.float() * scale[:, None]).to(x.dtype).reshape(x.shape)
    cache_t[r, :, p] = deq
    qkv[:, c0:c0 + nkv * d] = deq.reshape(-1, nkv * d)


class WiringOracle:
    """prefill and decode_step on a bf16 KVCache whose attention callback appends with the bf16 op, fake-quantises
    the slots just written (cache and qkv alike) and attends with the bf16 ops: what an FP8 cache must compute."""

    def __init__(self, model, n, s_max, dev):
        self.model, self.dev = model, dev
        self.cache = KVCache(model.config, n, s_max, device=dev)
        self.lens = [0] * n

    def _attend(self, pos, tok_rows, pos_max, attention):
        cache = self.cache
        cos, sin = self.model._rope_tables(cache.s_max, self.dev)

        def attend(i, attn, qkv):
            qkv = G._append(attn, qkv, cache, i, cos, sin, pos, tok_rows, pos_max)
            _fake_quantize(cache.k[i], qkv, attn.nq * attn.d, tok_rows, pos, attn.nkv, attn.d)
            _fake_quantize(cache.v[i], qkv, (attn.nq + attn.nkv) * attn.d, tok_rows, pos, attn.nkv, attn.d)
            return attention(i, attn, qkv)

        return attend

    @torch.no_grad()
    def prefill(self, prompts):
        model, dev = self.model, self.dev
        lens = [len(p) for p in prompts]
        ids = torch.cat(prompts).to(dev)
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev)
        cu = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(dev)
        tok_rows = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(torch.int32).to(dev)
        attend = self._attend(pos, tok_rows, max(lens) - 1, lambda i, attn, qkv: ops.attention(
            qkv, attn.nq, attn.nkv, attn.d, cu, max(lens), window=attn.window))
        x, res = G._run_layers(model, ops.embedding(ids, model.embed_tokens.weight), attend, "blas")
        last = (cu[1:] - 1).long()
        self.lens = lens
        return G._last_logits(model, x[last], res[last], "blas")

    @torch.no_grad()
    def step(self, tokens, linear):
        model, dev, cache = self.model, self.dev, self.cache
        n = len(self.lens)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        pos = torch.tensor(self.lens, device=dev)
        new_lens = (pos + 1).to(torch.int32)
        plan_len = max(self.lens) + 1
        attend = self._attend(pos, rows, plan_len - 1, lambda i, attn, qkv: ops.decode_attention(
            qkv, cache.k[i], cache.v[i], rows, new_lens, attn.nq, attn.nkv, attn.d, plan_len, window=attn.window))
        x, res = G._run_layers(model, ops.embedding(tokens.to(dev), model.embed_tokens.weight), attend, linear)
        self.lens = [v + 1 for v in self.lens]
        return G._last_logits(model, x, res, linear)


def _teacher_forced(kind, dev, linear, kv_cache):
    model, _ = gc.models(kind, dev)
    seqs = gc.sequences(kind)
    cache = KVCache(model.config, 2, PRE[0] + WIRING_STEPS, device=dev, kv_cache=kv_cache)
    out = [prefill(model, [s[:p] for s, p in zip(seqs, PRE)], cache).float().cpu()]
    for t in range(WIRING_STEPS):
        out.append(decode_step(model, torch.stack([s[p + t] for s, p in zip(seqs, PRE)]), cache, linear=linear).float().cpu())
    return torch.stack(out, 1)  # [2, 1 + steps, V]


def check_wiring(kind, dev, linear, exact):
    """Teacher-forced prefill on 8 / 5 tokens and WIRING_STEPS decode steps on KVCache(kv_cache="fp8") against
    the WiringOracle: bit for bit when `exact` (linear="skinny" on the GPU), else within 2 * e_full (both sides
    hold identical cache values; only GEMM order differs).  Prints e_fp8 beside e_full and e_cached and asserts
    only that it is finite and positive: a bf16-sized change of k can flip an e4m3 code, so no bf16 bound holds."""
    model, ref = gc.models(kind, dev)
    seqs = gc.sequences(kind)
    got = _teacher_forced(kind, dev, linear, "fp8")
    oracle = WiringOracle(model, 2, PRE[0] + WIRING_STEPS, dev)
    want = [oracle.prefill([s[:p] for s, p in zip(seqs, PRE)]).float().cpu()]
    for t in range(WIRING_STEPS):
        want.append(oracle.step(torch.stack([s[p + t] for s, p in zip(seqs, PRE)]), linear).float().cpu())
    want = torch.stack(want, 1)
    cached = _teacher_forced(kind, dev, linear, "bf16")
    e_full = e_cached = e_fp8 = 0.0
    for i, (s, p) in enumerate(zip(seqs, PRE)):
        r = gc.full_logits(ref, s[: p + WIRING_STEPS])[p - 1:]
        e_full = max(e_full, (gc.full_logits(model, s[: p + WIRING_STEPS])[p - 1:] - r).abs().max().item())
        e_cached = max(e_cached, (cached[i] - r).abs().max().item())
        e_fp8 = max(e_fp8, (got[i] - r).abs().max().item())
    print(f"[kv-fp8] {kind} {linear} teacher-forced: e_full {e_full:.5f}, e_cached {e_cached:.5f}, e_fp8 {e_fp8:.5f}")
    assert e_full > 0 and e_fp8 > 0 and e_fp8 == e_fp8 and e_fp8 != float("inf")
    if exact:
        for t in range(1 + WIRING_STEPS):
            assert torch.equal(got[:, t], want[:, t]), f"{kind}: logits of step {t} differ from the oracle's"
    else:
        d = (got - want).abs().max().item()
        assert d <= 2 * e_full, f"{kind}: FP8-cache path {d} from the oracle, allowed {2 * e_full}"
    assert not torch.equal(got, cached), "the FP8 cache computed the bf16 cache's logits"


def check_graph_bitwise(kind, dev, linear="skinny"):
    """The captured loop on an FP8 cache returns the bucketed eager loop's ids bit for bit, greedy and under the
    fused sampler."""
    model, _ = gc.models(kind, dev)
    prompts = dc.long_prompts(kind)
    fp8 = sc.fp8_weights(kind, dev) if linear == "skinny-fp8" else None
    for kw in ({}, dict(sampler="fused", temperature=[0.0, gc.SAMPLE_T], top_k=[0, 50], top_p=[1.0, 0.95], seed=5)):
        common = dict(s_max=dc.S_MAX, linear=linear, fp8=fp8, kv_cache="fp8", **kw)
        graph = generate(model, prompts, dc.NEW, decode="graph", **common)
        eager = generate(model, prompts, dc.NEW, decode="eager", bucketed=True, **common)
        for g, e in zip(graph, eager):
            assert g.shape == (dc.NEW,) and torch.equal(g, e), (g.tolist(), e.tolist())
        if not kw:
            assert all(len(set(g.tolist())) >= dc.NEW - 2 for g in graph), "degenerate continuation"


@functools.lru_cache(maxsize=None)
def plain_loop(kind, dev, linear, kv_cache):
    """ids [n, NEW] of prefill + decode_step planned for the fixed bucket P throughout (what _spec_cases.reference
    computes), on a cache of the given format."""
    model, _ = gc.models(kind, dev)
    prompts = dc.long_prompts(kind)
    P = decode_bucket(max(len(p) for p in prompts) + dc.NEW, dc.S_MAX)
    cache = KVCache(model.config, len(prompts), dc.S_MAX, device=dev, kv_cache=kv_cache)
    logits = prefill(model, prompts, cache)
    ids = []
    for step in range(dc.NEW):
        nxt = logits.argmax(-1)
        ids.append(nxt.cpu())
        if step + 1 < dc.NEW:
            logits = decode_step(model, nxt, cache, linear=linear, plan_len=P)
    return torch.stack(ids, 1)


def check_speculative(kind, dev, linear="skinny"):
    """An oracle drafter and a drafter spoiled at every index, k = 2 and 4, on an FP8 cache: the plain loop's ids
    bit for bit.  A spoiled draft leaves rejected quantised keys past lens; equality shows that they are
    overwritten and never attended."""
    model, _ = gc.models(kind, dev)
    prompts = dc.long_prompts(kind)
    ref = plain_loop(kind, dev, linear, "fp8")
    assert all(len(set(r.tolist())) >= dc.NEW - 2 for r in ref), f"degenerate reference {ref.tolist()}"
    for k in (2, 4):
        for wrong_at in [None] + list(range(k - 1)):
            spec = Speculative(sc.Oracle(ref, prompts, wrong_at=wrong_at), k=k)
            got = generate(model, prompts, dc.NEW, s_max=dc.S_MAX, linear=linear, speculate=spec, kv_cache="fp8")
            for i, (g, r) in enumerate(zip(got, ref)):
                assert torch.equal(g, r), f"{kind} k={k} wrong_at={wrong_at}: row {i} {g.tolist()} != {r.tolist()}"
            st = spec.stats
            if wrong_at is None:
                assert st["accepted"] == st["proposed"] > 0, st
            else:
                assert st["accepted"] < st["proposed"], st


def check_arguments(dev):
    model, _ = gc.models("llama", dev)
    prompts = [p[:12] for p in dc.long_prompts("llama")]
    with pytest.raises(ValueError, match="kv_cache"):
        generate(model, prompts, 4, kv_cache="int8")
    with pytest.raises(ValueError, match="kv_cache"):
        KVCache(model.config, 2, 16, device=dev, kv_cache="int8")
    cfg = model.config
    a = KVCache(cfg, 3, 40, device=dev)
    b = KVCache(cfg, 3, 40, device=dev, kv_cache="fp8")
    D = cfg.head_dim
    vectors = 2 * cfg.num_hidden_layers * 3 * cfg.num_key_value_heads * 40  # K and V, per layer, row, head, position
    assert a.nbytes == vectors * 2 * D and b.nbytes == vectors * (D + 4)   # bf16: 2 D bytes; fp8: D codes + an f32 scale
    assert b.nbytes * 2 * D == a.nbytes * (D + 4)
    assert a.k_scale is None and a.v_scale is None and len(b.k_scale) == len(b.v_scale) == cfg.num_hidden_layers
    assert b.k[0].dtype == FP8 and b.k_scale[0].shape == b.k[0].shape[:3] and b.k_scale[0].dtype == torch.float32
    b.lens += 3
    b.max_len = 3
    b.reset()
    assert b.max_len == 0 and int(b.lens.sum()) == 0
    out = generate(model, prompts, 4, kv_cache="fp8")
    assert all(o.shape == (4,) for o in out)


def greedy_share(kind, dev, linear):
    """Share of the 24 greedy ids per row on an FP8 cache that equal the bf16-cache run's ids."""
    model, _ = gc.models(kind, dev)
    prompts = [s[:p] for s, p in zip(gc.sequences(kind), PRE)]
    a = generate(model, prompts, gc.NEW_TOKENS, linear=linear)
    b = generate(model, prompts, gc.NEW_TOKENS, linear=linear, kv_cache="fp8")
    return sum(int((x == y).sum()) for x, y in zip(a, b)) / (2 * gc.NEW_TOKENS)
