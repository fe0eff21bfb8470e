"""Cases, float64 references and f32 error terms of the KV-cache operators kv_cache_append_ and
decode_attn (csrc/kernels/decode_attn.hip, dtg.ops._cpu), shared by test_decode_attn_cpu.py (the CPU
operators) and test_decode_attn_gpu.py (the gfx950 kernels).  The references are plain torch in
float64 and use none of the package's own ops.

decode_attn, per sequence b, query head g and output column c, over the n attended keys
j in [max(0, len - window), len) of cache row rows[b]:

    s_j = scale * sum_i q_i k_ji,   p_j = exp(s_j - m) / sum_j exp(s_j - m),  m = max_j s_j,
    out_c = sum_j p_j v_jc.

Bound (tests/_refs.py): half a bf16 ulp of out for the single store, plus an f32 term of U = 2^-24 per
operation on the magnitudes combined, times K = 8.  The kernel runs QK and PV on the VALU in f32 and
does NOT round P to bf16, so there is no 2^-9 sum p |v| term.  In units of U:

  * s_j: D products, a D-term reduction and the scale on sum_i |scale q_i k_ji|:
        e_j = (D + 2) * scale * sum_i |q_i k_ji|.
    It moves the unnormalised weight of key j by that relative amount (exp' = exp).
  * the exponent s_j - m_run is taken against a running max and later rescaled by exp(m_run - m_new)
    steps; m itself cancels between numerator and denominator, the subtractions round on at most
    2 |s_j - m| in total, exp and the product with v round once each:
        rel_j = e_j + 2 |s_j - m| + 2.
  * numerator: the relative errors above on p_j |v_jc|, plus an n-term sum and up to n rescaling
    products on sum_j p_j |v_jc|.  Denominator: the same on sum_j p_j = 1; it scales |out_c|.  The
    division rounds once more on |out_c|:
        term_c = K U [ sum_j p_j |v_jc| (rel_j + n + 1) + |out_c| (sum_j p_j rel_j + n + 1) ].

Nothing here comes from a run of the code under test.
"""
import functools

import torch

import dtg.ops  # noqa: F401  (defines torch.ops.dtg)
from _refs import K, U, assert_within, f64, rope_ref

SENTINEL = 0x4B4B  # bf16 bits the append tests fill the caches with


# name -> (D, nq, nkv, lens, rows, rows_max, S_max, window, q_scale, poison, splits tried)
def _c(D, nq, nkv, lens, splits, rows=None, rows_max=None, S_max=None, window=0, q_scale=1.0, poison=False):
    rows = list(range(len(lens))) if rows is None else rows
    S_max = S_max or max(8, max(lens) + 3)
    return (D, nq, nkv, tuple(lens), tuple(rows), rows_max or len(lens), S_max, window, q_scale, poison, tuple(splits))


CASES = {
    "single_key": _c(128, 4, 2, [1], (0, 1, 2)),
    "boundaries": _c(128, 4, 2, [1, 2, 63, 64, 65], (1, 2, 5)),
    "boundaries_d64": _c(64, 4, 2, [1, 2, 63, 64, 65], (1, 2, 5)),
    "empty_splits": _c(128, 8, 2, [1, 300], (5,)),
    "window": _c(128, 4, 2, [300, 40, 64], (1, 3), window=64),
    "window_d64": _c(64, 2, 2, [300, 40, 64], (1, 3), window=64),
    "logit_range": _c(128, 4, 1, [200, 70], (1, 3), q_scale=8.0),
    "row_indirection": _c(64, 4, 2, [20, 65, 130], (0, 2), rows=[4, 0, 2], rows_max=5),
    "poisoned": _c(128, 4, 2, [1, 300], (1, 5), poison=True),
    "poisoned_window": _c(64, 4, 2, [300, 40, 64], (1, 3), rows=[3, 0, 1], rows_max=5, window=64, poison=True),
    "planned_split": _c(128, 2, 1, [511, 300], (0,), S_max=512),  # long enough for the plan itself to split
}
# every group-size and head-dim instantiation (2, 4, 8 ride along)
for _D in (64, 128):
    for _G in (1, 2, 3, 4, 7, 8, 16):
        CASES[f"G{_G}_D{_D}"] = _c(_D, 2 * _G, 2, [37, 130], (1, 3))

RUNS = [(name, s) for name, c in CASES.items() for s in c[-1]]


def run_id(r):
    return f"{r[0]}-splits{r[1]}"


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Inputs (CPU, bf16) and the reference of one case; computed once, shared, never modified."""
    D, nq, nkv, lens, rows, rows_max, S_max, window, q_scale, poison, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    B, G = len(lens), nq // nkv
    qkv = torch.randn(B, (nq + 2 * nkv) * D, generator=g)
    qkv[:, : nq * D] *= q_scale
    qkv = qkv.to(torch.bfloat16)
    kc = torch.randn(rows_max, nkv, S_max, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(rows_max, nkv, S_max, D, generator=g).to(torch.bfloat16)
    scale = D ** -0.5
    if poison:  # everything outside each row's attended range, unused rows included
        keep = torch.zeros(rows_max, S_max, dtype=torch.bool)
        for b in range(B):
            keep[rows[b], (max(0, lens[b] - window) if window else 0): lens[b]] = True
        kc = torch.where(keep[:, None, :, None], kc, torch.full_like(kc, float("nan")))
        vc = torch.where(keep[:, None, :, None], vc, torch.full_like(vc, float("nan")))
    ref = torch.zeros(B, nq * D, dtype=torch.float64)
    term = torch.zeros(B, nq * D, dtype=torch.float64)
    for b in range(B):
        n1 = lens[b]
        n0 = max(0, n1 - window) if window else 0
        n = n1 - n0
        q = f64(qkv)[b, : nq * D].reshape(nkv, G, D)
        k, v = f64(kc)[rows[b], :, n0:n1], f64(vc)[rows[b], :, n0:n1]       # [nkv, n, D]
        s = scale * torch.einsum("hgd,hnd->hgn", q, k)
        e = (D + 2) * scale * torch.einsum("hgd,hnd->hgn", q.abs(), k.abs())
        m = s.amax(-1, keepdim=True)
        p = torch.softmax(s, -1)
        rel = e + 2 * (s - m).abs() + 2
        o = torch.einsum("hgn,hnd->hgd", p, v)
        num = torch.einsum("hgn,hnd->hgd", p * (rel + n + 1), v.abs())
        den = (p * rel).sum(-1, keepdim=True) + n + 1
        ref[b] = o.reshape(-1)
        term[b] = (K * U * (num + o.abs() * den)).reshape(-1)
    return dict(name=name, D=D, nq=nq, nkv=nkv, G=G, B=B, lens=torch.tensor(lens, dtype=torch.int32),
                rows=torch.tensor(rows, dtype=torch.int32), max_len=max(lens), window=window, scale=scale,
                qkv=qkv, kc=kc, vc=vc, ref=ref, term=term)


def _args(c, dev):
    return tuple(c[k].to(dev) for k in ("qkv", "kc", "vc", "rows", "lens"))


def check_decode(c, dev, splits):
    """The raw operator on `dev` against the reference; twice, bitwise equal."""
    qkv, kc, vc, rows, lens = _args(c, dev)
    runs = [torch.ops.dtg.decode_attn(qkv, kc, vc, rows, lens, c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"],
                                      c["window"], splits) for _ in range(2)]
    assert runs[0].shape == (c["B"], c["nq"] * c["D"]) and runs[0].dtype == torch.bfloat16
    assert_within(runs[0], c["ref"], c["term"], f"decode_attn {c['name']} splits {splits}")
    assert torch.equal(runs[0].cpu().view(torch.int16), runs[1].cpu().view(torch.int16)), "not reproducible"
    assert torch.equal(qkv.cpu().view(torch.int16), c["qkv"].view(torch.int16)), "qkv was written"


def check_public_decode(c, dev, fused, splits, monkeypatch):
    """ops.decode_attention through the kernels and through the DTG_DECODE_FUSED=0 composition: the
    same reference, the same bound."""
    from dtg import ops
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    qkv, kc, vc, rows, lens = _args(c, dev)
    out = ops.decode_attention(qkv, kc, vc, rows.long(), lens, c["nq"], c["nkv"], c["D"], c["max_len"],
                               window=c["window"], splits=splits)
    assert_within(out, c["ref"], c["term"], f"decode_attention {c['name']} {'fused' if fused else 'composed'}")


# ---------------------------------------------------------------------------------------------
# kv_cache_append_
# ---------------------------------------------------------------------------------------------
APPEND_DIMS = (64, 128)
NQ, NKV, ROWS_MAX, S_MAX, MAX_POS = 4, 2, 4, 8, 16
# two prompts of lengths 5 and 1 packed together (cache rows 3 and 1), then a one-token decode step
# for both rows in the other order
PREFILL = dict(pos=[0, 1, 2, 3, 4, 0], rows=[3, 3, 3, 3, 3, 1])
STEP = dict(pos=[1, 5], rows=[1, 3])


@functools.lru_cache(maxsize=None)
def tables(D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    return fr.cos().float().contiguous(), fr.sin().float().contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def fresh_caches(D, dev):
    kc = torch.full((ROWS_MAX, NKV, S_MAX, D), SENTINEL, dtype=torch.int16).view(torch.bfloat16).to(dev)
    return kc, kc.clone()


def append_inputs(D, T, seed):
    g = torch.Generator().manual_seed(seed + D)
    return (2.0 * torch.randn(T, (NQ + 2 * NKV) * D, generator=g)).to(torch.bfloat16)


def _expect_cache(cache, written, what):
    """`written`: {(row, pos): [nkv, D] bf16}.  Those slots hold exactly that; every other element
    still holds the sentinel."""
    exp = torch.full(cache.shape, SENTINEL, dtype=torch.int16)
    for (r, p), val in written.items():
        exp[r, :, p] = _bits(val)
    assert torch.equal(_bits(cache), exp), f"{what}: cache differs from the addressed writes over the sentinel"


def check_append(D, dev, rope):
    """The packed prefill followed by the decode step, on one pair of caches."""
    ops = torch.ops.dtg
    cos, sin = (t.to(dev) for t in tables(D)) if rope else (torch.empty(0, device=dev), torch.empty(0, device=dev))
    kc, vc = fresh_caches(D, dev)
    k_written, v_written = {}, {}
    for seed, batch in ((1, PREFILL), (2, STEP)):
        T = len(batch["pos"])
        x = append_inputs(D, T, seed)
        pos = torch.tensor(batch["pos"], dtype=torch.long)
        rows = torch.tensor(batch["rows"], dtype=torch.int32)
        qkv = x.clone().to(dev)
        ops.kv_cache_append_(qkv, kc, vc, cos, sin, pos.to(dev), rows.to(dev), NQ, NKV, D)
        nqk = (NQ + NKV) * D
        if rope:
            # bit for bit what rope_ makes of the same input on the same device ...
            want = x.clone().to(dev)
            ops.rope_(want, cos, sin, pos.to(dev), NQ + NKV, D, False)
            assert torch.equal(_bits(qkv), _bits(want)), "roped q / k differ from rope_ (or v columns changed)"
            # ... and within the f64 reference's bound, independently of rope_
            r64, term = rope_ref(x, *tables(D), pos, NQ + NKV, D, False)
            assert_within(qkv[:, :nqk], r64[:, :nqk], term[:, :nqk], f"kv_cache_append_ rope D{D}")
        else:
            assert torch.equal(_bits(qkv), _bits(x)), "copy-only form changed qkv"
        assert torch.equal(_bits(qkv[:, nqk:]), _bits(x[:, nqk:])), "v columns of qkv changed"
        k_new = qkv[:, NQ * D: nqk].cpu().reshape(T, NKV, D)
        for t in range(T):
            k_written[(batch["rows"][t], batch["pos"][t])] = k_new[t]
            v_written[(batch["rows"][t], batch["pos"][t])] = x[t, nqk:].reshape(NKV, D)
        _expect_cache(kc, k_written, f"k D{D}")
        _expect_cache(vc, v_written, f"v D{D}")


def check_append_out_of_range(D, dev, rope):
    """Tokens whose pos or row lies outside the cache write nothing and are left as they were; the one
    valid token beside them is handled as usual."""
    ops = torch.ops.dtg
    cos, sin = (t.to(dev) for t in tables(D)) if rope else (torch.empty(0, device=dev), torch.empty(0, device=dev))
    kc, vc = fresh_caches(D, dev)
    pos = torch.tensor([S_MAX, -1, 2, 0, 3], dtype=torch.long)
    rows = torch.tensor([0, 1, ROWS_MAX, -1, 2], dtype=torch.int32)
    x = append_inputs(D, 5, 3)
    qkv = x.clone().to(dev)
    ops.kv_cache_append_(qkv, kc, vc, cos, sin, pos.to(dev), rows.to(dev), NQ, NKV, D)
    assert torch.equal(_bits(qkv[:4]), _bits(x[:4])), "an out-of-range token was modified"
    nqk = (NQ + NKV) * D
    _expect_cache(kc, {(2, 3): qkv[4, NQ * D: nqk].cpu().reshape(NKV, D)}, f"k D{D}")
    _expect_cache(vc, {(2, 3): x[4, nqk:].reshape(NKV, D)}, f"v D{D}")
    if rope:
        assert not torch.equal(_bits(qkv[4, :nqk]), _bits(x[4, :nqk])), "the valid token was not roped"
