"""Cases, float64 references and f32 error terms of decode_attn_multi (csrc/kernels/decode_attn.hip,
dtg.ops._cpu): Q new tokens per sequence against the KV cache, shared by test_decode_attn_multi_cpu.py and
test_decode_attn_multi_gpu.py.  The references are plain torch in float64 and use none of the package's ops.

Token (b, t) is row b * Q + t of qkv and lens and attends keys [max(0, len - window), len) of cache row
rows[b].  In a case, len of token (b, t) is first[b] + t (what a verify pass passes: pos + 1) unless the
token is listed inactive (len 0); a sequence listed under bad_rows gets a row outside the cache.  Both must
give exact zeros.

The bound is that of tests/_decode_cases.py, term for term (the per-token arithmetic is decode_attn's; see
the derivation there): half a bf16 ulp for the store plus, with U = 2^-24 and K = 8 from tests/_refs.py,

    e_j   = (D + 2) * scale * sum_i |q_i k_ji|,      rel_j = e_j + 2 |s_j - m| + 2,
    term_c = K U [ sum_j p_j |v_jc| (rel_j + n + 1) + |out_c| (sum_j p_j rel_j + n + 1) ].

At window 0 the kernel also promises the bits of decode_attn on the token alone (same max_len and splits);
check_bitwise asserts that against the operator on the same device.  Nothing here comes from a run of the
code under test."""
import functools

import torch

import dtg.ops  # noqa: F401  (defines torch.ops.dtg)
from _refs import K, U, assert_within, f64


def _c(D, nq, nkv, Q, first, splits, rows=None, rows_max=None, S_max=None, window=0, q_scale=1.0, poison=False,
       inactive=(), bad_rows=()):
    rows = list(range(len(first))) if rows is None else list(rows)
    S_max = S_max or max(8, max(first) + Q + 2)
    return dict(D=D, nq=nq, nkv=nkv, Q=Q, first=tuple(first), rows=tuple(rows), rows_max=rows_max or len(first),
                S_max=S_max, window=window, q_scale=q_scale, poison=poison, inactive=frozenset(inactive),
                bad_rows=frozenset(bad_rows), splits=tuple(splits))


CASES = {
    # token lens 62..65 and 63..66 straddle the 64-key tile, 255..258 the tile at 256; 5 splits of 258 keys
    # have 64-key chunks, so the same tokens straddle chunk edges as well
    "straddle": _c(128, 4, 2, 4, [62, 63, 255], (1, 2, 5)),
    "straddle_d64": _c(64, 8, 2, 4, [62, 63, 255], (1, 2, 5)),
    # long enough for the plan itself to split: 2 chunks of 256; 254..257 straddles the chunk edge, and the
    # second chunk is empty for the first two tokens of that sequence and for the whole last sequence
    "planned_split": _c(128, 4, 2, 4, [508, 254, 100], (0,), S_max=512),
    "planned_split_g4": _c(64, 8, 2, 5, [507, 253], (0,), S_max=512),
    "empty_splits": _c(128, 8, 2, 2, [1, 300], (5,)),
    "window": _c(128, 4, 2, 4, [300, 40, 62], (1, 3), window=64),
    "window_d64": _c(64, 2, 2, 4, [300, 40, 62], (1, 3), window=64),
    "logit_range": _c(128, 4, 1, 3, [200, 70], (1, 3), q_scale=8.0),
    "row_indirection": _c(64, 4, 2, 3, [20, 65, 130], (0, 2), rows=[4, 0, 2], rows_max=5),
    # tokens past a row's q_valid (len 0), a wholly inactive sequence and rows outside the cache
    "inactive": _c(128, 4, 2, 4, [40, 70, 20, 33, 50], (1, 2), inactive=[(0, 2), (0, 3), (1, 0), (3, 0), (3, 1), (3, 2), (3, 3)],
                   bad_rows={2: -1, 4: 5}.items()),
    "poisoned": _c(128, 4, 2, 4, [1, 300], (1, 5), poison=True),
    "poisoned_window": _c(64, 4, 2, 4, [300, 40, 62], (1, 3), rows=[3, 0, 1], rows_max=5, window=64, poison=True),
}
# every token count: one partial tile, exactly one tile, several tiles (G 4: tiles of 4 tokens; G 2: of 8)
for _Q in (1, 2, 3, 4, 5, 8, 16):
    CASES[f"Q{_Q}_G4_D64"] = _c(64, 8, 2, _Q, [62, 130], (1, 2))
    CASES[f"Q{_Q}_G2_D128"] = _c(128, 4, 2, _Q, [61, 250], (1, 2))
# every group-size (and with it query-tile) and head-dim instantiation, 3 tokens: a partial tile except at G 16
for _D in (64, 128):
    for _G in (1, 2, 3, 4, 7, 8, 16):
        CASES[f"G{_G}_D{_D}"] = _c(_D, 2 * _G, 2, 3, [37, 130], (1, 3))

RUNS = [(name, s) for name, c in CASES.items() for s in c["splits"]]


def run_id(r):
    return f"{r[0]}-splits{r[1]}"


def token_lens(c):
    return [[0 if (b, t) in c["inactive"] else f + t for t in range(c["Q"])] for b, f in enumerate(c["first"])]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Inputs (CPU, bf16) and the reference of one case; computed once, shared, never modified."""
    c = CASES[name]
    D, nq, nkv, Q, window, S_max, rows_max = c["D"], c["nq"], c["nkv"], c["Q"], c["window"], c["S_max"], c["rows_max"]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    B, G = len(c["first"]), nq // nkv
    bad = dict(c["bad_rows"])
    rows = [bad.get(b, r) for b, r in enumerate(c["rows"])]
    lens = token_lens(c)
    qkv = torch.randn(B * Q, (nq + 2 * nkv) * D, generator=g)
    qkv[:, : nq * D] *= c["q_scale"]
    qkv = qkv.to(torch.bfloat16)
    kc = torch.randn(rows_max, nkv, S_max, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(rows_max, nkv, S_max, D, generator=g).to(torch.bfloat16)
    scale = D ** -0.5

    def span(n1):
        return (max(0, n1 - window) if window else 0), n1

    if c["poison"]:  # everything outside the tokens' attended ranges, unused rows included
        keep = torch.zeros(rows_max, S_max, dtype=torch.bool)
        for b in range(B):
            for n1 in lens[b]:
                if b not in bad and n1 > 0:
                    keep[rows[b], slice(*span(n1))] = True
        kc = torch.where(keep[:, None, :, None], kc, torch.full_like(kc, float("nan")))
        vc = torch.where(keep[:, None, :, None], vc, torch.full_like(vc, float("nan")))
    ref = torch.zeros(B * Q, nq * D, dtype=torch.float64)
    term = torch.zeros(B * Q, nq * D, dtype=torch.float64)
    zero = torch.zeros(B * Q, dtype=torch.bool)
    for b in range(B):
        for t in range(Q):
            i = b * Q + t
            n0, n1 = span(lens[b][t])
            n = n1 - n0
            if b in bad or n <= 0:
                zero[i] = True
                continue
            q = f64(qkv)[i, : nq * D].reshape(nkv, G, D)
            k, v = f64(kc)[rows[b], :, n0:n1], f64(vc)[rows[b], :, n0:n1]       # [nkv, n, D]
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
    flat = [n for row in lens for n in row]
    return dict(name=name, D=D, nq=nq, nkv=nkv, G=G, B=B, Q=Q, lens=torch.tensor(flat, dtype=torch.int32),
                rows=torch.tensor(rows, dtype=torch.int32), max_len=max(flat), window=window, scale=scale,
                qkv=qkv, kc=kc, vc=vc, ref=ref, term=term, zero=zero)


def _args(c, dev):
    return tuple(c[k].to(dev) for k in ("qkv", "kc", "vc", "rows", "lens"))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _run(c, dev, splits):
    qkv, kc, vc, rows, lens = _args(c, dev)
    return torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows, lens, c["Q"], c["nq"], c["nkv"], c["D"], c["scale"],
                                           c["max_len"], c["window"], splits)


def check_multi(c, dev, splits):
    """The raw operator on `dev` against the reference; inactive tokens exactly zero; twice, bitwise equal;
    qkv untouched."""
    qkv = c["qkv"].to(dev)
    kc, vc, rows, lens = (c[k].to(dev) for k in ("kc", "vc", "rows", "lens"))
    runs = [torch.ops.dtg.decode_attn_multi(qkv, kc, vc, rows, lens, c["Q"], c["nq"], c["nkv"], c["D"], c["scale"],
                                            c["max_len"], c["window"], splits) for _ in range(2)]
    assert runs[0].shape == (c["B"] * c["Q"], c["nq"] * c["D"]) and runs[0].dtype == torch.bfloat16
    assert_within(runs[0], c["ref"], c["term"], f"decode_attn_multi {c['name']} splits {splits}")
    assert (_bits(runs[0])[c["zero"]] == 0).all(), "an inactive token's output row is not exact zeros"
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "not reproducible"
    assert torch.equal(_bits(qkv), _bits(c["qkv"])), "qkv was written"


def check_bitwise(c, dev, splits):
    """Window 0: every output row equals decode_attn on that token alone (its qkv row, rows[b], its len, the
    same max_len and splits), compared as int16 views; Q = 1: decode_attn on the batch as well."""
    assert c["window"] == 0
    qkv, kc, vc, rows, lens = _args(c, dev)
    got = _bits(_run(c, dev, splits))
    one = lambda *a: torch.ops.dtg.decode_attn(*a, c["nq"], c["nkv"], c["D"], c["scale"], c["max_len"], 0, splits)  # noqa: E731
    for b in range(c["B"]):
        for t in range(c["Q"]):
            i = b * c["Q"] + t
            alone = one(qkv[i:i + 1], kc, vc, rows[b:b + 1], lens[i:i + 1])
            assert torch.equal(got[i:i + 1], _bits(alone)), f"{c['name']} splits {splits}: token ({b}, {t}) differs from decode_attn"
    if c["Q"] == 1:
        assert torch.equal(got, _bits(one(qkv, kc, vc, rows, lens))), "Q = 1 differs from decode_attn on the batch"


BITWISE_RUNS = [r for r in RUNS if CASES[r[0]]["window"] == 0]


def check_public(c, dev, fused, splits, monkeypatch):
    """ops.decode_attention_multi through the operator and through the DTG_DECODE_FUSED=0 composition: the same
    reference, the same bound."""
    from dtg import ops
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_DECODE_FUSED", fused)
    qkv, kc, vc, rows, lens = _args(c, dev)
    out = ops.decode_attention_multi(qkv, kc, vc, rows.long(), lens, c["Q"], c["nq"], c["nkv"], c["D"], c["max_len"],
                                     window=c["window"], splits=splits)
    assert out.shape == (c["B"] * c["Q"], c["nq"] * c["D"])
    assert_within(out, c["ref"], c["term"], f"decode_attention_multi {c['name']} {'fused' if fused else 'composed'}")
    assert (_bits(out)[c["zero"]] == 0).all()


PUBLIC_CASES = ["straddle", "window", "poisoned_window", "row_indirection", "inactive", "G7_D64", "logit_range", "Q5_G4_D64"]


def check_public_errors(dev):
    import pytest

    from dtg import ops

    c = make_case("straddle")
    qkv, kc, vc, rows, lens = _args(c, dev)
    a = (c["Q"], c["nq"], c["nkv"], c["D"])
    with pytest.raises(ValueError, match="q_len"):
        ops.decode_attention_multi(qkv, kc, vc, rows, lens, 5, *a[1:], c["max_len"])
    with pytest.raises(ValueError, match="q_len"):
        ops.decode_attention_multi(qkv, kc, vc, rows, lens, 0, *a[1:], c["max_len"])
    with pytest.raises(ValueError, match="max_len"):
        ops.decode_attention_multi(qkv, kc, vc, rows, lens, *a, kc.shape[2] + 1)
    with pytest.raises(ValueError, match="caches must be"):
        ops.decode_attention_multi(qkv, kc[:, :1], vc, rows, lens, *a, 1)
    with pytest.raises(ValueError, match="rows must be an integer tensor"):
        ops.decode_attention_multi(qkv, kc, vc, rows.repeat_interleave(c["Q"]), lens, *a, c["max_len"])
    with pytest.raises(ValueError, match="rows must be an integer tensor"):
        ops.decode_attention_multi(qkv, kc, vc, rows.float(), lens, *a, c["max_len"])
    with pytest.raises(ValueError, match="lens must be an integer tensor"):
        ops.decode_attention_multi(qkv, kc, vc, rows, lens[:-1], *a, c["max_len"])
    with pytest.raises(ValueError, match="must not be negative"):
        ops.decode_attention_multi(qkv, kc, vc, rows, lens, *a, c["max_len"], window=-1)
