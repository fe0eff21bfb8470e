"""Cases, float64 references and error bounds of the training attention operators flash_attn_fwd / _bwd,
their _drop, _varlen and fused-QKV forms (csrc/kernels/flash_attn.hip, dtg.ops._cpu), shared by
test_flash_attn_cpu.py (CPU operators, emulation, sensitivity) and test_flash_attn_gpu.py (the gfx950
kernels).  The references are plain torch in float64, per sequence and per head; the masks and
Philox4x32-10 are written out here, and nothing comes from the package's own ops.

Reference, per sequence (n_q queries, n_k keys, off = n_k - n_q) and query head h (kv head h // group):

    visible(i, j):  causal  j <= i + off,   window (causal calls only)  i + off - window < j
    S = scale Q K^T,   lse = log sum_visible exp S,   P = exp(S - lse),   o = (W o P) V
    W = keep * 256 / thr with dropout (keep: byte (j & 3) of word (i & 3) of Philox4x32-10(counter
    {j & ~3, s0 + (i & ~3), h, offset lo}, key {seed lo, seed hi ^ offset hi}) < thr), else 1.
    An empty key set gives lse = -inf, o = 0.
    backward, with the GIVEN o (the reference's, rounded once to bf16) and lse (rounded to f32):
    P = exp(S - lse),  delta = rowsum(dO o O),  dP = dO V^T,  dS = P o (W o dP - delta),
    dQ = scale dS K,  dK = scale dS^T Q,  dV = (W o P)^T dO;  dK, dV summed over the group's heads.
    Fused RoPE backward: _refs.rope_ref(inverse=True) on the unrounded dQ / dK.

Causal key ranges with 0 < k_len < q_len have rows without keys among rows with keys; nothing in the
project produces them and the CPU operator returns NaN there, so no case has one.

Bound (tests/_refs.py): |out - ref| <= half a bf16 ulp of ref (the single store) + term; lse is f32 and
gets the term alone.  U = 2^-24 per f32 operation on the magnitudes combined, times K = 8 (summation
order inside the MFMA, exp2 / log2 intrinsics); E = 2^-8 bounds the relative error of rounding an MFMA
operand to bf16 (8 significant bits: half an ulp is 2^-8 of a value at the bottom of its binade and 2^-9
only at the top; with 2^-9 the float64 emulation of test_flash_attn_cpu.py leaves the bound).  What the
kernel source shows, and the terms that follow (in units of U unless E):

  * scale enters late everywhere.  The MFMA accumulates the raw q.k in f32 (bf16 products are exact):
    D products and adds on sum|q k|; the forward and dQ kernels then take exp2(fma(s, c2, -m)) with
    c2 = f32(scale log2 e); the dK/dV kernel starts the accumulator at -lse / scale and takes
    exp2(s' c2).  dQ and dK are multiplied by scale once, in f32, at the store (after the split sum).
        e_ij = (D + 2) scale sum_d |q_id k_jd|
  * forward: the running max is rescaled lazily, only when a tile's max exceeds it by 2^8, so the
    unnormalised P is at most 2^8 when it is rounded to bf16 -- the same relative error E -- and the
    exponent's roundoff is on |s - m| + 8 ln 2 instead of |s - m|.  l is summed from the UNROUNDED P (and
    counts dropped entries), so E appears in the numerator only:
        rel_ij = e_ij + 2 (|s_ij - m_i| + 8 ln 2) + 2
        o_ic:  E sum_j w p |v_jc|  +  K U [sum_j w p |v_jc| (rel_ij + n_k + 2) + |o_ic| (sum_j p rel_ij + n_k + 2)]
               + 2^8 2^-126 sum_j |v_jc|   (a P below the smallest normal bf16 may be flushed)
    lse = (m + log2 l) ln 2 : l's relative error is lse's absolute error; m, log2 l and the product round
    on at most 3 (max|s| + 8 ln 2 + ln n_k + 1):
        lse_i: K U [sum_j p rel_ij + n_k + 1 + 3 (max_j |s_ij| + 8 ln 2 + ln n_k + 1)]
  * backward: P = exp2(s c2 - lse log2 e); in the dK/dV kernel the accumulator carries -lse / scale
    through D / 16 MFMA steps, so lse's magnitude is rounded with the sum:
        relp_ij = (D + 2)(scale sum|q k| + |lse_i|) + 2 |lse_i| + 2 |s_ij - lse_i| + 2
    delta is reduced in f32 in the dQ kernel's prologue: 8 sequential products per 16-byte chunk, then a
    butterfly over the row's D / 8 lanes, written to memory and read back by the dK/dV kernel, whose dP
    accumulator starts at -delta.  dP - delta cancels, so its error is absolute:
        eg_ij = (D + 1) w sum|dO v| + (2 D + 2) sum|dO o| + w |dP_ij| + |delta_i|
        err(dS_ij / scale) = p_ij (eg_ij + |w dP - delta| (relp_ij + 2))
    dS / scale and the (dropped, rescaled) P are rounded to bf16 as MFMA operands:
        dQ_ic: scale [E sum_j |dS||k_jc| + K U (sum_j err_ij |k_jc| + (n_k + 2) sum_j |dS||k_jc|)]
        dK_jc: scale [E sum_hi |dS||q_ic| + K U (sum_hi err_ij |q_ic| + (G n_q + 10) sum_hi |dS||q_ic|)]
        dV_jc: E sum_hi w p |dO_ic| + K U sum_hi w p |dO_ic| (relp_ij + G n_q + 10)
    sums over the group's G heads h and the queries i; the 10 holds the up to 8 f32 partials of the split
    dK/dV path (bwd_kv_combine_kernel adds them in split order) and the final products.
  * fused RoPE backward: the rotation is linear, so a term t of the unrotated gradient becomes
    |cos| t_1 + |sin| t_2, plus rope_ref's own f32 term.  The kernels rotate in f32 before the single
    store, with one exception the source states: on the split dK/dV path the combine kernel stores bf16
    dK and a separate rope pass rotates it, so dK is rounded twice; there (and only there) the half ulp
    of the stored unrotated dK (taken at |dK| plus its own bound, so a value pushed into the next binade
    is covered), rotated the same way, is added to dK's term (`dk_chained`).
  * window = 1 leaves only the diagonal: P = 1, o = v, so dP - delta is exactly 0 in the reference and
    dQ = dK = 0.  The kernels form dP (MFMA) and delta (VALU) as two f32 sums of the same products in
    different orders, so their zero is not exact; they are held to the absolute eg term alone, and the
    exact zero is asserted of the reference.

max_outlier_share is 0 everywhere.  Nothing here comes from a run of the code under test.
"""
import functools
import math
import os

import numpy as np
import torch

import dtg.ops  # noqa: F401  (defines torch.ops.dtg)
from _refs import K, TINY, U, assert_within, bf16_ulp, f64, rope_ref, round_bf16

E = 2.0 ** -8
LN2_8 = 8.0 * math.log(2.0)
PACK_A = (0, 1, 2, 31, 32, 33, 0, 63, 64, 65, 127, 128, 129, 0)
PACK_B = (0, 191, 193, 0, 257, 1, 0)
MAX_POS = 272

# Random123 known answers (kat_vectors): counter, key -> Philox4x32-10 output
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox(c, key):
    """Philox4x32-10 on four uint64 numpy arrays of 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m for x in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def drop_thr(p):
    return max(1, min(256, int(math.floor((1.0 - p) * 256.0 + 0.5))))


def keep_mask(seed, offset, head, s0, nq, nk, p):
    """bool [nq, nk] of fa::DropCfg's counter layout."""
    i = np.arange(nq, dtype=np.uint64)[:, None] + np.zeros((1, nk), dtype=np.uint64)
    j = np.arange(nk, dtype=np.uint64)[None, :] + np.zeros((nq, 1), dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    w = philox([j & ~np.uint64(3), np.uint64(s0) + (i & ~np.uint64(3)), np.full_like(i, head),
                np.full_like(i, offset & 0xFFFFFFFF)], (seed & 0xFFFFFFFF, (seed >> 32) ^ (offset >> 32)))
    word = np.choose((i & np.uint64(3)).astype(np.int64), w)
    byte = (word >> (np.uint64(8) * (j & np.uint64(3)))) & np.uint64(255)
    return torch.from_numpy(byte.astype(np.int64) < drop_thr(p))


def visible(nq, nk, causal, window, mut=None):
    i = torch.arange(nq)[:, None]
    j = torch.arange(nk)[None, :]
    off = nk - nq
    vis = torch.ones(nq, nk, dtype=torch.bool)
    if causal:
        vis = j <= i + off + (1 if mut == "causal_off1" else 0)
        if window > 0:
            vis = vis & (i + off - window + {"win_lo": -1, "win_hi": 1}.get(mut, 0) < j)
    if mut == "last_key" and nk > 1:
        vis = vis.clone()
        vis[:, -1] = False
    return vis


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _c(D, hq, hkv, lens, causal=True, window=0, q_scale=1.0, kr=None, Tk=None, drop=None, rope=False):
    return dict(D=D, hq=hq, hkv=hkv, lens=tuple(lens), causal=causal, window=window, q_scale=q_scale, kr=kr, Tk=Tk,
                drop=drop, rope=rope)


CASES = {}
for _p, _lens in (("A", PACK_A), ("B", PACK_B)):
    for _causal in (True, False):
        CASES[f"edge_{_p}_{'c' if _causal else 'nc'}_d128"] = _c(128, 4, 2, _lens, _causal)
        CASES[f"edge_{_p}_{'c' if _causal else 'nc'}_d64"] = _c(64, 4, 4, _lens, _causal)
EDGE = [n for n in CASES]
for _hq, _hkv, _D in ((4, 4, 128), (4, 2, 64), (6, 2, 64), (8, 1, 128), (3, 1, 64)):
    CASES[f"heads_{_hq}_{_hkv}"] = _c(_D, _hq, _hkv, (0, 33, 130, 65))
HEADS = [n for n in CASES if n.startswith("heads")]
for _i, _w in enumerate((1, 2, 63, 64, 65, 128, 129, 1000)):
    CASES[f"window_{_w}"] = _c((128, 64)[_i % 2], 4, (2, 4)[_i % 2], (1, 64, 65, 129, 257), window=_w)
CASES["window_64_noncausal"] = _c(64, 4, 4, (1, 64, 65, 129, 257), causal=False, window=64)
WINDOW = [n for n in CASES if n.startswith("window_") and n[7:].isdigit()]
CASES["logit_c"] = _c(128, 4, 2, (257, 65), q_scale=8.0)
CASES["logit_nc"] = _c(64, 4, 4, (257, 65), causal=False, q_scale=8.0)
LOGIT = ["logit_c", "logit_nc"]
# the entries parallel/context_parallel.py::cp_ranges produces: "diag" (causal, k_len == q_len) and "off"
# (non-causal); gaps between the ranges, k / v longer than every range
CASES["kr_diag"] = _c(128, 4, 2, (33, 0, 128, 65), kr=((3, 33), (40, 0), (50, 128), (200, 65)), Tk=300)
CASES["kr_off"] = _c(64, 4, 2, (33, 33, 128, 0, 128, 33, 0, 128), causal=False,
                     kr=((2, 0), (5, 1), (10, 64), (80, 200), (290, 200), (500, 64), (570, 0), (580, 0)), Tk=600)
KR = ["kr_diag", "kr_off"]
for _p in (0.0, 0.1, 0.5, 0.999):
    for _causal in (True, False):
        for _D in (64, 128):
            CASES[f"drop_{_p}_{'c' if _causal else 'nc'}_d{_D}"] = _c(
                _D, 4, (4, 2)[_D == 128], (1, 33, 130), _causal,
                drop=(_p, 0x123456789AB, 77 + ((1 << 32) if _p == 0.5 else 0)))
DROP = [n for n in CASES if n.startswith("drop_")]
CASES["rope_A_d128"] = _c(128, 4, 2, PACK_A, rope=True)
CASES["rope_B_d64"] = _c(64, 4, 4, PACK_B, rope=True)
CASES["rope_window"] = _c(128, 4, 2, (1, 64, 65, 129, 257), window=65, rope=True)
ROPE = ["rope_A_d128", "rope_B_d64", "rope_window"]


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def tables(D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    return fr.cos().float().contiguous(), fr.sin().float().contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's CPU bf16 tensors: q [T, hq, D], k / v [Tk, hkv, D], dO [T, hq, D] (distinct data per head)."""
    c = dict(CASES[name], name=name)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    T = sum(c["lens"])
    Tk = c["Tk"] or T
    c.update(T=T, Tk=Tk, G=c["hq"] // c["hkv"], scale=c["D"] ** -0.5, cu=_cu(c["lens"]),
             q=(torch.randn(T, c["hq"], c["D"], generator=g) * c["q_scale"]).to(torch.bfloat16),
             k=torch.randn(Tk, c["hkv"], c["D"], generator=g).to(torch.bfloat16),
             v=torch.randn(Tk, c["hkv"], c["D"], generator=g).to(torch.bfloat16),
             do=torch.randn(T, c["hq"], c["D"], generator=g).to(torch.bfloat16))
    if c["rope"]:
        c["pos"] = torch.cat([torch.arange(n) for n in c["lens"]]).long()  # restart per sequence
    return c


def _ranges(c, mut=None):
    cu = c["cu"].tolist()
    out = []
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        ka, n = (a, b - a) if c["kr"] is None else c["kr"][s]
        if mut == "kstart_off1" and n:
            ka = min(ka + 1, c["Tk"] - n)
        out.append((a, b, ka, ka + n))
    return out


def _rot_abs(t, cos, sin, pos, nheads, D):
    """A term of the unrotated gradient after the (linear) rotation: |cos| t1 + |sin| t2 on the pairs."""
    T, half = t.shape[0], D // 2
    v = t[:, : nheads * D].reshape(T, nheads, D)
    c, s = f64(cos)[pos][:, None, :].abs(), f64(sin)[pos][:, None, :].abs()
    t1, t2 = v[..., :half], v[..., half:]
    out = t.clone()
    out[:, : nheads * D] = torch.cat([c * t1 + s * t2, c * t2 + s * t1], -1).reshape(T, nheads * D)
    return out


def reference(c, mut=None, emulate=False, given=None):
    """o, lse, dq, dk, dv (float64, unrounded), their terms, and the rounded o / lse the backward was
    given.  `mut`: one deliberate mistake (the sensitivity test).  `emulate`: P and dS rounded to bf16
    where the kernels pack them.  `given`: (o bf16, lse f32) to differentiate at instead of the reference's."""
    D, hq, hkv, G, scale = c["D"], c["hq"], c["hkv"], c["G"], c["scale"]
    T, Tk = c["T"], c["Tk"]
    window = c["window"] if c["causal"] else 0
    kvmap = [(h % hkv) if mut == "head_order" else h // G for h in range(hq)]
    q, k, v, do = f64(c["q"]), f64(c["k"]), f64(c["v"]), f64(c["do"])
    r = {n: torch.zeros(T, hq, D, dtype=torch.float64) for n in ("o", "o_t", "dq", "dq_t")}
    r.update({n: torch.zeros(Tk, hkv, D, dtype=torch.float64) for n in ("dk", "dk_t", "dv", "dv_t")})
    r["lse"] = torch.full((hq, T), float("-inf"), dtype=torch.float64)
    r["lse_t"] = torch.zeros(hq, T, dtype=torch.float64)
    sc = 1.0
    if c["drop"]:
        sc = 256.0 / drop_thr(c["drop"][0])
    seqs = []
    for a, b, ka, kb in _ranges(c, mut):
        nq, nk = b - a, kb - ka
        if nq == 0 or nk == 0:
            seqs.append(None)
            continue
        Q, dO = q[a:b].transpose(0, 1), do[a:b].transpose(0, 1)                  # [hq, nq, D]
        Kh, Vh = k[ka:kb].transpose(0, 1)[kvmap], v[ka:kb].transpose(0, 1)[kvmap]  # [hq, nk, D]
        vis = visible(nq, nk, c["causal"], window, mut)
        assert vis.any(-1).all(), "a row without keys among rows with keys"
        W = torch.ones(hq, nq, nk, dtype=torch.float64)
        if c["drop"]:
            p_, seed, off = c["drop"]
            s0 = 0 if mut == "drop_s0" else a
            W = torch.stack([keep_mask(seed, off, h, s0, nq, nk, p_) for h in range(hq)]).double() * sc
            if mut == "drop_shift":
                W = torch.roll(W, 1, -1)
        S = scale * Q @ Kh.transpose(1, 2)
        Sabs = scale * Q.abs() @ Kh.abs().transpose(1, 2)
        Sm = S.masked_fill(~vis, float("-inf"))
        m = Sm.amax(-1, keepdim=True)
        lse = torch.logsumexp(Sm, -1)
        P = torch.exp(Sm - lse[..., None])
        rel = torch.where(vis, (D + 2) * Sabs + 2 * ((S - m).abs() + LN2_8) + 2, torch.zeros_like(S))
        if emulate:
            pu = torch.exp(Sm - m)
            o = (round_bf16(pu * (W != 0)) @ Vh) * sc / pu.sum(-1, keepdim=True)
        else:
            o = (P * W) @ Vh
        smax = S.abs().masked_fill(~vis, 0).amax(-1)
        prel = (P * rel).sum(-1)
        r["o"][a:b] = o.transpose(0, 1)
        r["o_t"][a:b] = (E * ((P * W) @ Vh.abs()) + 256 * TINY * Vh.abs().sum(1, keepdim=True)
                         + K * U * ((P * W * (rel + nk + 2)) @ Vh.abs() + o.abs() * (prel[..., None] + nk + 2))).transpose(0, 1)
        r["lse"][:, a:b] = lse
        r["lse_t"][:, a:b] = K * U * (prel + nk + 1 + 3 * (smax + LN2_8 + math.log(nk) + 1))
        seqs.append((a, b, ka, kb, Q, dO, Kh, Vh, vis, W, S, Sabs))
    if given is None:
        r["o_in"], r["lse_in"] = round_bf16(r["o"]).to(torch.bfloat16), r["lse"].float()
    else:
        r["o_in"], r["lse_in"] = given
    og_all, lg_all = f64(r["o_in"]), f64(r["lse_in"])
    for sq in seqs:
        if sq is None:
            continue
        a, b, ka, kb, Q, dO, Kh, Vh, vis, W, S, Sabs = sq
        nq, nk = b - a, kb - ka
        og, lg = og_all[a:b].transpose(0, 1), lg_all[:, a:b, None]
        P = torch.where(vis, torch.exp(S - lg), torch.zeros_like(S))
        dP = dO @ Vh.transpose(1, 2)
        A = dO.abs() @ Vh.abs().transpose(1, 2)
        delta = (dO * og).sum(-1, keepdim=True)
        B = (dO * og).abs().sum(-1, keepdim=True)
        if mut == "delta_neighbour":
            delta = torch.roll(delta, -1, 1)
        g = W * dP - delta
        dS = P * g
        relp = torch.where(vis, (D + 2) * (Sabs + lg.abs()) + 2 * lg.abs() + 2 * (S - lg).abs() + 2, torch.zeros_like(S))
        err = P * ((D + 1) * W * A + (2 * D + 2) * B + W * dP.abs() + delta.abs() + g.abs() * (relp + 2))
        Pw = P * (W != 0) if mut == "dv_rescale" else P * W
        dSq, dSk, Pv = dS, dS, Pw
        if emulate:
            dSq = dSk = round_bf16(dS)
            Pv = round_bf16(Pw)
        r["dq"][a:b] = (scale * dSq @ Kh).transpose(0, 1)
        dq_abs = scale * dS.abs() @ Kh.abs()
        r["dq_t"][a:b] = (E * dq_abs + K * U * (scale * err @ Kh.abs() + (nk + 2) * dq_abs)).transpose(0, 1)
        rows = torch.ones(nq, 1, dtype=torch.float64)
        if mut == "kv_item_row":
            rows[31::32] = 0
        heads = [h for h in range(hq) if not (mut == "gqa_head" and G > 1 and h % G == G - 1)]
        cnt = G * nq + 10
        dk_h = scale * (dSk * rows).transpose(1, 2) @ Q * (scale if mut == "dk_scale2" else 1.0)
        dv_h = (Pv * rows).transpose(1, 2) @ dO
        dk_abs = scale * dS.abs().transpose(1, 2) @ Q.abs()
        dk_t = E * dk_abs + K * U * (scale * err.transpose(1, 2) @ Q.abs() + cnt * dk_abs)
        dv_t = E * (Pw.transpose(1, 2) @ dO.abs()) + K * U * ((Pw * (relp + cnt)).transpose(1, 2) @ dO.abs())
        for h in range(hq):
            kh = kvmap[h]
            if h in heads:
                r["dk"][ka:kb, kh] += dk_h[h]
                r["dv"][ka:kb, kh] += dv_h[h]
            r["dk_t"][ka:kb, kh] += dk_t[h]
            r["dv_t"][ka:kb, kh] += dv_t[h]
    r["dk_chain"] = None
    if c["rope"]:
        cos, sin = tables(D)
        for n, nh in (("dq", hq), ("dk", hkv)):
            flat, t = r[n].reshape(-1, nh * D), r[n + "_t"].reshape(-1, nh * D)
            if n == "dk":
                # half an ulp of the STORED unrotated dK, which may lie one binade above the reference's:
                # the ulp is taken at the largest magnitude the bound lets it have
                top = flat.abs() + t + 0.5 * bf16_ulp(flat)
                r["dk_chain"] = _rot_abs(0.5 * bf16_ulp(top), cos, sin, c["pos"], nh, D).reshape(-1, nh, D)
            out, rt = rope_ref(flat, cos, sin, c["pos"], nh, D, mut != "rope_sign")
            r[n] = out.reshape(-1, nh, D)
            r[n + "_t"] = (rt + _rot_abs(t, cos, sin, c["pos"], nh, D)).reshape(-1, nh, D)
    return r


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Inputs and reference of one case; computed once, shared, never modified."""
    c = dict(inputs(name))
    c["ref"] = reference(c)
    return c


# ---------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def planned_nsplit(c, kv_split, max_seqlen):
    """The dK/dV split the launch plan takes (flash_attn_plan.h); decides only where the documented second
    rounding of the fused-RoPE dK applies."""
    if (c["causal"] and c["window"]) or c["kr"] is not None:
        return 1
    if not c["drop"] and os.environ.get("DTG_FA_KV_PF") == "2":  # read when the extension loads
        return 1
    if kv_split > 0:
        return min(8, kv_split)
    wgs = c["hkv"] * len(c["lens"]) * -(-max_seqlen // 128)
    return min(4, -(-512 // wgs)) if 0 < wgs < 512 else 1


def compare(c, r, outs, family, dk_chained=False):
    """Every output of `outs` against the reference r, one assert_within per sequence (a short sequence
    cannot hide); a failure names the case, the output, the sequence and the index inside it:
    (row, head, column) for o / dq / dk / dv, (head, row) for lse."""
    for s, (a, b, ka, kb) in enumerate(_ranges(c)):
        for n, out in outs.items():
            lo, hi = (ka, kb) if n in ("dk", "dv") else (a, b)
            if hi == lo:
                continue
            name = f"{family}|{n}|{c['name']} seq {s}"
            if n == "lse":
                o_, ref, t = out[:, lo:hi], r["lse"][:, lo:hi], r["lse_t"][:, lo:hi]
                noinf = torch.isneginf(ref)
                assert torch.equal(torch.isneginf(f64(o_)), noinf), f"{name}: -inf rows differ"
                if noinf.all():
                    continue
                assert not noinf.any()
            else:
                o_, ref, t = out[lo:hi], r[n][lo:hi], r[n + "_t"][lo:hi]
                if n == "dk" and dk_chained:
                    t = t + r["dk_chain"][lo:hi]
            assert_within(o_, ref, t, name)
    if c["kr"] is not None:  # rows with no keys: exact; keys outside every range: exactly zero
        outside = torch.ones(c["Tk"], dtype=torch.bool)
        for a, b, ka, kb in _ranges(c):
            outside[ka:kb] = False
            if kb == ka and b > a:
                for n in ("o", "dq"):
                    if n in outs:
                        assert not _bits(outs[n][a:b]).any(), f"{family} {c['name']}: {n} of rows without keys is not 0"
        for n in ("dk", "dv"):
            if n in outs:
                assert not _bits(outs[n])[outside].any(), f"{family} {c['name']}: {n} outside every key range is not 0"


def _qkv_on(c, dev, layout):
    """q, k, v on `dev` in one of the token-stride layouts: 'pad8' (8 extra elements per token) or 'fused'
    (views of one [T, (hq + 2 hkv) D] tensor, also returned)."""
    T, hq, hkv, D = c["T"], c["hq"], c["hkv"], c["D"]
    if c["kr"] is not None:
        qb = torch.zeros(T, hq * D + 8, dtype=torch.bfloat16)
        qb[:, : hq * D] = c["q"].reshape(T, -1)
        return qb.to(dev)[:, : hq * D].view(T, hq, D), c["k"].to(dev), c["v"].to(dev), None
    W = (hq + 2 * hkv) * D
    base = torch.zeros(T, W + (8 if layout == "pad8" else 0), dtype=torch.bfloat16)
    base[:, :W] = torch.cat([c["q"].reshape(T, -1), c["k"].reshape(T, -1), c["v"].reshape(T, -1)], 1)
    base = base.to(dev)
    view = lambda h0, nh: base[:, h0 * D: (h0 + nh) * D].view(T, nh, D)  # noqa: E731
    return view(0, hq), view(hq, hkv), view(hq + hkv, hkv), base


def _kr(c, dev):
    ks = torch.tensor([x[0] for x in c["kr"]], dtype=torch.int32, device=dev)
    kl = torch.tensor([x[1] for x in c["kr"]], dtype=torch.int32, device=dev)
    return ks, kl, max(x[1] for x in c["kr"])


def _rng(c, dev):
    return torch.tensor([c["drop"][1], c["drop"][2]], dtype=torch.int64, device=dev)


def run_fwd(c, dev, layout="pad8", max_seqlen=None):
    ops = torch.ops.dtg
    q, k, v, _ = _qkv_on(c, dev, layout)
    ms = max_seqlen or max(c["lens"])
    cu = c["cu"].to(dev)
    if c["kr"] is not None:
        ks, kl, mk = _kr(c, dev)
        return ops.flash_attn_varlen_fwd(q, k, v, cu, ks, kl, ms, mk, c["scale"], c["causal"])
    if c["drop"]:
        return ops.flash_attn_fwd_drop(q, k, v, cu, ms, c["scale"], c["causal"], c["drop"][0], _rng(c, dev))
    return ops.flash_attn_fwd(q, k, v, cu, ms, c["scale"], c["causal"], c["window"])


def run_bwd(c, dev, layout="pad8", max_seqlen=None, given=None):
    """dq, dk, dv [*, H, D] of the raw backward operator at the reference's rounded o and lse: the separate
    q / k / v form for 'pad8', the fused-QKV form (and the _rope / _drop fused forms) for 'fused'."""
    ops = torch.ops.dtg
    r = c["ref"]
    q, k, v, base = _qkv_on(c, dev, layout)
    ms = max_seqlen or max(c["lens"])
    cu, do = c["cu"].to(dev), c["do"].to(dev)
    o, lse = (r["o_in"], r["lse_in"]) if given is None else given
    o, lse = o.to(dev), lse.to(dev)
    hq, hkv, D, T = c["hq"], c["hkv"], c["D"], c["T"]
    if c["kr"] is not None:
        ks, kl, mk = _kr(c, dev)
        return ops.flash_attn_varlen_bwd(do, q, k, v, o, lse, cu, ks, kl, ms, mk, c["scale"], c["causal"])
    if layout == "fused" or c["rope"]:
        if c["rope"]:
            cos, sin = (t.to(dev) for t in tables(D))
            dqkv = ops.flash_attn_bwd_qkv_rope(do, base, hq, hkv, D, o, lse, cu, ms, c["scale"], c["causal"], cos, sin,
                                               c["pos"].to(dev), c["window"])
        elif c["drop"]:
            dqkv = ops.flash_attn_bwd_qkv_drop(do, base, hq, hkv, D, o, lse, cu, ms, c["scale"], c["causal"],
                                               c["drop"][0], _rng(c, dev))
        else:
            dqkv = ops.flash_attn_bwd_qkv(do, base, hq, hkv, D, o, lse, cu, ms, c["scale"], c["causal"], c["window"])
        assert dqkv.shape == (T, (hq + 2 * hkv) * D)
        return (dqkv[:, : hq * D].reshape(T, hq, D), dqkv[:, hq * D: (hq + hkv) * D].reshape(T, hkv, D),
                dqkv[:, (hq + hkv) * D:].reshape(T, hkv, D))
    if c["drop"]:
        return ops.flash_attn_bwd_drop(do, q, k, v, o, lse, cu, ms, c["scale"], c["causal"], c["drop"][0], _rng(c, dev))
    return ops.flash_attn_bwd(do, q, k, v, o, lse, cu, ms, c["scale"], c["causal"], c["window"])


def check_fwd(c, dev, family, layout="pad8", max_seqlen=None):
    o, lse = run_fwd(c, dev, layout, max_seqlen)
    assert o.shape == (c["T"], c["hq"], c["D"]) and o.dtype == torch.bfloat16
    assert lse.shape == (c["hq"], c["T"]) and lse.dtype == torch.float32
    compare(c, c["ref"], {"o": o, "lse": lse}, family)
    return o, lse


def check_bwd(c, dev, family, layout="pad8", max_seqlen=None, kv_split=0):
    dq, dk, dv = run_bwd(c, dev, layout, max_seqlen)
    chained = (c["rope"] and torch.device(dev).type != "cpu"
               and planned_nsplit(c, kv_split, max_seqlen or max(c["lens"])) > 1)
    compare(c, c["ref"], {"dq": dq, "dk": dk, "dv": dv}, family, dk_chained=chained)
    return dq, dk, dv


def check_case(name, dev, family, layout="pad8", max_seqlen=None):
    c = make_case(name)
    check_fwd(c, dev, family, layout, max_seqlen)
    check_bwd(c, dev, family, layout, max_seqlen)


def check_edge_pack(dev, family="edge"):
    """The edge-length packs in both layouts and grid heights (what the env-knob child process runs)."""
    for name in EDGE:
        check_case(name, dev, family, "pad8", None)
        check_case(name, dev, family, "fused", 300)


def check_tuning(name, dev, knobs):
    """Backward under every (kv_split, kv_qb): within the bound, reproducible, dQ independent of the knobs."""
    from dtg import ops

    c = make_case(name)
    dq0 = None
    for split, qb in knobs:
        with ops.fa_tuning(dev, kv_split=split, kv_qb=qb):
            a = check_bwd(c, dev, f"tuning split{split} qb{qb}", "pad8", None, kv_split=split)
            b = run_bwd(c, dev, "pad8")
        for x, y, n in zip(a, b, ("dq", "dk", "dv")):
            assert torch.equal(_bits(x), _bits(y)), f"{name} split {split} qb {qb}: {n} not reproducible"
        dq0 = a[0] if dq0 is None else dq0
        assert torch.equal(_bits(a[0]), _bits(dq0)), f"{name} split {split} qb {qb}: dq depends on the dK/dV knobs"


def check_window_identities(dev):
    """window = 1: only the diagonal is visible, so the reference's dQ and dK are exactly zero and the
    outputs are held to the absolute cancellation term alone (the kernel's dP and delta are two f32 sums of
    the same products in different orders, so its own zero is not exact).  A window on a non-causal call
    has no effect: bit for bit the un-windowed result."""
    r = make_case("window_1")["ref"]
    assert not r["dq"].any() and not r["dk"].any()
    cw = make_case("window_64_noncausal")
    cp = dict(cw, window=0)  # the same data
    for x, y in zip(run_fwd(cw, dev) + run_bwd(cw, dev), run_fwd(cp, dev) + run_bwd(cp, dev)):
        assert torch.equal(_bits(x), _bits(y)), "a window changed a non-causal call"


def check_drop(name, dev, splits=(1, 3)):
    from dtg import ops

    c = make_case(name)
    check_fwd(c, dev, "dropout")
    for s in splits:
        with ops.fa_tuning(dev, kv_split=s):
            check_bwd(c, dev, f"dropout split{s}", kv_split=s)


def check_p0_is_plain(dev):
    """p = 0 (thr = 256, every byte kept) against the reference computed WITHOUT dropout."""
    c = dict(make_case("drop_0.0_c_d64"))
    plain = dict(c, drop=None)
    plain["ref"] = reference(plain)
    o, lse = run_fwd(c, dev)
    compare(plain, plain["ref"], {"o": o, "lse": lse}, "dropout p0")
    dq, dk, dv = run_bwd(c, dev)
    compare(plain, plain["ref"], {"dq": dq, "dk": dk, "dv": dv}, "dropout p0")


def check_mask_probes(dev, D=64, p=0.5, splits=(1, 3)):
    """The kernels' keep decisions read bit for bit.  Sequences of n <= D keys, the probed one second in the
    pack (s0 = 5), MHA with 3 heads.  q = 0 makes P uniform over the visible keys.
      forward: v_j = e_j                      ->  o_ij  = keep_ij (256 / thr) / nvis_i
      dK/dV:   dO_i = e_i                     ->  dV_ji = keep_ij (256 / thr) / nvis_i
      dQ:      k_j = e_j, o = 0, dO_i = e_0, v_j0 = 1  (dP = 1, delta = 0)  ->  dQ_ij = scale keep_ij (256 / thr) / nvis_i
    Each element is classified at half the kept value and compared with the reference mask by torch.equal."""
    from dtg import ops

    ot = torch.ops.dtg
    H, lens, seed, off = 3, (5, 40, 61), 0xABCDEF0123, 9 + (1 << 33)
    T, cu, scale = sum(lens), _cu(lens), D ** -0.5
    thr = drop_thr(p)
    rng = torch.tensor([seed, off], dtype=torch.int64, device=dev)
    eye = torch.zeros(T, H, D)
    for a, n in zip(cu.tolist(), lens):
        eye[a:a + n] = torch.eye(n, D)[:, None, :]
    eye = eye.to(torch.bfloat16).to(dev)
    zero = torch.zeros(T, H, D, dtype=torch.bfloat16, device=dev)
    col0 = zero.clone()
    col0[:, :, 0] = 1
    g = torch.Generator().manual_seed(5)
    rnd = torch.randn(T, H, D, generator=g).to(torch.bfloat16).to(dev)
    for causal in (True, False):
        want, kept_val, lse = [], [], torch.zeros(H, T)
        for s, (a, n) in enumerate(zip(cu.tolist(), lens)):
            vis = visible(n, n, causal, 0)
            nvis = vis.sum(-1, keepdim=True).double()
            want.append(torch.stack([keep_mask(seed, off, h, a, n, n, p) & vis for h in range(H)]))
            kept_val.append((256.0 / thr) / nvis)
            lse[:, a:a + n] = torch.log(nvis)[:, 0].float()
        lse = lse.to(dev)
        cud = cu.to(dev)

        def read(x, s, transpose, mul=1.0):  # [n, H, n] block of sequence s -> bool [H, n, n] (query, key)
            a, n = cu.tolist()[s], lens[s]
            blk = f64(x[a:a + n, :, :n]).permute(1, 2, 0) if transpose else f64(x[a:a + n, :, :n]).permute(1, 0, 2)
            assert not f64(x[a:a + n, :, n:]).any(), "columns past the sequence are not zero"
            return blk > 0.5 * mul * kept_val[s]

        what = f"causal {causal}"
        o, _ = ot.flash_attn_fwd_drop(zero, rnd, eye, cud, max(lens), scale, causal, p, rng)
        for s in range(len(lens)):
            assert torch.equal(read(o, s, False), want[s]), f"forward keep mask differs, seq {s}, {what}"
        for split in splits:
            with ops.fa_tuning(dev, kv_split=split, kv_qb=64):
                _, _, dv = ot.flash_attn_bwd_drop(eye, zero, rnd, rnd, rnd, lse, cud, max(lens), scale, causal, p, rng)
                dq, _, _ = ot.flash_attn_bwd_drop(col0, zero, eye, col0, zero, lse, cud, max(lens), scale, causal, p, rng)
            for s in range(len(lens)):
                assert torch.equal(read(dv, s, True), want[s]), f"dK/dV keep mask differs, seq {s}, split {split}, {what}"
                assert torch.equal(read(dq, s, False, scale), want[s]), f"dQ keep mask differs, seq {s}, split {split}, {what}"


def check_public_attention(name, dev):
    """ops.attention on the fused layout: o against the reference; its autograd backward bit for bit the raw
    operators' (which check_case holds to the reference) at the forward's own o and lse."""
    from dtg import ops

    c = make_case(name)
    _, _, _, base = _qkv_on(c, dev, "fused")
    x = base.clone().requires_grad_(True)
    out = ops.attention(x, c["hq"], c["hkv"], c["D"], c["cu"].to(dev), max(c["lens"]), causal=c["causal"], window=c["window"])
    compare(c, c["ref"], {"o": out.view(c["T"], c["hq"], c["D"])}, "public")
    out.backward(c["do"].to(dev).reshape(c["T"], -1))
    o, lse = run_fwd(c, dev, "fused")
    assert torch.equal(_bits(out), _bits(o.reshape(c["T"], -1)))
    dq, dk, dv = run_bwd(c, dev, "fused", given=(o, lse))
    assert torch.equal(_bits(x.grad), _bits(torch.cat([dq.reshape(c["T"], -1), dk.reshape(c["T"], -1), dv.reshape(c["T"], -1)], 1)))
    # and at its own o / lse the backward meets the reference's bound too
    r = reference(c, given=(o.cpu(), lse.cpu()))
    compare(c, r, {"dq": dq, "dk": dk, "dv": dv}, "public")


def check_refusals_and_empties(dev):
    import pytest

    ot = torch.ops.dtg
    D, H = 64, 2
    bf = dict(dtype=torch.bfloat16, device=dev)
    e3, elz = torch.empty(0, H, D, **bf), torch.empty(H, 0, device=dev)
    cu1 = torch.zeros(1, dtype=torch.int32, device=dev)
    o, lse = ot.flash_attn_fwd(e3, e3, e3, cu1, 0, 0.125, True, 0)
    assert o.shape == (0, H, D) and lse.shape == (H, 0)
    for g in ot.flash_attn_bwd(e3, e3, e3, e3, e3, elz, cu1, 0, 0.125, True, 0):
        assert g.shape == (0, H, D)
    # tokens but nseq = 0 / max_seqlen = 0: zero gradients, no launch
    x = torch.randn(4, H, D).to(**bf)
    l4 = torch.zeros(H, 4, device=dev)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    # (the CPU operators ignore max_seqlen, so the max_seqlen = 0 form is the kernels' alone)
    for cu_, ms in ((cu1, 4), (cu, 0))[: 1 if torch.device(dev).type == "cpu" else 2]:
        o, lse = ot.flash_attn_fwd(x, x, x, cu_, ms, 0.125, True, 0)
        assert o.shape == (4, H, D) and lse.shape == (H, 4)
        for g in ot.flash_attn_bwd(x, x, x, x, x, l4, cu_, ms, 0.125, True, 0):
            assert g.shape == (4, H, D) and not _bits(g).any()
    # The fa::conflict combinations (rope with key ranges or dropout, dropout with a window) have no
    # operator that could express them -- the plan header's native check pins the rule itself -- so the
    # refusal a caller can meet is the public one.
    from dtg import ops

    qkv = torch.randn(4, 3 * H * D).to(**bf)
    cos, sin = (t.to(dev) for t in tables(D))
    for kw in (dict(window=2), dict(cos=cos, sin=sin, pos=torch.arange(4, device=dev))):
        with pytest.raises(ValueError, match="dropout"):
            ops.attention(qkv, H, H, D, cu, 4, dropout_p=0.1, **kw)
    if torch.device(dev).type != "cpu":  # the CPU operators take any width and any p
        rng = torch.tensor([1, 2], dtype=torch.int64, device=dev)
        with pytest.raises(RuntimeError, match="dropout"):
            ot.flash_attn_fwd_drop(x, x, x, cu, 4, 0.125, True, 1.0, rng)  # p outside [0, 1)
        for Dbad in (32, 96):
            y = torch.randn(4, H, Dbad).to(**bf)
            with pytest.raises(RuntimeError, match="head_dim"):
                ot.flash_attn_fwd(y, y, y, cu, 4, 0.125, True, 0)
    odd = torch.randn(4, H * D + 4).to(**bf)[:, : H * D].view(4, H, D)  # token stride not a multiple of 8
    with pytest.raises(RuntimeError, match="token stride"):
        ot.flash_attn_fwd(odd, x, x, cu, 4, 0.125, True, 0)
    with pytest.raises(RuntimeError, match="token stride"):
        ot.flash_attn_bwd(x, x, odd, x, x, l4, cu, 4, 0.125, True, 0)


def report():
    """Largest error in bf16 ulps and largest error / bound per (family, output), from _refs.RESULTS."""
    import _refs

    agg = {}
    for name, (ulps, ratio) in _refs.RESULTS.items():
        if name.count("|") < 2:
            continue
        fam, out, _ = name.split("|", 2)
        old = agg.get((fam, out), (0.0, 0.0))
        agg[(fam, out)] = (max(old[0], ulps), max(old[1], ratio))
    return agg
