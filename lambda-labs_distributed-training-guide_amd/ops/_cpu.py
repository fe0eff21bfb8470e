"""CPU implementations of the `dtg` operators (plain PyTorch, f32 math).

They define the numerics the gfx950 kernels are tested against (tests compare a HIP kernel
with these on the same inputs) and they run the CPU plumbing configuration (GPT-2 / tiny
Llama on the build box).  Registered for the CPU dispatch key only.
"""
import math

import torch
import torch.nn.functional as F

from ._schema import LIB

_LOG2E = 1.4426950408889634


def rmsnorm_fwd(x, w, eps):
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
    n = (xf * rstd[:, None]).to(x.dtype)
    y = (w.float() * n.float()).to(x.dtype)
    return y, rstd


def add_rmsnorm_fwd(x, res, w, eps):
    h = (x.float() + res.float()).to(x.dtype)
    y, rstd = rmsnorm_fwd(h, w, eps)
    return y, h, rstd


def rmsnorm_bwd(dy, x, w, rstd, dres):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    n = xf * rstd[:, None]
    g = dyf * wf
    dot = (g * n).mean(-1, keepdim=True)
    dx = rstd[:, None] * (g - n * dot)
    if dres is not None:
        dx = dx + dres.float()
    dw = (dyf * n.to(x.dtype).float()).sum(0)
    return dx.to(x.dtype), dw.to(w.dtype)


def rope_(qkv, cos, sin, pos, nheads, head_dim, inverse):
    T = qkv.shape[0]
    half = head_dim // 2
    view = qkv[:, : nheads * head_dim].reshape(T, nheads, head_dim)
    x1 = view[..., :half].float()
    x2 = view[..., half:].float()
    c = cos[pos][:, None, :]
    s = sin[pos][:, None, :]
    if inverse:
        s = -s
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    qkv[:, : nheads * head_dim] = torch.cat([o1, o2], dim=-1).to(qkv.dtype).reshape(T, nheads * head_dim)


def _qk_weights(wq, wk, nq, nkv):
    """[nq + nkv, D] f32: the q weight for the q heads, the k weight for the k heads."""
    return torch.cat([wq.float()[None].expand(nq, -1), wk.float()[None].expand(nkv, -1)], 0)


def _qk_rotate(y, cos, sin, pos, inverse):
    """rope_'s rotation of [T, heads, D] f32 values (pairs (i, i + D/2)); empty tables: identity."""
    if cos.numel() == 0:
        return y
    half = y.shape[-1] // 2
    c = cos[pos][:, None, :]
    s = sin[pos][:, None, :]
    if inverse:
        s = -s
    y1, y2 = y[..., :half], y[..., half:]
    return torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], -1)


def qk_norm_rope_fwd_(qkv, wq, wk, cos, sin, pos, nq, nkv, head_dim, eps):
    """y = w * x * rsqrt(mean(x^2) + eps) per (token, head), then rope_'s rotation, all in f32 with one
    rounding on the in-place store; returns the pre-norm q|k and rstd (csrc/kernels/qk_norm.hip)."""
    T, nh, d = qkv.shape[0], nq + nkv, head_dim
    xqk = qkv[:, : nh * d].clone()
    x = xqk.float().reshape(T, nh, d)
    rstd = torch.rsqrt(x.pow(2).mean(-1) + eps)
    y = _qk_weights(wq, wk, nq, nkv) * (x * rstd[..., None])
    qkv[:, : nh * d] = _qk_rotate(y, cos, sin, pos, False).reshape(T, nh * d).to(qkv.dtype)
    return xqk, rstd


def qk_norm_rope_bwd_(dqkv, xqk, rstd, wq, wk, cos, sin, pos, nq, nkv, head_dim):
    T, nh, d = dqkv.shape[0], nq + nkv, head_dim
    dy = _qk_rotate(dqkv[:, : nh * d].float().reshape(T, nh, d), cos, sin, pos, True)
    xh = xqk.float().reshape(T, nh, d) * rstd.reshape(T, nh, 1)
    g = _qk_weights(wq, wk, nq, nkv) * dy
    dx = rstd.reshape(T, nh, 1) * (g - xh * (g * xh).mean(-1, keepdim=True))
    dw = dy * xh  # before the in-place store: for f32 inputs without rotation dy is a view of dqkv
    dqkv[:, : nh * d] = dx.reshape(T, nh * d).to(dqkv.dtype)
    return dw[:, :nq].sum((0, 1)).to(wq.dtype), dw[:, nq:].sum((0, 1)).to(wk.dtype)


def kv_cache_append_(qkv, k_cache, v_cache, cos, sin, pos, rows, nq, nkv, head_dim):
    """rope_ on the q and k heads at pos (empty tables: already roped), then k and v of every token to
    cache[rows[t], :, pos[t], :]; tokens whose pos / rows lie outside the cache (or, when roping, past
    the tables) are left untouched and write nothing (csrc/kernels/decode_attn.hip)."""
    T, d = qkv.shape[0], head_dim
    if not (k_cache.dim() == 4 and k_cache.shape == v_cache.shape and k_cache.shape[1] == nkv and k_cache.shape[3] == d):
        raise RuntimeError("dtg: kv_cache_append_: caches must be contiguous bf16 [rows_max, nkv, S_max, head_dim]")
    if not (qkv.dim() == 2 and qkv.shape[1] >= (nq + 2 * nkv) * d and pos.numel() == T and rows.numel() == T):
        raise RuntimeError("dtg: kv_cache_append_: qkv must be [T, (nq + 2 nkv) * head_dim] with one pos and row per token")
    pos, rows = pos.long(), rows.long()
    ok = (pos >= 0) & (pos < k_cache.shape[2]) & (rows >= 0) & (rows < k_cache.shape[0])
    if cos.numel():
        ok &= pos < cos.shape[0]
        sel = qkv[ok]
        rope_(sel, cos, sin, pos[ok], nq + nkv, d, False)
        qkv[ok] = sel
    k = qkv[:, nq * d:(nq + nkv) * d].reshape(T, nkv, d)
    v = qkv[:, (nq + nkv) * d:(nq + 2 * nkv) * d].reshape(T, nkv, d)
    k_cache[rows[ok], :, pos[ok]] = k[ok]
    v_cache[rows[ok], :, pos[ok]] = v[ok]


def _check_fp8_cache(name, k_cache, v_cache, k_scale, v_scale):
    if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
        raise RuntimeError(f"dtg: {name}: caches must be float8_e4m3fn tensors")
    for s in (k_scale, v_scale):
        if s.dtype != torch.float32 or s.shape != k_cache.shape[:3] or not s.is_contiguous():
            raise RuntimeError(f"dtg: {name}: scales must be contiguous f32 tensors [rows_max, nkv, S_max]")


def _e4m3_vectors(x):
    """x f32 [..., D] -> (e4m3 codes as uint8 [..., D], scale f32 [...]): one power-of-two scale per vector, the
    one that puts amax into (224, 448], read off amax's exponent bits as the append kernel does (a significand
    up to 1.75 = 448 / 256 goes to [256, 448] with 2^(E - 135), a larger one to (224, 256) with 2^(E - 134));
    floored at 2^-100, 1 for an all-zero vector.  The quotient is clamped to +-448 by comparisons, which a NaN
    passes, and rounded to nearest even by the cast."""
    amax = torch.nan_to_num(x.abs(), nan=0.0).amax(-1)
    bits = amax.view(torch.int32)
    k = (bits >> 23) - 134 - ((bits & 0x7FFFFF) <= 0x600000).to(torch.int32)
    k = torch.where(amax == 0, torch.zeros_like(k), k.clamp_min(-100)).to(torch.int32)
    scale = ((k + 127) << 23).view(torch.float32)
    q = x * ((127 - k) << 23).view(torch.float32)[..., None]
    q = torch.where(q > 448.0, 448.0, torch.where(q < -448.0, -448.0, q))
    return q.to(torch.float8_e4m3fn).view(torch.uint8), scale


def kv_cache_append_fp8_(qkv, k_cache, v_cache, k_scale, v_scale, cos, sin, pos, rows, nq, nkv, head_dim):
    """kv_cache_append_ into an e4m3 cache: the roped k and the v of every in-range token are quantised per
    (token, kv head) vector, codes and scales go to cache / scale[rows[t], :, pos[t]], and the dequantised
    values (code * scale, exact in bf16) replace k and v in qkv (csrc/kernels/decode_attn.hip)."""
    T, d = qkv.shape[0], head_dim
    _check_fp8_cache("kv_cache_append_fp8_", k_cache, v_cache, k_scale, v_scale)
    if not (k_cache.dim() == 4 and k_cache.shape == v_cache.shape and k_cache.shape[1] == nkv and k_cache.shape[3] == d):
        raise RuntimeError("dtg: kv_cache_append_fp8_: caches must be contiguous float8_e4m3fn [rows_max, nkv, S_max, head_dim]")
    if not (qkv.dim() == 2 and qkv.shape[1] >= (nq + 2 * nkv) * d and pos.numel() == T and rows.numel() == T):
        raise RuntimeError("dtg: kv_cache_append_fp8_: qkv must be [T, (nq + 2 nkv) * head_dim] with one pos and row per token")
    pos, rows = pos.long(), rows.long()
    ok = (pos >= 0) & (pos < k_cache.shape[2]) & (rows >= 0) & (rows < k_cache.shape[0])
    if cos.numel():
        ok &= pos < cos.shape[0]
        sel = qkv[ok]
        rope_(sel, cos, sin, pos[ok], nq + nkv, d, False)
        qkv[ok] = sel
    n = int(ok.sum())
    for cache, scales, c0 in ((k_cache, k_scale, nq * d), (v_cache, v_scale, (nq + nkv) * d)):
        codes, s = _e4m3_vectors(qkv[ok, c0:c0 + nkv * d].float().reshape(n, nkv, d))
        cache.view(torch.uint8)[rows[ok], :, pos[ok]] = codes
        scales[rows[ok], :, pos[ok]] = s
        deq = codes.view(torch.float8_e4m3fn).float() * s[..., None]
        qkv[ok, c0:c0 + nkv * d] = deq.reshape(n, nkv * d).to(qkv.dtype)


def decode_attn_fp8(qkv, k_cache, v_cache, k_scale, v_scale, rows, lens, q_len, nq, nkv, head_dim, scale, max_len,
                    window, splits):
    """decode_attn (q_len = 1) / decode_attn_multi (q_len > 1) on an e4m3 cache: a key vector is
    float(code) * its scale, exactly a bf16 value; only the attended keys and their scales are read."""
    _check_fp8_cache("decode_attn_fp8", k_cache, v_cache, k_scale, v_scale)
    if q_len < 1 or qkv.shape[0] % q_len or rows.numel() * q_len != qkv.shape[0] or lens.numel() != qkv.shape[0]:
        raise RuntimeError("dtg: decode_attn_fp8: qkv and lens need q_len >= 1 rows per entry of rows")

    def load(r, lo, n):
        return (k_cache[r, :, lo:n].float() * k_scale[r, :, lo:n, None], v_cache[r, :, lo:n].float() * v_scale[r, :, lo:n, None])

    return _decode_rows("decode_attn_fp8", qkv, k_cache, v_cache, load, rows.repeat_interleave(q_len), lens, nq, nkv,
                        head_dim, scale, max_len, window)


def decode_attn(qkv, k_cache, v_cache, rows, lens, nq, nkv, head_dim, scale, max_len, window=0, splits=0):
    """One query token per sequence against keys [max(0, len - window), len) of its cache row, f32
    softmax, one rounding.  The CPU reference takes any head dim and group size; `splits` has no
    meaning here (one pass)."""
    return _decode_rows("decode_attn", qkv, k_cache, v_cache,
                        lambda r, lo, n: (k_cache[r, :, lo:n].float(), v_cache[r, :, lo:n].float()), rows, lens, nq, nkv,
                        head_dim, scale, max_len, window)


def _decode_rows(name, qkv, k_cache, v_cache, load, rows, lens, nq, nkv, head_dim, scale, max_len, window):
    """decode_attn's loop; load(r, lo, n) returns the f32 keys and values [nkv, n - lo, D] of cache row r."""
    B, d, g = qkv.shape[0], head_dim, nq // nkv
    if nq % nkv or not (k_cache.dim() == 4 and k_cache.shape == v_cache.shape and k_cache.shape[1] == nkv
                        and k_cache.shape[3] == d):
        raise RuntimeError(f"dtg: {name}: caches must be contiguous [rows_max, nkv, S_max, head_dim]")
    if not 0 <= max_len <= k_cache.shape[2]:
        raise RuntimeError(f"dtg: {name}: max_len must lie in [0, S_max]")
    out = torch.zeros(B, nq * d, dtype=qkv.dtype)
    for b in range(B):
        n, r = int(lens[b]), int(rows[b])
        if not 0 <= r < k_cache.shape[0]:
            continue
        n = min(n, k_cache.shape[2])
        lo = max(0, n - window) if window > 0 else 0
        if n <= lo:
            continue
        q = qkv[b, : nq * d].float().reshape(nkv, g, d)
        k, v = load(r, lo, n)
        p = torch.softmax(torch.einsum("hgd,hsd->hgs", q, k) * scale, -1)
        out[b] = torch.einsum("hgs,hsd->hgd", p, v).reshape(nq * d).to(qkv.dtype)
    return out


def decode_attn_multi(qkv, k_cache, v_cache, rows, lens, q_len, nq, nkv, head_dim, scale, max_len, window, splits):
    """q_len tokens per sequence, token (b, t) = row b * q_len + t of qkv and lens, against cache row rows[b]:
    decode_attn's loop over the tokens."""
    if q_len < 1 or qkv.shape[0] % q_len or rows.numel() * q_len != qkv.shape[0] or lens.numel() != qkv.shape[0]:
        raise RuntimeError("dtg: decode_attn_multi: qkv and lens need q_len >= 1 rows per entry of rows")
    return decode_attn(qkv, k_cache, v_cache, rows.repeat_interleave(q_len), lens, nq, nkv, head_dim, scale, max_len,
                       window, splits)


def swiglu_fwd(gu):
    inter = gu.shape[1] // 2
    g, u = gu[:, :inter].float(), gu[:, inter:].float()
    return (F.silu(g) * u).to(gu.dtype)


SKINNY_MAX_M = 16  # rows of x the skinny kernels are instantiated for (kSkinnyMaxM); imported where it is needed


def _skinny_check(name, x, w, act, chunk, w_layout):
    """The refusals the two skinny operators share; `chunk` = weights per 16-B load, `w_layout` the operator's
    own message for the weight matrix."""
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: x must be a bf16 tensor")
    if act not in (0, 1):
        raise RuntimeError(f"{name}: act must be 0 (none) or 1 (SwiGLU)")
    if x.dim() != 2 or not 1 <= x.shape[0] <= SKINNY_MAX_M:
        raise RuntimeError(f"{name}: x must be [M, K] with 1 <= M <= {SKINNY_MAX_M}")
    if x.shape[1] % chunk:
        raise RuntimeError(f"{name}: K must be a multiple of {chunk}")
    if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        raise RuntimeError(f"{name}: x must have unit inner stride and 16-B aligned rows")
    if w.dim() != 2 or w.shape[1] != x.shape[1] or w.shape[0] < 1 or not w.is_contiguous() or w.data_ptr() % 16:
        raise RuntimeError(f"{name}: {w_layout}")
    if act and w.shape[0] % 2:
        raise RuntimeError(f"{name}: the SwiGLU epilogue needs an even N (gate rows, then up rows)")


def _skinny_tail(name, y, bias, act, dtype):
    """f32 product [M, N] -> + bias, one rounding, swiglu_fwd when act."""
    if bias is not None:
        if bias.dtype != torch.bfloat16 or bias.dim() != 1 or bias.shape[0] != y.shape[1] or not bias.is_contiguous():
            raise RuntimeError(f"{name}: bias must be a contiguous bf16 [N]")
        y = y + bias.float()
    y = y.to(dtype)
    return swiglu_fwd(y) if act else y


def skinny_linear(x, w, bias, act=0):
    """y = x @ w^T (+ bias) at 1 <= M <= 16 rows, f32 sums, one rounding; act = 1: the gate and up halves
    of that (rounded) product through swiglu_fwd, [M, N / 2] (csrc/kernels/skinny_gemm.hip).  Refuses
    what the kernel refuses."""
    name = "dtg: skinny_linear"
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: x and w must be bf16 tensors")
    _skinny_check(name, x, w, act, 8, "w must be a contiguous [N, K] on x's device")
    return _skinny_tail(name, x.float() @ w.float().t(), bias, act, x.dtype)


def skinny_linear_fp8(x, wq, scale, bias, act=0):
    """y = (x @ float(wq)^T) * scale (+ bias) at 1 <= M <= 16 rows: wq float8_e4m3fn [N, K], scale f32 [N];
    f32 sums, one rounding; act = 1 as skinny_linear (csrc/kernels/skinny_gemm.hip).  Refuses what the
    kernel refuses."""
    name = "dtg: skinny_linear_fp8"
    if wq.dtype != torch.float8_e4m3fn:
        raise RuntimeError(f"{name}: wq must be a float8_e4m3fn tensor")
    _skinny_check(name, x, wq, act, 16, "wq must be a contiguous 16-B aligned [N, K] on x's device")
    if scale.dtype != torch.float32 or scale.dim() != 1 or scale.shape[0] != wq.shape[0] or not scale.is_contiguous():
        raise RuntimeError(f"{name}: scale must be a contiguous f32 [N] on x's device")
    return _skinny_tail(name, (x.float() @ wq.float().t()) * scale, bias, act, x.dtype)


def swiglu_bwd(dh, gu):
    inter = gu.shape[1] // 2
    g, u, d = gu[:, :inter].float(), gu[:, inter:].float(), dh.float()
    s = torch.sigmoid(g)
    du = d * g * s
    dg = d * u * s * (1 + g * (1 - s))
    return torch.cat([dg, du], dim=1).to(gu.dtype)


def ce_fwd_bwd_(logits, labels, ignore_index, grad_scale, compute_grad):
    x = logits.float()
    lse = torch.logsumexp(x, dim=-1)
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, safe[:, None])[:, 0]
    loss = torch.where(valid, lse - xl, torch.zeros_like(lse))
    if compute_grad:
        g = torch.exp(x - lse[:, None])
        g.scatter_add_(1, safe[:, None], -torch.ones_like(g[:, :1]))
        g = g * grad_scale
        g[~valid] = 0
        logits.copy_(g.to(logits.dtype))
    return loss


def ce_stats(logits, labels, vocab_start):
    x = logits.float()
    m = x.max(-1).values
    s = torch.exp(x - m[:, None]).sum(-1)
    local = labels - vocab_start
    inside = (local >= 0) & (local < x.shape[1])
    xl = x.gather(1, local.clamp(0, x.shape[1] - 1)[:, None])[:, 0]
    return m, s, torch.where(inside, xl, torch.zeros_like(xl))


def ce_grad_(logits, labels, lse, vocab_start, ignore_index, grad_scale):
    x = logits.float()
    g = torch.exp(x - lse[:, None])
    local = labels - vocab_start
    inside = (local >= 0) & (local < x.shape[1])
    onehot = torch.zeros_like(g)
    rows = torch.nonzero(inside).flatten()
    onehot[rows, local[rows]] = 1.0
    g = (g - onehot) * grad_scale
    g[labels == ignore_index] = 0
    logits.copy_(g.to(logits.dtype))


def adamw_t_(p, master, g, m, v, pt, mats, ntiles, lr, beta1, beta2, eps, wd, step, grad_scale, hyper=None,
             tile_cols=64, gscale=None):
    """The HIP kernel's semantics: only the elements of the listed matrices are updated; each
    matrix with a transposed slot gets its new values transposed into `pt`."""
    for off, rows, cols, toff, _ in mats.tolist():
        n = rows * cols
        sl = slice(off, off + n)
        adamw_(p[sl], None if master is None else master[sl], g[sl], m[sl], v[sl], lr, beta1, beta2, eps, wd,
               step, grad_scale, hyper, gscale)
        if toff >= 0:
            pt[toff:toff + n].copy_(p[sl].view(rows, cols).t().reshape(-1))


def adamw_(p, master, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, hyper=None, gscale=None):
    bc1 = 1 - beta1**step
    bc2 = math.sqrt(1 - beta2**step)
    if hyper is not None:
        lr, bc1, bc2 = (float(x) for x in hyper[:3].tolist())
    if gscale is not None:  # the kernel's f32 product grad_scale * gscale[0]
        grad_scale = float(torch.tensor(grad_scale, dtype=torch.float32) * gscale.float().reshape(-1)[0])
    pf = master if master is not None else p.float()
    gf = g.float() * grad_scale
    mf, vf = m.float(), v.float()
    pf = pf * (1 - lr * wd)
    mf = mf + (gf - mf) * (1 - beta1)
    vf = vf * beta2 + (1 - beta2) * gf * gf
    pf = pf - (lr / bc1) * mf / (vf.sqrt() / bc2 + eps)
    m.copy_(mf)
    v.copy_(vf)
    if master is not None:
        master.copy_(pf)
    p.copy_(pf)


_SUMSQ_CHUNK = 1 << 20


def grad_sumsq_(g, acc, slot):
    """acc[slot] += sum(g^2) in f32, a chunk at a time (no f32 temporary the size of g)."""
    assert g.dim() == 1 and acc.dtype == torch.float32
    for i in range(0, g.numel(), _SUMSQ_CHUNK):
        acc[slot] += g[i:i + _SUMSQ_CHUNK].float().square().sum()  # not in place: .float() of f32 is g itself


def _key_ranges(cu_seqlens, k_start=None, k_len=None):
    """[(q0, q1, k0, k1)] per sequence: self-attention by default, else explicit key ranges with
    the bottom-right-aligned causal mask (query i of n_q attends keys <= i + n_k - n_q)."""
    cu = cu_seqlens.tolist()
    out = []
    for i in range(len(cu) - 1):
        a, b = cu[i], cu[i + 1]
        if k_start is None:
            out.append((a, b, a, b))
        else:
            ks, kl = int(k_start[i]), int(k_len[i])
            out.append((a, b, ks, ks + kl))
    return out


def _mask(nq, nk, window=0):
    # True = masked: key j > query i + (nk - nq), or (sliding window) j <= i + (nk - nq) - window
    i = torch.arange(nq)[:, None]
    j = torch.arange(nk)[None, :]
    m = j > i + (nk - nq)
    if window > 0:
        m = m | (j <= i + (nk - nq) - window)
    return m


def _attn_ref(q, k, v, cu_seqlens, scale, causal, k_start=None, k_len=None, window=0):
    """Per-sequence f32 attention; returns o (bf16/in dtype) and lse [Hq, T] (natural log)."""
    T, hq, d = q.shape
    hkv = k.shape[1]
    rep = hq // hkv
    o = torch.zeros(T, hq, d, dtype=torch.float32)
    lse = torch.full((hq, T), float("-inf"), dtype=torch.float32)
    for a, b, ka, kb in _key_ranges(cu_seqlens, k_start, k_len):
        if b <= a:
            continue
        qs = q[a:b].float().transpose(0, 1)  # [hq, s, d]
        ks = k[ka:kb].float().transpose(0, 1).repeat_interleave(rep, 0)
        vs = v[ka:kb].float().transpose(0, 1).repeat_interleave(rep, 0)
        sc = qs @ ks.transpose(1, 2) * scale
        if causal:
            sc = sc.masked_fill(_mask(b - a, kb - ka, window), float("-inf"))
        l_ = torch.logsumexp(sc, -1)
        p = torch.exp(sc - l_[..., None])
        o[a:b] = (p @ vs).transpose(0, 1)
        lse[:, a:b] = l_
    return o, lse


def _check_qkv(t, name, heads, d):
    """check_qkv of csrc/kernels/flash_attn.hip: [T, H, D], contiguous heads, 16-B token stride."""
    if not (t.dim() == 3 and t.shape[1] == heads and t.shape[2] == d and t.stride(2) == 1 and t.stride(1) == d
            and t.stride(0) % 8 == 0):
        raise RuntimeError(f"dtg: {name} must be [T, H, D] with contiguous heads and 16-B aligned token stride")


def _check_attn_inputs(q, k, v):
    _check_qkv(q, "q", q.shape[1], q.shape[2])
    _check_qkv(k, "k", k.shape[1], q.shape[2])
    _check_qkv(v, "v", k.shape[1], q.shape[2])


def flash_attn_fwd(q, k, v, cu_seqlens, max_seqlen, scale, causal, window=0):
    _check_attn_inputs(q, k, v)
    o, lse = _attn_ref(q, k, v, cu_seqlens, scale, causal, window=window)
    return o.to(q.dtype), lse


# ---- attention dropout: the kernels' counter-based keep mask (csrc/kernels/flash_attn.hip DropCfg)
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit values (Random123's round function)."""
    import numpy as np

    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & m32, np.uint64(k1) & m32
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_PHILOX_W[0])) & m32
            k1 = (k1 + np.uint64(_PHILOX_W[1])) & m32
        p0 = np.uint64(_PHILOX_M[0]) * c[0]
        p1 = np.uint64(_PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
    return c


def dropout_threshold(p):
    """(thr, scale): keep iff random byte < thr; keep probability thr / 256, scale 256 / thr."""
    thr = max(1, min(256, int(round((1.0 - p) * 256.0))))
    return thr, 256.0 / thr


def dropout_keep(seed, offset, head, s0, nq, nk, p):
    """bool [nq, nk]: the keep decision of (query q, key k) of the sequence starting at token s0
    (sequence-relative q, k) for query head `head` -- byte (k & 3) of word (q & 3) of
    Philox4x32-10({k & ~3, s0 + (q & ~3), head, offset lo}, key = {seed lo, seed hi ^ offset hi}).
    The offset's high word goes into the key, so offsets past 2^32 (long runs draw 4 per call)
    never repeat an earlier mask."""
    import numpy as np

    thr, _ = dropout_threshold(p)
    q = np.arange(nq, dtype=np.uint64)[:, None]
    k = np.arange(nk, dtype=np.uint64)[None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    offset = int(offset) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(k & ~np.uint64(3), np.uint64(s0) + (q & ~np.uint64(3)), np.full_like(q, head),
                      np.full_like(q, offset & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) ^ (offset >> 32))
    sel = (q & np.uint64(3)).astype(np.int64)
    word = np.choose(np.broadcast_to(sel, (nq, nk)), [np.broadcast_to(x, (nq, nk)) for x in w])
    byte = (word >> (np.uint64(8) * (k & np.uint64(3)))) & np.uint64(255)
    return torch.from_numpy(byte.astype(np.int64) < thr)


def _drop_masks(cu_seqlens, hq, p, seed, offset):
    out = []
    for a, b, _, _ in _key_ranges(cu_seqlens):
        out.append(torch.stack([dropout_keep(seed, offset, h, a, b - a, b - a, p) for h in range(hq)]) if b > a else None)
    return out


def _rng_pair(rng):
    seed, offset = (int(x) for x in rng.reshape(-1).tolist())
    return seed, offset


def philox_rng(like, increment):
    """{seed, offset} of one dropout call from torch's CPU generator (reproducible under
    torch.manual_seed, checkpointed with the RNG state)."""
    r = torch.randint(0, 2**62, (2,))
    return torch.tensor([int(r[0]), int(r[1] % (2**31))], dtype=torch.int64)


def flash_attn_fwd_drop(q, k, v, cu_seqlens, max_seqlen, scale, causal, p, rng):
    """o = (M o softmax(S) * 256/thr) V per sequence; lse of the undropped softmax."""
    seed, offset = _rng_pair(rng)
    _check_attn_inputs(q, k, v)
    T, hq, d = q.shape
    rep = hq // k.shape[1]
    _, sc_keep = dropout_threshold(p)
    o = torch.zeros(T, hq, d, dtype=torch.float32)
    lse = torch.full((hq, T), float("-inf"), dtype=torch.float32)
    for (a, b, _, _), m in zip(_key_ranges(cu_seqlens), _drop_masks(cu_seqlens, hq, p, seed, offset)):
        if b <= a:
            continue
        qs = q[a:b].float().transpose(0, 1)
        ks = k[a:b].float().transpose(0, 1).repeat_interleave(rep, 0)
        vs = v[a:b].float().transpose(0, 1).repeat_interleave(rep, 0)
        s = qs @ ks.transpose(1, 2) * scale
        if causal:
            s = s.masked_fill(_mask(b - a, b - a), float("-inf"))
        l_ = torch.logsumexp(s, -1)
        pr = torch.exp(s - l_[..., None]) * m * sc_keep
        o[a:b] = (pr @ vs).transpose(0, 1)
        lse[:, a:b] = l_
    return o.to(q.dtype), lse


def flash_attn_bwd_drop(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, p, rng):
    seed, offset = _rng_pair(rng)
    _check_attn_inputs(q, k, v)
    T, hq, d = q.shape
    hkv = k.shape[1]
    rep = hq // hkv
    _, sc_keep = dropout_threshold(p)
    dq = torch.zeros(T, hq, d, dtype=torch.float32)
    dk = torch.zeros(T, hkv, d, dtype=torch.float32)
    dv = torch.zeros(T, hkv, d, dtype=torch.float32)
    for (a, b, _, _), m in zip(_key_ranges(cu_seqlens), _drop_masks(cu_seqlens, hq, p, seed, offset)):
        if b <= a:
            continue
        qs = q[a:b].float().transpose(0, 1)
        ks = k[a:b].float().transpose(0, 1).repeat_interleave(rep, 0)
        vs = v[a:b].float().transpose(0, 1).repeat_interleave(rep, 0)
        dos = dout[a:b].float().transpose(0, 1)
        os_ = o[a:b].float().transpose(0, 1)
        s = qs @ ks.transpose(1, 2) * scale
        if causal:
            s = s.masked_fill(_mask(b - a, b - a), float("-inf"))
        pr = torch.exp(s - lse[:, a:b].float()[..., None])
        z = pr * m * sc_keep
        dvh = z.transpose(1, 2) @ dos
        dpr = (dos @ vs.transpose(1, 2)) * m * sc_keep
        delta = (dos * os_).sum(-1, keepdim=True)
        ds = pr * (dpr - delta)
        dq[a:b] = (ds @ ks * scale).transpose(0, 1)
        dk[a:b] += (ds.transpose(1, 2) @ qs * scale).view(hkv, rep, b - a, d).sum(1).transpose(0, 1)
        dv[a:b] += dvh.view(hkv, rep, b - a, d).sum(1).transpose(0, 1)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


# ---- LayerNorm with fused dropout + residual add, GELU-tanh (csrc/kernels/layernorm.hip, gelu.hip)
_LN_STREAM_TAG = 0x4C4E4452


def ln_dropout_keep(seed, offset, T, H, p):
    """bool [T, H]: the keep decision of element (row, col) -- byte (col & 3) of word
    ((col >> 2) & 1) of Philox4x32-10({col >> 3, row, offset lo, "LNDR"}, key = {seed lo,
    seed hi ^ offset hi}) < thr.  The counter layout of layernorm.hip, bit for bit."""
    import numpy as np

    thr, _ = dropout_threshold(p)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    offset = int(offset) & 0xFFFFFFFFFFFFFFFF
    rows = np.arange(T, dtype=np.uint64)[:, None]
    chunks = np.arange(H // 8, dtype=np.uint64)[None, :]
    shape = (T, H // 8)
    w = philox4x32_10(np.broadcast_to(chunks, shape), np.broadcast_to(rows, shape),
                      np.full(shape, offset & 0xFFFFFFFF, dtype=np.uint64),
                      np.full(shape, _LN_STREAM_TAG, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) ^ (offset >> 32))
    byte = np.stack([(w[j >> 2] >> np.uint64(8 * (j & 3))) & np.uint64(255) for j in range(8)], axis=-1)
    return torch.from_numpy((byte.astype(np.int64) < thr).reshape(T, H))


def _ln_check_rows(t, name):
    """check_rows of norm_common.h as layernorm.hip uses it: 2-D, unit inner stride, 16-B aligned rows, H % 8 == 0."""
    if not (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0):
        raise RuntimeError(f"dtg: {name} must be 2-D with unit inner stride and 16-byte aligned rows")
    if t.shape[1] % 8:
        raise RuntimeError("dtg: layernorm: bad weight/hidden")
    if t.shape[1] > 16384:
        raise RuntimeError("dtg: layernorm: unsupported hidden size")


def _ln_drop(p, rng):
    if not 0.0 <= p < 1.0:
        raise RuntimeError("dtg: layernorm dropout: p must be in [0, 1)")
    if p == 0.0:
        if rng is not None:
            raise RuntimeError("dtg: layernorm dropout: rng given with p == 0")
        return None
    if rng is None:
        raise RuntimeError("dtg: layernorm dropout: rng must be a contiguous int64 [2] tensor {seed, offset}")
    return _rng_pair(rng)


def _ln_stats(h, eps):
    """Two-pass f32 mean and rstd of the rows (the kernel's order: mean, then the centred squares)."""
    hf = h.float()
    mean = hf.mean(-1)
    d = hf - mean[:, None]
    return mean, torch.rsqrt((d * d).mean(-1) + eps)


def layernorm_fwd(x, w, b, eps):
    _ln_check_rows(x, "x")
    mean, rstd = _ln_stats(x, eps)
    return F.layer_norm(x, (x.shape[1],), w, b, eps), mean, rstd


def dropout_add_layernorm_fwd(x, res, w, b, eps, p, rng):
    _ln_check_rows(x, "x")
    _ln_check_rows(res, "residual")
    so = _ln_drop(p, rng)
    xf = x.float()
    if so is not None:
        keep = ln_dropout_keep(so[0], so[1], x.shape[0], x.shape[1], p)
        xf = torch.where(keep, xf * dropout_threshold(p)[1], torch.zeros_like(xf))
    h = (res.float() + xf).to(x.dtype)
    y, mean, rstd = layernorm_fwd(h, w, b, eps)
    return y, h, mean, rstd


def layernorm_bwd(dy, h, w, mean, rstd, dres, p, rng):
    _ln_check_rows(h, "h")
    so = _ln_drop(p, rng)
    dyf, wf, r = dy.float(), w.float(), rstd[:, None]
    n = (h.float() - mean[:, None]) * r
    g = dyf * wf
    dhf = r * (g - g.mean(-1, keepdim=True) - n * (g * n).mean(-1, keepdim=True))
    if dres is not None:
        dhf = dhf + dres.float()
    dh = dhf.to(h.dtype)
    dx = dh
    if so is not None:
        keep = ln_dropout_keep(so[0], so[1], h.shape[0], h.shape[1], p)
        dx = torch.where(keep, dhf * dropout_threshold(p)[1], torch.zeros_like(dhf)).to(h.dtype)
    return dh, dx, (dyf * n).sum(0).to(w.dtype), dyf.sum(0).to(w.dtype)


_GELU_C = math.sqrt(2.0 / math.pi)
_GELU_A = 0.044715


def _gelu_check(x, name):
    if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.shape[1] % 8 == 0):
        raise RuntimeError(f"dtg: {name}: x must be [T, I] with unit inner stride, 16-byte aligned rows and I % 8 == 0")


def gelu_fwd(x):
    _gelu_check(x, "gelu_fwd")
    return F.gelu(x, approximate="tanh").contiguous()


def gelu_bwd(dh, x):
    """dh * (sigma + x sigma (1 - sigma) 2u'), sigma = sigmoid(2u): the kernel's closed form."""
    _gelu_check(x, "gelu_bwd")
    xf = x.float()
    s = torch.sigmoid(2 * _GELU_C * (xf + _GELU_A * xf * xf * xf))
    du2 = 2 * _GELU_C * (1 + 3 * _GELU_A * xf * xf)
    return (dh.float() * (s + xf * s * (1 - s) * du2)).to(x.dtype)


def gelu_bwd_t(dh, x):
    if x.shape[0] % 8:
        raise RuntimeError("dtg: gelu_bwd_t: T must be a multiple of 8")
    dx = gelu_bwd(dh, x)
    return dx, dx.t().contiguous(), gelu_fwd(x).t().contiguous()


def _qkv_heads(qkv, nq, nkv, d):
    """q [T, nq, d], k and v [T, nkv, d] of a fused [T, (nq + 2 nkv) * d] activation."""
    T = qkv.shape[0]
    q = qkv[:, : nq * d].reshape(T, nq, d)
    k = qkv[:, nq * d : (nq + nkv) * d].reshape(T, nkv, d)
    v = qkv[:, (nq + nkv) * d :].reshape(T, nkv, d)
    return q, k, v


def flash_attn_bwd_qkv_drop(dout, qkv, nq, nkv, head_dim, o, lse, cu_seqlens, max_seqlen, scale, causal, p, rng):
    T = qkv.shape[0]
    q, k, v = _qkv_heads(qkv, nq, nkv, head_dim)
    dq, dk, dv = flash_attn_bwd_drop(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, p, rng)
    return torch.cat([dq.reshape(T, -1), dk.reshape(T, -1), dv.reshape(T, -1)], dim=1)


def flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, k_start, k_len, max_seqlen_q, max_seqlen_k, scale, causal):
    _check_attn_inputs(q, k, v)
    o, lse = _attn_ref(q, k, v, cu_seqlens_q, scale, causal, k_start, k_len)
    return o.to(q.dtype), lse


def _flash_attn_bwd_f32(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, window=0, k_start=None,
                        k_len=None):
    """flash_attn_bwd's dq, dk, dv in f32, before the store's rounding (the fused RoPE form rotates
    them first, as the kernel epilogues do)."""
    T, hq, d = q.shape
    _check_attn_inputs(q, k, v)
    # the HIP entry point's layout contract (csrc/kernels/flash_attn.hip), checked here too so the
    # CPU suite catches a caller that would only fail on the GPU (the rime --cp path passed a
    # strided per-slot view of the LSE at batch 1)
    if not (lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (hq, T)):
        raise RuntimeError("dtg: flash_attn_bwd: lse must be f32 [Hq, T]")
    if not (o.is_contiguous() and dout.shape == o.shape and o.shape[0] == T):
        raise RuntimeError("dtg: flash_attn_bwd: o/dout")
    hkv = k.shape[1]
    rep = hq // hkv
    dq = torch.zeros(T, hq, d, dtype=torch.float32)
    dk = torch.zeros(k.shape[0], hkv, d, dtype=torch.float32)
    dv = torch.zeros(k.shape[0], hkv, d, dtype=torch.float32)
    for a, b, ka, kb in _key_ranges(cu_seqlens, k_start, k_len):
        if b <= a:
            continue
        qs = q[a:b].float().transpose(0, 1)                               # [hq, s, d]
        ks = k[ka:kb].float().transpose(0, 1).repeat_interleave(rep, 0)
        vs = v[ka:kb].float().transpose(0, 1).repeat_interleave(rep, 0)
        dos = dout[a:b].float().transpose(0, 1)
        os_ = o[a:b].float().transpose(0, 1)
        sc = qs @ ks.transpose(1, 2) * scale
        if causal:
            sc = sc.masked_fill(_mask(b - a, kb - ka, window), float("-inf"))
        p = torch.exp(sc - lse[:, a:b].float()[..., None])
        dvh = p.transpose(1, 2) @ dos
        dp = dos @ vs.transpose(1, 2)
        delta = (dos * os_).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        dqh = ds @ ks * scale
        dkh = ds.transpose(1, 2) @ qs * scale
        dq[a:b] = dqh.transpose(0, 1)
        dk[ka:kb] += dkh.view(hkv, rep, kb - ka, d).sum(1).transpose(0, 1)
        dv[ka:kb] += dvh.view(hkv, rep, kb - ka, d).sum(1).transpose(0, 1)
    return dq, dk, dv


def flash_attn_bwd(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, window=0, k_start=None, k_len=None):
    """The kernel's semantics: P = exp(S*scale - lse) with the GIVEN lse, delta = rowsum(dO*O)
    with the GIVEN o (so a block of a larger softmax -- context parallelism -- gets the
    gradient of the full softmax)."""
    dq, dk, dv = _flash_attn_bwd_f32(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, window, k_start, k_len)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def flash_attn_varlen_bwd(dout, q, k, v, o, lse, cu_seqlens_q, k_start, k_len, max_seqlen_q, max_seqlen_k, scale,
                          causal):
    return flash_attn_bwd(dout, q, k, v, o, lse, cu_seqlens_q, max_seqlen_q, scale, causal, 0, k_start, k_len)


def flash_attn_bwd_qkv(dout, qkv, nq, nkv, head_dim, o, lse, cu_seqlens, max_seqlen, scale, causal, window=0):
    T = qkv.shape[0]
    q, k, v = _qkv_heads(qkv, nq, nkv, head_dim)
    dq, dk, dv = flash_attn_bwd(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, window)
    return torch.cat([dq.reshape(T, -1), dk.reshape(T, -1), dv.reshape(T, -1)], dim=1)


def flash_attn_bwd_qkv_rope(dout, qkv, nq, nkv, head_dim, o, lse, cu_seqlens, max_seqlen, scale, causal, cos, sin,
                            pos, window=0):
    # as the kernels' epilogues: the inverse rotation in f32, then the single rounding of the store
    T = qkv.shape[0]
    q, k, v = _qkv_heads(qkv, nq, nkv, head_dim)
    dq, dk, dv = _flash_attn_bwd_f32(dout, q, k, v, o, lse, cu_seqlens, max_seqlen, scale, causal, window)
    dqkv = torch.cat([dq.reshape(T, -1), dk.reshape(T, -1), dv.reshape(T, -1)], dim=1)
    rope_(dqkv, cos, sin, pos, nq + nkv, head_dim, True)
    return dqkv.to(qkv.dtype)


def swiglu_bwd_t(dh, gu):
    """check_x / check_dh of csrc/kernels/mlp_act.h, then the two untiled operators."""
    if not (gu.dim() == 2 and gu.stride(1) == 1 and gu.stride(0) % 8 == 0 and gu.shape[1] % 16 == 0):
        raise RuntimeError("dtg: swiglu_bwd_t: the pre-activation must be [T, 2 * I] with unit inner stride, "
                           "16-byte aligned rows and I % 8 == 0")
    if not (dh.dim() == 2 and dh.shape[0] == gu.shape[0] and dh.shape[1] == gu.shape[1] // 2):
        raise RuntimeError("dtg: swiglu_bwd_t: shape mismatch")
    dgu = swiglu_bwd(dh, gu)
    return dgu, dgu.t().contiguous(), swiglu_fwd(gu).t().contiguous()


def transpose2d(x):
    return x.t().contiguous()


def transpose_mats_(x, out, mats, mats_host, ntiles):
    for so, r, c, do, _t0 in mats_host.tolist():
        out[do:do + r * c].copy_(x[so:so + r * c].view(r, c).t().reshape(-1))


def embedding_bwd_(out, ids, dy):
    """out[id] += sum of dy rows with that id, f32 sums rounded once; ids outside [0, V) skipped."""
    acc = torch.zeros(out.shape, dtype=torch.float32)
    ids = ids.reshape(-1)
    keep = (ids >= 0) & (ids < out.shape[0])
    acc.index_add_(0, ids[keep], dy.reshape(-1, dy.shape[-1])[keep].float())
    out.copy_((out.float() + acc).to(out.dtype))


def sample_u(rng):
    """f32 [n]: the uniform of each row of the int64 [n, 3] tensor {seed, stream, step}:
    (word 0 of Philox4x32-10({step lo, step hi, stream lo, stream hi}, key = {seed lo, seed hi}) >> 8) * 2^-24,
    bit-equal to the kernel's draw.  Reads `rng` on the host."""
    import numpy as np

    g = rng.detach().cpu().numpy().astype(np.int64).view(np.uint64).reshape(-1, 3)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    w0 = philox4x32_10(lo[:, 2], hi[:, 2], lo[:, 1], hi[:, 1], lo[:, 0], hi[:, 0])[0]
    u = (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u).to(rng.device)


def sample_logits(logits, params, top_k, rng, u=None):
    """The definition of ops.sample_logits in f64, for all rows at once and on the tensors' device
    (DTG_SAMPLE_FUSED=0 runs this on the GPU).  The distinct values of a row and the masses of their tie
    groups come from one descending sort: the mass of {x >= t} is the running sum at the last element
    equal to t, found by searchsorted, which is what torch.unique + a group sum give, without its
    data-dependent shape."""
    n, V = logits.shape
    dev = logits.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    ninf = float("-inf")
    x = logits.to(torch.float64)
    x = torch.where(torch.isnan(x), torch.full_like(x, ninf), x)
    T, top_p, min_p = (params[:, i].to(torch.float64) for i in range(3))
    k = top_k.to(torch.int64)
    idx = torch.arange(V, device=dev)
    M = x.max(1).values
    first_max = torch.where(x == M[:, None], idx, V).min(1).values
    n_max = (x == M[:, None]).sum(1)
    dead, hot = M == ninf, M == float("inf")
    greedy = ~(T > 0)
    special = dead | hot | greedy
    Ms = torch.where(special, torch.zeros_like(M), M)[:, None]
    Ts = torch.where(special, torch.ones_like(T), T)[:, None]
    xs = torch.where(special[:, None], torch.zeros_like(x), x)  # special rows: any finite row, overridden below
    w = torch.where(xs == Ms, torch.ones_like(xs), torch.exp((xs - Ms) / Ts))
    w = torch.where(xs == ninf, torch.zeros_like(w), w)

    desc, order = xs.sort(1, descending=True)
    asc = desc.flip(1).contiguous()
    # t_k: the k-th largest, with multiplicity
    kth = desc.gather(1, (k - 1).clamp(0, V - 1)[:, None])[:, 0]
    t_k = torch.where((k > 0) & (k < V), kth, torch.full_like(kth, ninf))
    in_a = xs >= t_k[:, None]
    wa = w * in_a
    z_a = wa.sum(1)
    # t_p: the largest value t of A with mass {A, x >= t} >= top_p Z_A
    cs = wa.gather(1, order).cumsum(1)
    n_ge = V - torch.searchsorted(asc, desc.contiguous(), right=False)  # elements >= each sorted value
    mass_ge = cs.gather(1, n_ge - 1)
    ok = (desc >= t_k[:, None]) & (mass_ge >= (top_p * z_a)[:, None])
    t_p = torch.where(ok, desc, torch.full_like(desc, ninf)).max(1).values
    t_p = torch.where((top_p > 0) & (top_p < 1), t_p, torch.where(top_p <= 0, Ms[:, 0], torch.full_like(t_p, ninf)))
    # t_m: w >= min_p
    t_m = torch.where(min_p > 0, Ms[:, 0] + Ts[:, 0] * torch.log(min_p.clamp_min(1e-300)), torch.full_like(M, ninf))
    t_m = torch.where(torch.isnan(t_m), torch.full_like(t_m, ninf), t_m)
    thr = torch.minimum(torch.maximum(torch.maximum(t_k, t_p), t_m), Ms[:, 0])
    in_k = xs >= thr[:, None]
    c = (w * in_k).cumsum(1)  # index order
    z_k = c[:, -1]
    if u is None:
        u = sample_u(rng)
    u = u.to(torch.float64)
    u = torch.where(u >= 0, u.clamp(max=1.0), torch.zeros_like(u))
    ids = torch.searchsorted(c, (u * z_k)[:, None], right=True)[:, 0]
    last = torch.where(in_k, idx, -1).max(1).values
    ids = torch.where(ids >= V, last, ids)
    kept = in_k.sum(1)

    ids = torch.where(greedy | hot, first_max, ids)
    kept = torch.where(greedy, torch.ones_like(kept), kept)
    kept = torch.where(hot, n_max, kept)
    ids = torch.where(dead, torch.full_like(ids, -1), ids)
    kept = torch.where(dead, torch.zeros_like(kept), kept)
    return ids.to(torch.int64), kept.to(torch.int32)


_TUNING = [0, 64]


def flash_attn_tuning(like, kv_split, kv_qb):
    """CPU: the reference attention has no launch tuning; the knobs are only remembered."""
    old = list(_TUNING)
    if kv_split >= 0:
        _TUNING[0] = int(kv_split)
    if kv_qb >= 0:
        _TUNING[1] = int(kv_qb)
    return old


for _name, _fn in list(globals().items()):
    if _name in (
        "rmsnorm_fwd", "add_rmsnorm_fwd", "rmsnorm_bwd", "rope_", "swiglu_fwd", "swiglu_bwd",
        "ce_fwd_bwd_", "ce_stats", "ce_grad_", "adamw_", "adamw_t_", "grad_sumsq_", "flash_attn_fwd", "flash_attn_bwd",
        "flash_attn_bwd_qkv", "transpose2d", "transpose_mats_", "swiglu_bwd_t", "embedding_bwd_", "flash_attn_varlen_fwd",
        "flash_attn_varlen_bwd", "flash_attn_fwd_drop", "flash_attn_bwd_drop", "flash_attn_bwd_qkv_drop", "philox_rng",
        "flash_attn_bwd_qkv_rope", "flash_attn_tuning", "layernorm_fwd", "dropout_add_layernorm_fwd", "layernorm_bwd",
        "gelu_fwd", "gelu_bwd", "gelu_bwd_t", "qk_norm_rope_fwd_", "qk_norm_rope_bwd_", "kv_cache_append_", "decode_attn",
        "sample_logits", "skinny_linear", "skinny_linear_fp8", "decode_attn_multi",
        "kv_cache_append_fp8_", "decode_attn_fp8",
    ):
        LIB.impl(_name, _fn, "CPU")
