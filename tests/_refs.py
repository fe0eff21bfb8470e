"""float64 references and error bounds for the streaming kernels (RMSNorm, RoPE, SwiGLU, cross
entropy, AdamW).  Plain torch only: the bf16 / f32 inputs are upcast and every formula is evaluated
in float64, independently of the package's own CPU ops.

A bf16 output is held to  |out - ref| <= 0.5 * bf16_ulp(ref) + f32_term : half a bf16 ulp for the
one rounding on store, plus the propagated error of evaluating the formula in f32.  An f32 output
gets the f32 term alone.  Every f32 term is derived next to its reference from the formula: one unit
roundoff U = 2^-24 per operation on the magnitudes it combines (the sum of |terms| for an add, times
the length for a reduction), times K = 8 for the summation order and the fast exp / log / rsqrt
intrinsics.  Where an f32 intermediate can fall below the smallest normal f32 a flush to zero is
allowed for as well.  None of the terms comes from a run of the code under test.
"""
import math

import torch

U = 2.0 ** -24          # f32 unit roundoff
K = 8.0                 # summation order, __expf / __logf / rsqrtf
TINY = 2.0 ** -126      # smallest normal bf16 (and f32)

RESULTS = {}            # name -> (largest error in bf16 ulps, largest error / bound), for reports


def f64(t):
    return t.detach().cpu().double()


def round_bf16(x):
    """Nearest bf16 value (ties to even) of a float64 tensor, kept in float64: one rounding, not
    the two of a cast through f32."""
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), e.clamp_min(-125) - 8)
    return torch.round(x / q) * q


def bf16_ulp(ref):
    """2^(floor(log2 |ref|) - 7), floored at the smallest normal bf16."""
    a = ref.double().abs()
    _, e = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    return torch.where(a == 0, torch.full_like(a, TINY), ulp).clamp_min(TINY)


def assert_within(out, ref, f32_term, name, max_outlier_share=0.0, outlier_tol=None):
    """|out - ref| <= 0.5 * bf16_ulp(ref) + f32_term element-wise (no half ulp for an f32 `out`).

    With `max_outlier_share` > 0 (chained roundings) that share of the elements may exceed the
    bound, and each of them must stay within `outlier_tol`.  A bf16 reference below the smallest
    normal may be stored as +-0."""
    is_bf16 = out.dtype == torch.bfloat16
    o, ref = f64(out), ref.double()
    assert o.shape == ref.shape, f"{name}: shape {tuple(o.shape)} != {tuple(ref.shape)}"
    if o.numel() == 0:
        return
    assert torch.isfinite(o).all(), f"{name}: non-finite output"
    term = torch.as_tensor(f32_term, dtype=torch.float64).expand_as(ref)
    ulp = bf16_ulp(ref)
    bound = term + 0.5 * ulp if is_bf16 else term
    err = (o - ref).abs()
    if is_bf16:
        err = torch.where((ref.abs() < TINY) & (o == 0), torch.zeros_like(err), err)
    ratio = err / bound.clamp_min(1e-300)
    w = int(torch.argmax(ratio.flatten()))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(w), ref.shape)) if ref.dim() else ()
    worst = (f"worst at {idx}: out {o.flatten()[w].item():.9g} ref {ref.flatten()[w].item():.9g} "
             f"err {err.flatten()[w].item():.3g} = {(err / ulp).flatten()[w].item():.3f} bf16 ulp, "
             f"bound {bound.flatten()[w].item():.3g} (f32 term {term.flatten()[w].item():.3g})")
    old = RESULTS.get(name, (0.0, 0.0))
    RESULTS[name] = (max(old[0], (err / ulp).max().item()), max(old[1], ratio.max().item()))
    print(f"[numerics] {name}: max {(err / ulp).max().item():.3f} bf16 ulp, max err/bound "
          f"{ratio.max().item():.3f}; {worst}")
    over = err > bound
    n_over = int(over.sum())
    if n_over == 0:
        return
    allowed = int(max_outlier_share * o.numel())
    assert n_over <= allowed, f"{name}: {n_over} of {o.numel()} elements over the bound ({allowed} allowed); {worst}"
    tol = torch.as_tensor(outlier_tol, dtype=torch.float64).expand_as(ref)
    far = over & (err > tol)
    assert not far.any(), f"{name}: {int(far.sum())} outliers beyond the chained-rounding cap; {worst}"


# ---------------------------------------------------------------------------------------------
# RMSNorm:  h = bf16(x + res),  rstd = rsqrt(mean(h^2) + eps),  n = bf16(h rstd),  y = bf16(w n)
# ---------------------------------------------------------------------------------------------
def rmsnorm_ref(x, w, eps, res=None):
    xd = f64(x)
    h = xd if res is None else round_bf16(xd + f64(res))
    rstd = torch.rsqrt((h * h).mean(-1) + eps)
    n = round_bf16(h * rstd[:, None])
    y = round_bf16(f64(w) * n)
    return h, rstd, n, y


def rmsnorm_terms(h, rstd, n, w, x=None, res=None):
    """f32 terms of `rstd`, of the unrounded product w * n that `y` is compared with, the cap of
    y's chained-rounding outliers, and (fused add) of h."""
    H = h.shape[1]
    wd = f64(w)
    # sum(h^2): U per square and H U for the H-term reduction, relative to the sum; the mean, the
    # + eps and the rsqrt add 3 U.  rstd moves by half the relative error of its argument.
    rel = K * U * (H / 2 + 4)
    t = {"rstd": rstd * rel}
    # n = h * rstd carries rstd's relative error and the product's roundoff; it is not an output,
    # but it decides how often bf16(n) lands on the other side of a rounding midpoint.
    # y = w * bf16(n) is one more product (exact for two bf16 factors, counted all the same).
    t["y"] = K * U * (wd * n).abs()
    t["y_outlier"] = 0.5 * bf16_ulp(wd * n) + t["y"] + wd.abs() * bf16_ulp(n)
    if res is not None:
        # h = x + res: one add on |x| + |res|
        t["h"] = K * U * (f64(x).abs() + f64(res).abs())
    return t


def rmsnorm_bwd_ref(dy, x, w, rstd, dres=None):
    """dx = rstd (g - n mean(g n)) (+ dres), g = dy w, n = x rstd;  dw = sum_t dy bf16(n).
    Returns dx, dw unrounded, their error magnitudes in units of U, and the largest change of dw
    that one bf16(n) landing on the neighbouring value causes."""
    dyd, xd, wd, r = f64(dy), f64(x), f64(w), f64(rstd)[:, None]
    T, H = xd.shape
    n = xd * r
    g = dyd * wd
    dot = (g * n).mean(-1, keepdim=True)
    dx = r * (g - n * dot)
    # dot: H products and an H-term reduction of |g n|, then / H: (H + 2) U mean|g n|; it reaches
    # dx through rstd |n|.  n, n * dot, the subtraction and the final product each round once on
    # |g| + |n dot|.  The optional + dres is one more add.
    dx_mag = r * n.abs() * (H + 2) * (g * n).abs().mean(-1, keepdim=True) + 4 * r * (g.abs() + (n * dot).abs())
    if dres is not None:
        dx_mag = dx_mag + dx.abs() + f64(dres).abs()
        dx = dx + f64(dres)
    nb = round_bf16(n)
    dw = (dyd * nb).sum(0)
    # dw: a T-term reduction of products of two bf16 values
    dw_mag = (T + 1) * (dyd * nb).abs().sum(0)
    dw_flip = (dyd.abs() * bf16_ulp(n)).amax(0) if T else torch.zeros(H, dtype=torch.float64)
    return dx, dw, dx_mag, dw_mag, dw_flip


# ---------------------------------------------------------------------------------------------
# RoPE:  o1 = x1 c - x2 s,  o2 = x2 c + x1 s  on the pairs (i, i + D/2) of the first nheads heads
# ---------------------------------------------------------------------------------------------
def rope_ref(x, cos, sin, pos, nheads, D, inverse):
    """Returns the unrounded result (columns past nheads * D copied through) and its f32 term."""
    xd = f64(x)
    T, half = xd.shape[0], D // 2
    v = xd[:, : nheads * D].reshape(T, nheads, D)
    x1, x2 = v[..., :half], v[..., half:]
    c = f64(cos)[pos][:, None, :]
    s = f64(sin)[pos][:, None, :]
    if inverse:
        s = -s
    out = xd.clone()
    out[:, : nheads * D] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(T, nheads * D)
    # two products (U each) and one add / subtract (U on the sum of their magnitudes)
    term = torch.zeros_like(xd)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    term[:, : nheads * D] = K * U * 2 * mag.reshape(T, nheads * D)
    return out, term


def rope_roundtrip_term(x, cos, sin, pos, nheads, D):
    """f32 term of inverse(forward(x)) against x (two roundings): the forward result is off by up
    to e = 0.5 ulp(y) + f; the inverse rotation maps that to |c| e1 + |s| e2 (the rotation is
    linear), and adds its own f on top of the half ulp assert_within allows."""
    y, f_fwd = rope_ref(x, cos, sin, pos, nheads, D, False)
    T, half = y.shape[0], D // 2
    e = (0.5 * bf16_ulp(y) + f_fwd)[:, : nheads * D].reshape(T, nheads, D)
    e1, e2 = e[..., :half], e[..., half:]
    c = f64(cos)[pos][:, None, :].abs()
    s = f64(sin)[pos][:, None, :].abs()
    _, f_inv = rope_ref(round_bf16(y), cos, sin, pos, nheads, D, True)
    term = f_inv.clone()
    term[:, : nheads * D] += torch.cat([c * e1 + s * e2, c * e2 + s * e1], -1).reshape(T, nheads * D)
    return term


# ---------------------------------------------------------------------------------------------
# SwiGLU:  h = g sigma(g) u;  du = dh g sigma,  dg = dh u sigma (1 + g (1 - sigma))
# ---------------------------------------------------------------------------------------------
def _swiglu_parts(gu):
    gud = f64(gu)
    inter = gud.shape[1] // 2
    g, u = gud[:, :inter], gud[:, inter:]
    sig, oms = torch.sigmoid(g), torch.sigmoid(-g)  # 1 - sigma without cancellation
    # sigma = 1 / (1 + exp(-g)): the exponent's error |g| 2U scales exp (+ U for exp itself), which
    # moves sigma by (1 - sigma) of that; the add and the reciprocal round once each.  Units of U.
    srel = oms * (2 * g.abs() + 1) + 2
    return g, u, sig, oms, srel


def swiglu_ref(gu):
    g, u, sig, _, _ = _swiglu_parts(gu)
    return g * sig * u


def swiglu_term(gu):
    g, u, sig, _, srel = _swiglu_parts(gu)
    # two more products; sigma below the smallest normal f32 may be flushed before it meets g u
    return K * U * (g * sig * u).abs() * (srel + 2) + (g * u).abs() * TINY


def swiglu_bwd_ref(dh, gu):
    g, u, sig, oms, _ = _swiglu_parts(gu)
    d = f64(dh)
    return torch.cat([d * u * sig * (1 + g * oms), d * g * sig], 1)


def swiglu_bwd_term(dh, gu):
    g, u, sig, oms, srel = _swiglu_parts(gu)
    d = f64(dh)
    du_t = K * U * (d * g * sig).abs() * (srel + 2) + (d * g).abs() * TINY
    # 1 - sigma: sigma's error and U on 1 + sigma.  q = 1 + g (1 - sigma): |g| times that, the
    # product's roundoff and the add's on 1 + |g (1 - sigma)|.  q passes through zero near
    # g = -1.278, so this part is absolute: |dh u sigma| times q's error.  Three more products.
    e_oms = sig * srel + 1 + sig
    q = 1 + g * oms
    e_q = g.abs() * e_oms + (g * oms).abs() + 1 + (g * oms).abs()
    dg_t = K * U * ((d * u * sig).abs() * e_q + (d * u * sig * q).abs() * (srel + 3)) + (d * u * q).abs() * TINY
    return torch.cat([dg_t, du_t], 1)


# ---------------------------------------------------------------------------------------------
# Cross entropy:  lse = m + log(s), m = max x, s = sum exp(x - m);  loss = lse - x[label];
#                 grad = (exp(x - lse) - onehot(label)) scale;  ignored rows: 0 and 0
# ---------------------------------------------------------------------------------------------
def _ce_s_rel(x, m):
    # s: a V-term reduction (V U s) of exps (U each) whose exponents x - m carry (|x| + |m|) 2U,
    # which multiplies the result.  Relative to s.
    V = x.shape[1]
    return K * U * (V + 2 * (x.abs().amax(-1) + m.abs()) + 1)


def ce_stats_ref(logits, labels, vstart):
    """One vocabulary shard: m, s, the label's logit if the label lies in this shard (else 0), and
    the f32 term of s (m and the logit are copies of inputs: exact)."""
    x = f64(logits)
    m = x.max(-1).values
    s = torch.exp(x - m[:, None]).sum(-1)
    loc = labels.cpu() - vstart
    inside = (loc >= 0) & (loc < x.shape[1])
    xl = x.gather(1, loc.clamp(0, x.shape[1] - 1)[:, None])[:, 0]
    return m, s, torch.where(inside, xl, torch.zeros_like(xl)), s * _ce_s_rel(x, m)


def ce_ref(logits, labels, ignore, scale):
    x = f64(logits)
    labels = labels.cpu()
    m = x.max(-1).values
    s = torch.exp(x - m[:, None]).sum(-1)
    lse = m + torch.log(s)
    valid = labels != ignore
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, safe[:, None])[:, 0]
    loss = torch.where(valid, lse - xl, torch.zeros_like(lse))
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    grad = (torch.exp(x - lse[:, None]) - onehot) * scale
    grad[~valid] = 0
    return loss, grad, m, s, lse


def ce_terms(logits, labels, ignore, scale):
    x = f64(logits)
    labels = labels.cpu()
    loss, _, m, s, lse = ce_ref(logits, labels, ignore, scale)
    valid = labels != ignore
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, safe[:, None])[:, 0]
    s_rel = _ce_s_rel(x, m)
    # lse = m + log(s): the relative error of s is the absolute error of log(s); the log rounds on
    # |log s| and the add on |m| + |log s|
    lse_t = s_rel + K * U * (m.abs() + 2 * torch.log(s).abs())
    # loss = lse - x[label]
    loss_t = torch.where(valid, lse_t + K * U * (lse.abs() + xl.abs()), torch.zeros_like(lse_t))
    # p = exp(x - lse): the exponent is off by (|x| + |lse|) 2U and by lse's own error, and that
    # multiplies the result; exp and the product with scale round once each
    p = torch.exp(x - lse[:, None])
    p_rel = torch.expm1(K * U * 2 * (x.abs() + lse.abs()[:, None]) + lse_t[:, None]) + 2 * K * U
    grad_t = abs(scale) * p * p_rel
    # label column: p - 1 cancels, so its term is absolute: p's error (lse's roundoff, above) plus
    # U on the magnitudes 1 + p of the subtraction and U on the product
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    grad_t = grad_t + onehot * abs(scale) * K * U * (1 + p + (p - 1).abs())
    grad_t[~valid] = 0
    return {"loss": loss_t, "grad": grad_t, "s": s * s_rel, "lse": lse_t}


# ---------------------------------------------------------------------------------------------
# AdamW (update order of the header of adamw.hip):
#   p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;
#   p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps),   g = grad * grad_scale
# ---------------------------------------------------------------------------------------------
def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale):
    """One step from the given stored values (`p` is the f32 master where there is one).  Returns
    the new p, m, v BEFORE the store rounds them -- assert_within adds the half ulp of a bf16
    store, and the update of p uses the unrounded m and v as the kernel does -- and their f32
    terms.  A caller chains steps from the stored state, where the kernel rounds."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    bc1 = 1 - beta1 ** step
    bc2 = math.sqrt(1 - beta2 ** step)
    gs = g * grad_scale
    p1 = p * (1 - lr * wd)
    d = gs - m
    m1 = m + d * (1 - beta1)
    gg = gs * gs
    v1 = v * beta2 + (1 - beta2) * gg
    den = v1.sqrt() / bc2 + eps
    upd = (lr / bc1) * m1 / den
    p2 = p1 - upd
    # In units of U.  gs is one product.  1 - beta in f32: U (1 + beta) for the subtraction and
    # U beta for beta's own conversion.  A result below the smallest normal f32 may be flushed.
    e_1mb1, e_1mb2 = 1 + 2 * beta1, 1 + 2 * beta2
    # m' = m + (gs - m)(1 - b1): the difference (gs's error, U on |gs| + |m|), times 1 - b1 (its
    # error on |d|, the product's roundoff), then the add on |m| + |d (1 - b1)|
    e_d = 2 * gs.abs() + m.abs()
    e_m = d.abs() * e_1mb1 + (1 - beta1) * (e_d + d.abs()) + m.abs() + (1 - beta1) * d.abs()
    m_t = K * U * e_m + TINY
    # v' = v b2 + (1 - b2) gs gs: b2's conversion and the product on |v b2|; the error of 1 - b2 on
    # gs^2, gs's error twice and two products on (1 - b2) gs^2; the add on both
    e_v = 3 * v.abs() * beta2 + gg * e_1mb2 + 5 * (1 - beta2) * gg
    v_t = K * U * e_v + TINY
    # decay = 1 - lr wd: two conversions, a product and a subtraction, U (1 + 4 lr wd); p * decay
    # rounds once more
    e_p1 = p.abs() * (2 + 4 * abs(lr * wd))
    # den = sqrt(v') / bc2 + eps: v's error through the square root (taken as the width of the
    # interval, finite at v' = 0), then sqrt, bc2's conversion, the division, eps's conversion and
    # the add.  update = (lr / bc1) m' / den: m's error, den's relative error, and two conversions,
    # two divisions and a product.
    sq_w = (v1 + v_t).sqrt() - (v1 - v_t).clamp_min(0).sqrt()
    den_t = sq_w / bc2 + K * U * (3 * v1.sqrt() / bc2 + eps + den)
    upd_t = (lr / bc1) / den * m_t + upd.abs() / den * den_t + K * U * 5 * upd.abs()
    # p' = p decay - update
    p_t = K * U * (e_p1 + p1.abs() + upd.abs()) + upd_t
    return p2, m1, v1, {"p": p_t, "m": m_t, "v": v_t}
