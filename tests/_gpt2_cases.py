"""Cases, float64 references and bounds of the GPT-2 streaming kernels (layernorm.hip, gelu.hip),
shared by test_gpt2_kernels_gpu.py (the gfx950 kernels) and test_gpt2_kernels_cpu.py (the package's
CPU ops).  Conventions of tests/_refs.py: a bf16 output is held to half a bf16 ulp plus an f32 term,
an f32 output to the f32 term alone; every term is derived here from the formula (U per operation on
the magnitudes it combines, the length for a reduction, K for the summation order and the fast
intrinsics), none comes from a run of the code under test.
"""
import math

import torch

import dtg  # noqa: F401
from dtg import ops  # noqa: F401  (registers torch.ops.dtg)
from dtg.ops import _cpu as cpu_ops
import _refs as R
from _kernel_cases import BF, KU, OUTLIERS, _cpu, _gen

dops = torch.ops.dtg
U, K, TINY = R.U, R.K, R.TINY
EPS = 1e-5

# ------------------------------------------------------------------------------- LayerNorm
# 768 / 1600: GPT-2 and GPT-2-XL (lanes past the row); the others are the full and just-over PER edges
LN_HIDDEN = [8, 768, 1600, 2048, 2056, 4104, 8200, 16384]
LN_BWD_T = [1, 513, 1025]      # rows per block 1, 2, 3; the last block is short for 513 and 1025
LN_BWD_HIDDEN = [768, 2056, 8200]
OFFSET_ROW, EQUAL_ROW = 3, 4   # rows of ln_inputs(5, H)


def ln_inputs(T, H, seed=0):
    """x, residual, w, b, dy, dres.  For T = 5: row 3 of x is 64 + 0.5 randn (bf16 ulp 0.5 there: the
    row that a one-pass variance gets wrong), row 4 is all 1.5 (variance exactly 0); the residual
    is 0 on those two rows, so they reach the fused form's h unchanged."""
    g = _gen(seed)
    x = torch.randn(T, H, generator=g)
    res = torch.randn(T, H, generator=g)
    if T == 5:
        x[OFFSET_ROW] = 64 + 0.5 * torch.randn(H, generator=g)
        x[EQUAL_ROW] = 1.5
        res[OFFSET_ROW:] = 0
    w = 1 + 0.1 * torch.randn(H, generator=g)
    b = 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(T, H, generator=g)
    dres = torch.randn(T, H, generator=g)
    return tuple(t.to(BF) for t in (x, res, w, b, dy, dres))


def ln_ref(h, w, b, eps):
    """h: float64 values of the (bf16) rows.  mean, rstd, n = (h - mean) rstd, y = n w + b."""
    mean = h.mean(-1)
    d = h - mean[:, None]
    var = (d * d).mean(-1)
    rstd = torch.rsqrt(var + eps)
    n = d * rstd[:, None]
    return mean, var, rstd, n, n * R.f64(w) + R.f64(b)


def ln_terms(h, w, b, eps):
    """f32 terms of mean, rstd and y for a two-pass evaluation (mean, then the centred squares).

    mean: an H-term reduction, K U (H + 1) mean|h| -- unless every partial sum is exact: the row's
    values are multiples of q (its smallest bf16 ulp), so while sum|h| < 2^24 q every partial sum, in
    any order, is a multiple of q below 2^24 q and an f32 holds it exactly; then only the division
    rounds.  Call the mean's error delta.
    rstd: delta reaches the variance only as delta^2 (sum (h - m')^2 = sum (h - m)^2 + H delta^2).
    h - m' rounds once relative to the result (both are exact f32 values), the square once, the
    H-term reduction H times, all relative to the sum of positive terms; / H, + eps and rsqrt add
    three.  rstd moves by half the relative error of its argument: K U (H / 2 + 3) + delta^2 / 2(var + eps).

    Why a one-pass f32 variance E[h^2] - mean^2 exceeds this on the offset row (mean 64, spread 0.5):
    E[h^2] and mean^2 are both ~4096, so each rounds at U * 4096 = 2.4e-4 (and E[h^2] carries its
    reduction's roundings on top), against a variance of 0.25: up to ~1e-3 of the variance, ~5e-4 of
    rstd, whatever H is.  The sums of that row are exact (above), so delta^2 is nothing and the bound
    is K U (H / 2 + 3): 1.8e-4 at H = 768, 3.8e-4 at 1600, 4.9e-4 at 2048, beyond the one-pass error
    from H ~ 4000 on (K U H is a worst case; no tighter claim is made here).  How much of those
    roundings a given row realises is chance -- and for H a small power of two none: the squares
    of bf16 values and their short sums are exact in f32 -- so the CPU suite shows the rejection at
    1600 and 2048, where the realised error is 1.4 - 1.8 times the bound.
    y = (h - mean) rstd w + b: the subtraction on |h| + |mean| (this admits h rstd - mean rstd, the
    order of ATen's CPU kernel, as well), delta, rstd's error, two products and the add."""
    H = h.shape[1]
    mean, var, rstd, n, _ = ln_ref(h, w, b, eps)
    wd, bd = R.f64(w), R.f64(b)
    q = torch.where(h == 0, torch.full_like(h, float("inf")), R.bf16_ulp(h)).amin(-1)
    exact = h.abs().sum(-1) < 2.0 ** 24 * q
    delta = torch.where(exact, K * U * mean.abs(), K * U * (H + 1) * h.abs().mean(-1))
    rel = K * U * (H / 2 + 3) + delta ** 2 / (2 * (var + eps))
    d_t = delta[:, None] + K * U * (h.abs() + mean.abs()[:, None])
    n_t = rstd[:, None] * d_t + n.abs() * (rel[:, None] + K * U)
    y_t = wd.abs() * n_t + K * U * (2 * (n * wd).abs() + bd.abs())
    return {"mean": delta, "rstd": rstd * rel, "y": y_t}


def check_ln_outputs(y, mean, rstd, h64, w, b, eps, tag):
    mean_r, _, rstd_r, _, y_r = ln_ref(h64, w, b, eps)
    t = ln_terms(h64, w, b, eps)
    R.assert_within(mean, mean_r, t["mean"], f"{tag} mean")
    R.assert_within(rstd, rstd_r, t["rstd"], f"{tag} rstd")
    R.assert_within(y, y_r, t["y"], f"{tag} y")
    return mean_r, rstd_r


def check_layernorm_hidden(dev, H):
    x, res, w, b, _, _ = ln_inputs(5, H, seed=H)
    y, mean, rstd = dops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), EPS)
    assert mean.dtype == rstd.dtype == torch.float32 and mean.shape == rstd.shape == (5,) and y.dtype == BF
    _, rstd_r = check_ln_outputs(y, mean, rstd, R.f64(x), w, b, EPS, "layernorm_fwd")
    assert abs(rstd_r[EQUAL_ROW].item() * EPS ** 0.5 - 1) < 1e-12  # the reference: variance exactly 0 there
    y2, h2, mean2, rstd2 = dops.dropout_add_layernorm_fwd(x.to(dev), res.to(dev), w.to(dev), b.to(dev), EPS, 0.0, None)
    R.assert_within(h2, R.f64(x) + R.f64(res), KU * (R.f64(x).abs() + R.f64(res).abs()), "dropout_add_layernorm_fwd h")
    assert torch.equal(_cpu(h2)[OFFSET_ROW:], x[OFFSET_ROW:])
    check_ln_outputs(y2, mean2, rstd2, R.f64(h2), w, b, EPS, "dropout_add_layernorm_fwd")


def one_pass_rstd(x, eps):
    """The form the kernels must not use: f32 E[x^2] - mean^2."""
    xf = x.float()
    return torch.rsqrt((xf * xf).mean(-1) - xf.mean(-1) ** 2 + eps)


def ln_bwd_ref(dy, h, w, mean, rstd, dres=None):
    """dh = rstd (g - mean(g) - n mean(g n)) (+ dres), g = dy w, n = (h - mean) rstd; dw = sum_t dy n;
    db = sum_t dy, from the given f32 mean / rstd.  Unrounded, with error magnitudes in units of U.
    mean(g): an H-term reduction of products, (H + 1) mean|g|.  mean(g n): n rounds twice more,
    (H + 4) mean|g n|; it reaches dh through rstd |n|.  g, n, n * mean(g n), the two subtractions
    and the final product round once each on |g| + |mean(g)| + |n mean(g n)|; + dres is one more add."""
    dyd, hd, wd = R.f64(dy), R.f64(h), R.f64(w)
    m, r = R.f64(mean)[:, None], R.f64(rstd)[:, None]
    T, H = hd.shape
    n = (hd - m) * r
    g = dyd * wd
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * n).mean(-1, keepdim=True)
    dh = r * (g - c1 - n * c2)
    dh_mag = (r * ((H + 1) * g.abs().mean(-1, keepdim=True) + n.abs() * (H + 4) * (g * n).abs().mean(-1, keepdim=True))
              + 4 * r * (g.abs() + c1.abs() + (n * c2).abs()))
    if dres is not None:
        dh_mag = dh_mag + dh.abs() + R.f64(dres).abs()
        dh = dh + R.f64(dres)
    # T-term reductions; dy n is a product of a bf16 value and a twice-rounded n
    dw = (dyd * n).sum(0)
    dw_mag = (T + 3) * (dyd * n).abs().sum(0)
    db = dyd.sum(0)
    db_mag = (T + 1) * dyd.abs().sum(0)
    return dh, dw, db, dh_mag, dw_mag, db_mag


def _with_flip(out_ref, term):
    """The outlier cap rmsnorm_bwd's dw gets: the bound plus one flipped bf16 rounding of the result."""
    return 0.5 * R.bf16_ulp(out_ref) + term + R.bf16_ulp(out_ref)


def check_layernorm_bwd(dev, dy, h, w, mean, rstd, dres):
    args = [dy.to(dev), h.to(dev), w.to(dev), mean.to(dev), rstd.to(dev), None if dres is None else dres.to(dev), 0.0,
            None]
    dh, dx, dw, db = dops.layernorm_bwd(*args)
    dh_r, dw_r, db_r, dh_mag, dw_mag, db_mag = ln_bwd_ref(dy, h, w, mean, rstd, dres)
    tag = "layernorm_bwd" if dres is None else "layernorm_bwd+dres"
    assert torch.equal(dx, dh), "p == 0: dx is dh"
    R.assert_within(dh, dh_r, KU * dh_mag, f"{tag} dh", OUTLIERS, _with_flip(dh_r, KU * dh_mag))
    R.assert_within(dw, dw_r, KU * dw_mag, f"{tag} dw", OUTLIERS, _with_flip(dw_r, KU * dw_mag))
    R.assert_within(db, db_r, KU * db_mag, f"{tag} db", OUTLIERS, _with_flip(db_r, KU * db_mag))
    again = dops.layernorm_bwd(*args)
    assert all(torch.equal(a, c) for a, c in zip((dh, dx, dw, db), again)), "layernorm_bwd is not reproducible bit for bit"


def _ln_stats32(x, w, b):
    mean, _, rstd, _, _ = ln_ref(R.f64(x), w, b, EPS)
    return mean.float(), rstd.float()


def check_layernorm_bwd_rows(dev, T, with_dres):
    x, _, w, b, dy, dres = ln_inputs(T, 128, seed=T)
    mean, rstd = _ln_stats32(x, w, b)
    check_layernorm_bwd(dev, dy, x, w, mean, rstd, dres if with_dres else None)


def check_layernorm_bwd_hidden(dev, H, with_dres):
    x, _, w, b, dy, dres = ln_inputs(5, H, seed=H)
    mean, rstd = _ln_stats32(x, w, b)
    check_layernorm_bwd(dev, dy, x, w, mean, rstd, dres if with_dres else None)


RNG = (0x0123456789ABCDEF, (1 << 33) + 12)  # seed and offset both use their high words


def _rng(dev, offset=RNG[1]):
    return torch.tensor([RNG[0], offset], dtype=torch.int64).to(dev)


def check_layernorm_strided(dev):
    """x / residual / h as column slices of wider buffers (of different widths), dy non-contiguous:
    the same bits as for contiguous copies, with and without dropout."""
    T, H = 7, 2056
    g = _gen(11)
    xbuf = torch.randn(T, H + 16, generator=g).to(BF)
    rbuf = torch.randn(T, H + 24, generator=g).to(BF)
    _, _, w, b, dy, dres = ln_inputs(T, H, seed=12)
    xs, rs = xbuf.to(dev)[:, 8:8 + H], rbuf.to(dev)[:, 16:16 + H]
    xc, rc = xs.contiguous(), rs.contiguous()
    assert xs.stride(0) == H + 16 and rs.stride(0) == H + 24 and xc.stride(0) == H
    wd, bd = w.to(dev), b.to(dev)
    for a, c in zip(dops.layernorm_fwd(xs, wd, bd, EPS), dops.layernorm_fwd(xc, wd, bd, EPS)):
        assert torch.equal(a, c), "layernorm_fwd: strided x"
    _, mean, rstd = dops.layernorm_fwd(xc, wd, bd, EPS)
    dyc = dy.to(dev)
    dys = dyc.t().contiguous().t()
    assert not dys.is_contiguous()
    for p, rng in ((0.0, None), (0.5, _rng(dev))):
        for a, c in zip(dops.dropout_add_layernorm_fwd(xs, rs, wd, bd, EPS, p, rng),
                        dops.dropout_add_layernorm_fwd(xc, rc, wd, bd, EPS, p, rng)):
            assert torch.equal(a, c), "dropout_add_layernorm_fwd: strided x / residual"
        for dr in (None, dres.to(dev)):
            for a, c in zip(dops.layernorm_bwd(dys, xs, wd, mean, rstd, dr, p, rng),
                            dops.layernorm_bwd(dyc, xc, wd, mean, rstd, dr, p, rng)):
                assert torch.equal(a, c), "layernorm_bwd: strided h / non-contiguous dy"


def check_layernorm_empty(dev):
    H = 64
    x = torch.zeros(0, H, dtype=BF, device=dev)
    w = torch.ones(H, dtype=BF, device=dev)
    y, mean, rstd = dops.layernorm_fwd(x, w, w, EPS)
    assert y.shape == (0, H) and y.dtype == BF and mean.shape == rstd.shape == (0,) and mean.dtype == torch.float32
    for p, rng in ((0.0, None), (0.5, _rng(dev))):
        y, h, mean, rstd = dops.dropout_add_layernorm_fwd(x, x, w, w, EPS, p, rng)
        assert y.shape == h.shape == (0, H) and mean.shape == rstd.shape == (0,)
        for dres in (None, x):
            dh, dx, dw, db = dops.layernorm_bwd(x, x, w, mean, rstd, dres, p, rng)
            assert dh.shape == dx.shape == (0, H) and dw.shape == db.shape == (H,) and dw.dtype == BF
            assert torch.count_nonzero(dw) == 0 and torch.count_nonzero(db) == 0


def check_layernorm_bad_layouts(dev, raises):
    """`raises`: pytest.raises.  H not a multiple of 8, a non-unit inner stride, rng with p == 0."""
    w12 = torch.ones(12, dtype=BF, device=dev)
    x12 = torch.zeros(4, 12, dtype=BF, device=dev)
    w16 = torch.ones(16, dtype=BF, device=dev)
    wide = torch.zeros(4, 32, dtype=BF, device=dev)
    x16 = torch.zeros(4, 16, dtype=BF, device=dev)
    st = torch.ones(4, device=dev)
    for x, w in ((x12, w12), (wide[:, ::2], w16)):
        with raises(RuntimeError):
            dops.layernorm_fwd(x, w, w, EPS)
        with raises(RuntimeError):
            dops.dropout_add_layernorm_fwd(x, x, w, w, EPS, 0.0, None)
        with raises(RuntimeError):
            dops.layernorm_bwd(x, x, w, st, st, None, 0.0, None)
    with raises(RuntimeError, match="rng given with p == 0"):
        dops.dropout_add_layernorm_fwd(x16, x16, w16, w16, EPS, 0.0, _rng(dev))
    with raises(RuntimeError, match="rng given with p == 0"):
        dops.layernorm_bwd(x16, x16, w16, st, st, None, 0.0, _rng(dev))


# --------------------------------------------------------------------------------- dropout
DROP_T, DROP_H = 64, 768


def check_dropout(dev, p):
    """residual = 0 and |x| >= 1, so h == 0 exactly marks a dropped element."""
    g = _gen(int(p * 100))
    x = torch.randn(DROP_T, DROP_H, generator=g)
    x = (torch.sign(x) + x).to(BF)
    assert (x.float().abs() >= 1).all()
    _, _, w, b, dy, dres = ln_inputs(DROP_T, DROP_H, seed=7)
    zero = torch.zeros_like(x)
    thr, scale = cpu_ops.dropout_threshold(p)
    xd, zd, wd, bd = x.to(dev), zero.to(dev), w.to(dev), b.to(dev)
    y, h, mean, rstd = dops.dropout_add_layernorm_fwd(xd, zd, wd, bd, EPS, p, _rng(dev))
    keep = cpu_ops.ln_dropout_keep(RNG[0], RNG[1], DROP_T, DROP_H, p)
    assert torch.equal(_cpu(h) != 0, keep), "keep mask differs from the Philox function of dtg.ops._cpu"
    q, n = thr / 256.0, keep.numel()
    share = keep.double().mean().item()
    sigma = math.sqrt(q * (1 - q) / n)
    print(f"[dropout] p {p}: keep share {share:.5f}, thr / 256 {q:.5f}, sigma {sigma:.2e}")
    assert abs(share - q) <= 5 * sigma
    # kept values: bf16(x * scale), one product
    R.assert_within(h, R.f64(x) * scale * keep, KU * (R.f64(x) * scale).abs(), "dropout h")
    check_ln_outputs(y, mean, rstd, R.f64(h), w, b, EPS, "dropout_add_layernorm_fwd (p > 0)")
    again = dops.dropout_add_layernorm_fwd(xd, zd, wd, bd, EPS, p, _rng(dev))
    assert all(torch.equal(a, c) for a, c in zip((y, h, mean, rstd), again)), "the same rng must give the same bits"
    h_other = dops.dropout_add_layernorm_fwd(xd, zd, wd, bd, EPS, p, _rng(dev, RNG[1] + 4))[1]
    assert not torch.equal(_cpu(h_other) != 0, keep), "another offset must give another mask"
    # backward: dx = 0 exactly where dropped, bf16(scale * dh_f32) elsewhere (from the f32 dh)
    hc, mc, rc = _cpu(h), _cpu(mean), _cpu(rstd)
    for dr in (None, dres):
        dh, dx, dw, db = dops.layernorm_bwd(dy.to(dev), h, wd, mean, rstd, None if dr is None else dr.to(dev), p, _rng(dev))
        dh_r, dw_r, db_r, dh_mag, dw_mag, db_mag = ln_bwd_ref(dy, hc, w, mc, rc, dr)
        R.assert_within(dh, dh_r, KU * dh_mag, "layernorm_bwd (p > 0) dh", OUTLIERS, _with_flip(dh_r, KU * dh_mag))
        R.assert_within(dw, dw_r, KU * dw_mag, "layernorm_bwd (p > 0) dw", OUTLIERS, _with_flip(dw_r, KU * dw_mag))
        R.assert_within(db, db_r, KU * db_mag, "layernorm_bwd (p > 0) db", OUTLIERS, _with_flip(db_r, KU * db_mag))
        dxc = _cpu(dx)
        assert torch.count_nonzero(dxc[~keep]) == 0, "dx must be exactly 0 on dropped elements"
        # one more product on top of dh's f32 term, then the one rounding
        R.assert_within(dxc[keep], scale * dh_r[keep], scale * KU * dh_mag[keep] + KU * (scale * dh_r[keep]).abs(),
                        "layernorm_bwd (p > 0) dx")


# ------------------------------------------------------------------------------------ GELU
# -0.7578125 < zero of gelu' < -0.75; exp(-2u) overflows from x ~ -10 down
GELU_X = [0.0, 2.0 ** -20, -2.0 ** -20, -0.75, -0.7578125, 10.0, -10.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
GELU_DH = [1.0, -1.0, 3.5, -3.5]
GELU_C = math.sqrt(2.0 / math.pi)
GELU_A = 0.044715


def gelu_inputs(T, I):
    """x and dh [T, I]: the grid of x crossed with dh first (as much of it as fits), random after."""
    n = T * I
    g = _gen(T * 1000 + I)
    idx = torch.arange(n)
    nx, nd = len(GELU_X), len(GELU_DH)
    grid = idx < nx * nd
    x = torch.where(grid, torch.tensor(GELU_X)[idx % nx], 2 * torch.randn(n, generator=g))
    dh = torch.where(grid, torch.tensor(GELU_DH)[(idx // nx) % nd], torch.randn(n, generator=g))
    return x.view(T, I).to(BF), dh.view(T, I).to(BF)


def _gelu_parts(x):
    xd = R.f64(x)
    u = GELU_C * (xd + GELU_A * xd ** 3)
    umag = GELU_C * (xd.abs() + GELU_A * xd.abs() ** 3)
    sig, oms = torch.sigmoid(2 * u), torch.sigmoid(-2 * u)  # 1 - sigma without cancellation
    # u: x^3 (two products), * a, the add, * c: 5 U on umag, doubled into the exponent 2u, which scales
    # exp (+ U for exp itself) and moves sigma by (1 - sigma) of that; the add and the reciprocal round
    # once each.  Units of U.
    srel = oms * (10 * umag + 1) + 2
    return xd, sig, oms, srel


def gelu_ref(x):
    xd, sig, _, _ = _gelu_parts(x)
    return xd * sig


def gelu_term(x):
    """x sigma(2u): sigma's error and one product; a sigma below the smallest normal f32 may be
    flushed.  The K U 1.5 |x| admits the form 0.5 x (1 + tanh u) as well (ATen, which the CPU op
    calls): tanh and 1 + tanh round at U of 1, not of 1 + tanh, so x's negative tail loses relative
    accuracy there."""
    xd, sig, _, srel = _gelu_parts(x)
    return K * U * ((xd * sig).abs() * (srel + 1) + 1.5 * xd.abs()) + xd.abs() * TINY


def _gelu_grad_parts(x):
    xd, sig, oms, srel = _gelu_parts(x)
    up = 2 * GELU_C * (1 + 3 * GELU_A * xd * xd)
    return xd, sig, oms, srel, up, xd * sig * oms * up


def gelu_bwd_ref(dh, x):
    _, sig, _, _, _, t = _gelu_grad_parts(x)
    return R.f64(dh) * (sig + t)


def gelu_bwd_term(dh, x):
    """dh (sigma + t), t = x sigma (1 - sigma) 2u'.  1 - sigma: sigma's error and U on 1 + sigma.
    2u' = 2c (1 + 3a x^2): four roundings.  t: three products more.  sigma + t passes through zero
    near x = -0.7535, so the sum's error is absolute: both parts' errors and U on sigma + |t|; then
    the product with dh.  A flushed sigma moves the result by |dh| (1 + |x 2u'|) TINY."""
    xd, sig, oms, srel, up, t = _gelu_grad_parts(x)
    d = R.f64(dh)
    e_sig = sig * srel
    e_oms = sig * srel + 1 + sig
    e_t = (xd * up).abs() * (oms * e_sig + sig * e_oms) + 7 * t.abs()
    e_q = e_sig + e_t + sig + t.abs()
    return K * U * (d.abs() * e_q + (d * (sig + t)).abs()) + d.abs() * (1 + (xd * up).abs()) * TINY


def _strided(x, dev):
    T, C = x.shape
    buf = torch.full((T, C + 16), 7.0, dtype=BF)
    buf[:, 8:8 + C] = x
    view = buf.to(dev)[:, 8:8 + C]
    assert view.stride(0) == C + 16
    return view


def check_gelu(dev, T, I):
    x, dh = gelu_inputs(T, I)
    h = dops.gelu_fwd(x.to(dev))
    R.assert_within(h, gelu_ref(x), gelu_term(x), "gelu_fwd")          # asserts finiteness too
    dx = dops.gelu_bwd(dh.to(dev), x.to(dev))
    R.assert_within(dx, gelu_bwd_ref(dh, x), gelu_bwd_term(dh, x), "gelu_bwd")
    xs = _strided(x, dev)
    assert torch.equal(dops.gelu_fwd(xs), h), "gelu_fwd: strided x"
    assert torch.equal(dops.gelu_bwd(dh.to(dev), xs), dx), "gelu_bwd: strided x"


def check_gelu_bwd_t(dev, T, I):
    x, dh = gelu_inputs(T, I)
    xs = _strided(x, dev)
    dx, dx_t, h_t = dops.gelu_bwd_t(dh.to(dev), xs)
    assert dx.shape == (T, I) and dx_t.shape == (I, T) and h_t.shape == (I, T)
    # one functor behind the tiled and the untiled kernels: the same bits
    assert torch.equal(dx, dops.gelu_bwd(dh.to(dev), xs)), "gelu_bwd_t: dx != gelu_bwd"
    assert torch.equal(h_t.t(), dops.gelu_fwd(xs)), "gelu_bwd_t: h_t.t() != gelu_fwd"
    R.assert_within(dx, gelu_bwd_ref(dh, x), gelu_bwd_term(dh, x), "gelu_bwd_t dx")
    assert torch.equal(dx_t, dx.t()), "gelu_bwd_t: dx_t != dx.t()"
    R.assert_within(h_t.t(), gelu_ref(x), gelu_term(x), "gelu_bwd_t h_t")


def check_gelu_empty(dev):
    x = torch.zeros(0, 16, dtype=BF, device=dev)
    assert dops.gelu_fwd(x).shape == (0, 16)
    assert dops.gelu_bwd(x, x).shape == (0, 16)
    dx, dx_t, h_t = dops.gelu_bwd_t(x, x)
    assert dx.shape == (0, 16) and dx_t.shape == (16, 0) and h_t.shape == (16, 0)
