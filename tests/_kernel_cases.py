"""Cases and checks shared by test_kernel_numerics_gpu.py (the gfx950 kernels) and
test_kernel_refs_cpu.py (the package's f32 CPU ops): the same inputs, the same float64 references
and the same bounds (tests/_refs.py), on whichever device `dev` names.  Inputs are generated on the
CPU from fixed seeds.
"""
import pytest
import torch

import dtg  # noqa: F401
from dtg import ops  # noqa: F401  (registers torch.ops.dtg)
import _refs as R

dops = torch.ops.dtg
BF = torch.bfloat16
OUTLIERS = 1e-3  # share of elements a chained rounding may push past the single-rounding bound
IGNORE = -100
KU = R.K * R.U


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cpu(t):
    return t.detach().cpu()


# --------------------------------------------------------------------------------- RMSNorm
# every PER of pick_per (1, 2, 4, 8) with a full last pass, a row that ends in the first chunk of
# the last pass (PER 2, 4, 8), and H = 5120 (PER 4, last pass half used)
RMS_HIDDEN = [8, 2048, 4096, 8192, 16384, 2056, 4104, 8200, 5120]
RMS_BWD_T = [1, 513, 1025, 1537]  # rows per block 1, 2, 3, 4; the last block is short for 513..1537


def rms_inputs(T, H, seed=0):
    g = _gen(seed)
    x = torch.randn(T, H, generator=g).to(BF)
    res = torch.randn(T, H, generator=g).to(BF)
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    dy = torch.randn(T, H, generator=g).to(BF)
    dres = torch.randn(T, H, generator=g).to(BF)
    return x, res, w, dy, dres


def check_rmsnorm_fwd(dev, x, res, w, eps):
    """rmsnorm_fwd and add_rmsnorm_fwd against the reference; returns the reference rstd (f32)."""
    y, rstd = dops.rmsnorm_fwd(x.to(dev), w.to(dev), eps)
    h_r, rstd_r, n_r, _ = R.rmsnorm_ref(x, w, eps)
    t = R.rmsnorm_terms(h_r, rstd_r, n_r, w)
    R.assert_within(rstd, rstd_r, t["rstd"], "rmsnorm_fwd rstd")
    R.assert_within(y, R.f64(w) * n_r, t["y"], "rmsnorm_fwd y", OUTLIERS, t["y_outlier"])
    y2, h2, rstd2 = dops.add_rmsnorm_fwd(x.to(dev), res.to(dev), w.to(dev), eps)
    h_r, rstd2_r, n_r, _ = R.rmsnorm_ref(x, w, eps, res)
    t = R.rmsnorm_terms(h_r, rstd2_r, n_r, w, x, res)
    R.assert_within(h2, R.f64(x) + R.f64(res), t["h"], "add_rmsnorm_fwd h")
    R.assert_within(rstd2, rstd2_r, t["rstd"], "add_rmsnorm_fwd rstd")
    R.assert_within(y2, R.f64(w) * n_r, t["y"], "add_rmsnorm_fwd y", OUTLIERS, t["y_outlier"])
    return rstd_r.float(), _cpu(y)


def check_rmsnorm_bwd(dev, dy, x, w, rstd, dres):
    args = [dy.to(dev), x.to(dev), w.to(dev), rstd.to(dev), None if dres is None else dres.to(dev)]
    dx, dw = dops.rmsnorm_bwd(*args)
    dx_r, dw_r, dx_mag, dw_mag, dw_flip = R.rmsnorm_bwd_ref(dy, x, w, rstd, dres)
    tag = "rmsnorm_bwd" if dres is None else "rmsnorm_bwd+dres"
    R.assert_within(dx, dx_r, KU * dx_mag, f"{tag} dx")
    dw_t = KU * dw_mag
    R.assert_within(dw, dw_r, dw_t, f"{tag} dw", OUTLIERS, 0.5 * R.bf16_ulp(dw_r) + dw_t + dw_flip)
    dx2, dw2 = dops.rmsnorm_bwd(*args)
    assert torch.equal(dw, dw2) and torch.equal(dx, dx2), "rmsnorm_bwd is not reproducible bit for bit"
    return _cpu(dx)


def check_rmsnorm_hidden(dev, H):
    x, res, w, _, _ = rms_inputs(5, H, seed=H)
    check_rmsnorm_fwd(dev, x, res, w, 1e-5)


def check_rmsnorm_bwd_rows(dev, T, with_dres):
    x, _, w, dy, dres = rms_inputs(T, 128, seed=T)
    rstd = R.rmsnorm_ref(x, w, 1e-5)[1].float()
    check_rmsnorm_bwd(dev, dy, x, w, rstd, dres if with_dres else None)


def check_rmsnorm_bwd_hidden(dev, H):
    """The backward's PER paths (the issue's hidden sizes, T = 5, no dres: the trainer's launch)."""
    x, _, w, dy, _ = rms_inputs(5, H, seed=H)
    rstd = R.rmsnorm_ref(x, w, 1e-5)[1].float()
    check_rmsnorm_bwd(dev, dy, x, w, rstd, None)


def check_rmsnorm_strided(dev):
    """x and residual as column slices of wider buffers (of different widths), dy non-contiguous:
    the same bits as for contiguous copies."""
    T, H = 7, 2056
    g = _gen(11)
    xbuf = torch.randn(T, H + 16, generator=g).to(BF)
    rbuf = torch.randn(T, H + 24, generator=g).to(BF)
    _, _, w, dy, dres = rms_inputs(T, H, seed=12)
    xs, rs = xbuf.to(dev)[:, 8:8 + H], rbuf.to(dev)[:, 16:16 + H]
    xc, rc = xs.contiguous(), rs.contiguous()
    assert xs.stride(0) == H + 16 and rs.stride(0) == H + 24 and xc.stride(0) == H
    wd = w.to(dev)
    y_s, rstd_s = dops.rmsnorm_fwd(xs, wd, 1e-5)
    y_c, rstd_c = dops.rmsnorm_fwd(xc, wd, 1e-5)
    assert torch.equal(y_s, y_c) and torch.equal(rstd_s, rstd_c), "rmsnorm_fwd: strided x"
    for a, b in zip(dops.add_rmsnorm_fwd(xs, rs, wd, 1e-5), dops.add_rmsnorm_fwd(xc, rc, wd, 1e-5)):
        assert torch.equal(a, b), "add_rmsnorm_fwd: strided x / residual"
    dyc = dy.to(dev)
    dys = dyc.t().contiguous().t()
    assert not dys.is_contiguous()
    for dr in (None, dres.to(dev)):
        for a, b in zip(dops.rmsnorm_bwd(dys, xs, wd, rstd_c, dr), dops.rmsnorm_bwd(dyc, xc, wd, rstd_c, dr)):
            assert torch.equal(a, b), "rmsnorm_bwd: strided x / non-contiguous dy"
    # and the strided results are the right ones
    x = xbuf[:, 8:8 + H].contiguous()
    h_r, rstd_r, n_r, _ = R.rmsnorm_ref(x, w, 1e-5)
    t = R.rmsnorm_terms(h_r, rstd_r, n_r, w)
    R.assert_within(y_s, R.f64(w) * n_r, t["y"], "rmsnorm_fwd y (strided)", OUTLIERS, t["y_outlier"])


def check_rmsnorm_eps(dev, eps):
    """Rows where eps decides rstd (mean(x^2) ~ 1e-6 and an all-zero row) and rows where it must not
    matter (scaled by 1e3)."""
    H = 128
    x, res, w, dy, _ = rms_inputs(6, H, seed=21)
    scale = torch.tensor([1e-3, 1e-3, 0.0, 1e3, 1e3, 1.0])[:, None]
    x = (x.float() * scale).to(BF)
    res = (res.float() * scale).to(BF)
    rstd, y = check_rmsnorm_fwd(dev, x, res, w, eps)
    assert torch.count_nonzero(y[2]) == 0, "y of an all-zero row"
    assert abs(rstd[2].item() * eps ** 0.5 - 1) < 1e-6  # the reference itself: rstd == eps^-1/2 there
    dx = check_rmsnorm_bwd(dev, dy, x, w, rstd, None)
    # all-zero row: n = 0, so dx = rstd * dy * w exactly as the formula reduces
    R.assert_within(dx[2], rstd[2].double() * R.f64(dy[2]) * R.f64(w), KU * 4 * rstd[2].double() * (R.f64(dy[2]) * R.f64(w)).abs(),
                    "rmsnorm_bwd dx (zero row)")


def check_rmsnorm_empty(dev):
    H = 64
    x = torch.zeros(0, H, dtype=BF, device=dev)
    w = torch.ones(H, dtype=BF, device=dev)
    y, rstd = dops.rmsnorm_fwd(x, w, 1e-5)
    assert y.shape == (0, H) and y.dtype == BF and rstd.shape == (0,) and rstd.dtype == torch.float32
    y, h, rstd = dops.add_rmsnorm_fwd(x, x, w, 1e-5)
    assert y.shape == (0, H) and h.shape == (0, H) and rstd.shape == (0,)
    for dres in (None, x):
        dx, dw = dops.rmsnorm_bwd(x, x, w, rstd, dres)
        assert dx.shape == (0, H) and dw.shape == (H,) and dw.dtype == BF and torch.count_nonzero(dw) == 0


# ------------------------------------------------------------------------------------ RoPE
ROPE_MAX_POS = 64


def rope_tables(D, max_pos=ROPE_MAX_POS, theta=10000.0):
    inv = theta ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv
    return ang.cos().float(), ang.sin().float()


def rope_positions(T):
    """Packed sequences: ids restart mid-batch; position 0 and the last table row both occur."""
    if T == 1:
        return torch.tensor([ROPE_MAX_POS - 1])
    seq = list(range(12)) + list(range(10)) + [ROPE_MAX_POS - 1, 0, ROPE_MAX_POS - 1] + list(range(12))
    return torch.tensor(seq[:T])


def check_rope(dev, D, T, nh):
    """The rotated heads are a column slice [8, 8 + C) of a wider buffer (row_stride > columns), and
    C holds one more head than is rotated: that head and the buffer outside the slice stay put."""
    C, lo = nh * D + D, 8
    rot = slice(lo, lo + nh * D)
    full = torch.randn(T, lo + C + 16, generator=_gen(D + T + nh)).to(BF)
    cos, sin = rope_tables(D)
    pos = rope_positions(T)
    cd, sd = cos.to(dev), sin.to(dev)

    def untouched(out):
        assert torch.equal(out[:, :lo], full[:, :lo]) and torch.equal(out[:, lo + C:], full[:, lo + C:]), \
            "rope wrote outside its column slice"
        assert torch.equal(out[:, lo + nh * D:lo + C], full[:, lo + nh * D:lo + C]), "rope touched a head past nheads"

    fd = full.to(dev, copy=True)
    view = fd[:, lo:lo + C]
    assert view.stride(0) > view.size(1)
    dops.rope_(view, cd, sd, pos.to(dev), nh, D, False)
    out = _cpu(fd)
    ref, term = R.rope_ref(full[:, lo:lo + C], cos, sin, pos, nh, D, False)
    R.assert_within(out[:, rot], ref[:, :nh * D], term[:, :nh * D], "rope_ forward")
    untouched(out)
    assert torch.equal(out[pos == 0], full[pos == 0]), "position 0 must leave the row as it is"
    dops.rope_(view, cd, sd, pos.to(dev), nh, D, True)
    back = _cpu(fd)
    rt = R.rope_roundtrip_term(full[:, lo:lo + C], cos, sin, pos, nh, D)
    R.assert_within(back[:, rot], R.f64(full[:, rot]), rt[:, :nh * D], "rope_ inverse(forward)")
    untouched(back)
    # every token at position 0, both directions: bitwise the input
    for inverse in (False, True):
        fz = full.to(dev, copy=True)
        dops.rope_(fz[:, lo:lo + C], cd, sd, torch.zeros(T, dtype=torch.int64, device=dev), nh, D, inverse)
        assert torch.equal(_cpu(fz), full), "position 0 must leave the buffer as it is"
    _check_rope_last_row(dev, D)


def _check_rope_last_row(dev, D):
    """Three tokens at positions {0, 1, max_pos - 1}, 3 rotated heads in a buffer of 4 heads whose row
    stride is wider than its columns: pins the (token, head, group) decode at a head count that is not
    the buffer's and the table load at the last row.  Forward then inverse: head 4 and the padding keep
    their bits, the rotated heads return within the round-trip bound."""
    T, nh, lo = 3, 3, 8
    C = 4 * D
    full = torch.randn(T, lo + C + 24, generator=_gen(7 * D)).to(BF)
    cos, sin = rope_tables(D)
    pos = torch.tensor([0, 1, ROPE_MAX_POS - 1])
    fd = full.to(dev, copy=True)
    view = fd[:, lo:lo + C]
    assert view.stride(0) > view.size(1)
    for inverse in (False, True):
        dops.rope_(view, cos.to(dev), sin.to(dev), pos.to(dev), nh, D, inverse)
        out = _cpu(fd)
        keep = torch.ones(full.shape[1], dtype=torch.bool)
        keep[lo:lo + nh * D] = False
        assert torch.equal(out[:, keep], full[:, keep]), "rope wrote to head 4 or to the padding columns"
        if not inverse:
            assert not torch.equal(out[2, ~keep], full[2, ~keep]), "the token on the last table row was not rotated"
    rt = R.rope_roundtrip_term(full[:, lo:lo + C], cos, sin, pos, nh, D)
    R.assert_within(out[:, lo:lo + nh * D], R.f64(full[:, lo:lo + nh * D]), rt[:, :nh * D], "rope_ last row round trip")


def check_rope_empty(dev):
    cos, sin = rope_tables(64)
    x = torch.zeros(0, 128, dtype=BF, device=dev)
    dops.rope_(x, cos.to(dev), sin.to(dev), torch.zeros(0, dtype=torch.int64, device=dev), 2, 64, False)
    assert x.shape == (0, 128)


# ---------------------------------------------------------------------------------- SwiGLU
# the zero of 1 + g (1 - sigma) lies between -1.28125 and -1.25; __expf saturates past +-88
SWIGLU_GATES = [0.0, 2.0 ** -20, -2.0 ** -20, -1.25, -1.28125, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
SWIGLU_VALS = [1.0, -1.0, 3.5, -3.5]


def swiglu_inputs(T, I):
    """gu [T, 2I] and dh [T, I]: the gate grid crossed with up, dh in {+-1, +-3.5} first (as much
    of it as fits), random values after it."""
    n = T * I
    g = _gen(T * 1000 + I)
    idx = torch.arange(n)
    ng, nv = len(SWIGLU_GATES), len(SWIGLU_VALS)
    grid = idx < ng * nv * nv
    gate = torch.where(grid, torch.tensor(SWIGLU_GATES)[idx % ng], 2 * torch.randn(n, generator=g))
    up = torch.where(grid, torch.tensor(SWIGLU_VALS)[(idx // ng) % nv], 2 * torch.randn(n, generator=g))
    dh = torch.where(grid, torch.tensor(SWIGLU_VALS)[(idx // (ng * nv)) % nv], torch.randn(n, generator=g))
    gu = torch.cat([gate.view(T, I), up.view(T, I)], 1).to(BF)
    return gu, dh.view(T, I).to(BF)


def _strided_gu(gu, dev):
    T, C = gu.shape
    buf = torch.full((T, C + 16), 7.0, dtype=BF)
    buf[:, 8:8 + C] = gu
    view = buf.to(dev)[:, 8:8 + C]
    assert view.stride(0) == C + 16
    return view


def check_swiglu(dev, T, I):
    gu, dh = swiglu_inputs(T, I)
    h = dops.swiglu_fwd(gu.to(dev))
    R.assert_within(h, R.swiglu_ref(gu), R.swiglu_term(gu), "swiglu_fwd")
    dgu = dops.swiglu_bwd(dh.to(dev), gu.to(dev))
    R.assert_within(dgu, R.swiglu_bwd_ref(dh, gu), R.swiglu_bwd_term(dh, gu), "swiglu_bwd")
    gs = _strided_gu(gu, dev)
    assert torch.equal(dops.swiglu_fwd(gs), h), "swiglu_fwd: strided gu"
    assert torch.equal(dops.swiglu_bwd(dh.to(dev), gs), dgu), "swiglu_bwd: strided gu"


def check_swiglu_bwd_t(dev, T, I):
    gu, dh = swiglu_inputs(T, I)
    gs = _strided_gu(gu, dev)
    dgu, dgu_t, h_t = dops.swiglu_bwd_t(dh.to(dev), gs)
    assert dgu.shape == (T, 2 * I) and dgu_t.shape == (2 * I, T) and h_t.shape == (I, T)
    # one functor behind the tiled and the untiled kernels: the same bits
    assert torch.equal(dgu, dops.swiglu_bwd(dh.to(dev), gs)), "swiglu_bwd_t: dgu != swiglu_bwd"
    assert torch.equal(h_t.t(), dops.swiglu_fwd(gs)), "swiglu_bwd_t: h_t.t() != swiglu_fwd"
    R.assert_within(dgu, R.swiglu_bwd_ref(dh, gu), R.swiglu_bwd_term(dh, gu), "swiglu_bwd_t dgu")
    assert torch.equal(dgu_t, dgu.t()), "swiglu_bwd_t: dgu_t != dgu.t()"
    R.assert_within(h_t.t(), R.swiglu_ref(gu), R.swiglu_term(gu), "swiglu_bwd_t h_t")


def check_swiglu_bwd_t_refusals(dev):
    """gu widths 24 (I = 12) and 33 (2I + 1, in rows of 40 so that only the width is wrong), and a
    dh of the right size that is not [T, I]."""
    odd = torch.zeros(8, 24, dtype=BF, device=dev)
    plus1 = torch.zeros(8, 40, dtype=BF, device=dev)[:, :33]
    assert plus1.stride(0) % 8 == 0 and plus1.stride(1) == 1
    for gu in (odd, plus1):
        with pytest.raises(RuntimeError, match="swiglu_bwd_t"):
            dops.swiglu_bwd_t(torch.zeros(8, gu.size(1) // 2, dtype=BF, device=dev), gu)
    gu = torch.zeros(8, 32, dtype=BF, device=dev)
    for shape in ((8 * 16,), (8, 16, 1), (16, 8)):
        with pytest.raises(RuntimeError, match="swiglu_bwd_t"):
            dops.swiglu_bwd_t(torch.zeros(shape, dtype=BF, device=dev), gu)


def check_swiglu_empty(dev):
    gu = torch.zeros(0, 32, dtype=BF, device=dev)
    dh = torch.zeros(0, 16, dtype=BF, device=dev)
    assert dops.swiglu_fwd(gu).shape == (0, 16)
    assert dops.swiglu_bwd(dh, gu).shape == (0, 32)
    dgu, dgu_t, h_t = dops.swiglu_bwd_t(dh, gu)
    assert dgu.shape == (0, 32) and dgu_t.shape == (32, 0) and h_t.shape == (16, 0)


# --------------------------------------------------------------------------- cross entropy
CE_ROWS = 9
CE_VOCABS = [1, 3, 7, 8, 9, 511, 512, 513, 4097]
CE_SCALE = 0.25


def ce_rows(V, o, seed=0):
    """[9, V] logits and labels.  Row kinds: 3 * randn (rows 0, 6, 7, 8), all equal (1), one logit
    30 above the rest with the label on it (2) and off it (3), everything shifted by +1e4 (4) and
    -1e4 (5).  Rows 6 and 7 are ignored.  Labels cycle with the row and the slice offset through
    column 0, column V - 1, and columns in the scalar head, the vector body and the tail."""
    g = _gen(seed + 17 * V + o)
    x = 3 * torch.randn(CE_ROWS, V, generator=g)
    x[1] = 1.5
    cols = [0, V - 1, min(3, V - 1), V // 2, max(V - 3, 0)]
    labels = torch.tensor([cols[(r + o) % 5] for r in range(CE_ROWS)])
    x[2, labels[2]] = x[2].max() + 30
    peak = cols[(3 + o + 1) % 5]
    x[3, peak] = x[3].max() + 30
    if peak == labels[3] and V > 1:
        labels[3] = (peak + 1) % V
    x[4] += 1e4
    x[5] -= 1e4
    labels[6] = labels[7] = IGNORE
    return x.to(BF), labels


def check_ce(dev, V):
    """Every slice offset 0..7 out of a [9, V + 16] buffer: every length of the scalar head (head > V
    for the short rows too), and odd V shifts the alignment from row to row as well."""
    for o in range(8):
        x, labels = ce_rows(V, o)
        full = torch.randn(CE_ROWS, V + 16, generator=_gen(o)).to(BF)
        full[:, o:o + V] = x
        fd, ld = full.to(dev, copy=True), labels.to(dev)
        view = fd[:, o:o + V]
        loss0 = dops.ce_fwd_bwd_(view, ld, IGNORE, CE_SCALE, False)
        assert torch.equal(_cpu(fd), full), f"V={V} o={o}: compute_grad=False wrote to the logits"
        loss = dops.ce_fwd_bwd_(view, ld, IGNORE, CE_SCALE, True)
        assert torch.equal(loss, loss0), f"V={V} o={o}: the loss depends on compute_grad"
        out = _cpu(fd)
        loss_r, grad_r, _, _, _ = R.ce_ref(x, labels, IGNORE, CE_SCALE)
        t = R.ce_terms(x, labels, IGNORE, CE_SCALE)
        R.assert_within(loss, loss_r, t["loss"], "ce_fwd_bwd_ loss")
        R.assert_within(out[:, o:o + V], grad_r, t["grad"], "ce_fwd_bwd_ grad")
        ign = labels == IGNORE
        assert torch.count_nonzero(out[:, o:o + V][ign]) == 0 and torch.count_nonzero(_cpu(loss)[ign]) == 0
        assert torch.equal(out[:, :o], full[:, :o]) and torch.equal(out[:, o + V:], full[:, o + V:]), \
            f"V={V} o={o}: pad columns written"


def check_ce_vocab_parallel(dev):
    """Two shards split at an odd column; labels in this shard, in the other one, and ignored."""
    V, cut = 1001, 333
    x, labels = ce_rows(V, 0)
    labels[0], labels[8] = cut - 1, cut  # the last column of shard 0 and the first of shard 1
    shards = [(x[:, :cut].contiguous().to(dev), 0), (x[:, cut:].contiguous().to(dev), cut)]
    ld = labels.to(dev)
    stats = []
    for sh, start in shards:
        m, s, xl = dops.ce_stats(sh, ld, start)
        m_r, s_r, xl_r, s_t = R.ce_stats_ref(sh, labels, start)
        assert torch.equal(_cpu(m).double(), m_r) and torch.equal(_cpu(xl).double(), xl_r), "ce_stats m / xl"
        R.assert_within(s, s_r, s_t, "ce_stats s")
        stats.append((R.f64(m), R.f64(s), R.f64(xl)))
    (m0, s0, x0), (m1, s1, x1) = stats
    mm = torch.maximum(m0, m1)
    lse = mm + torch.log(s0 * torch.exp(m0 - mm) + s1 * torch.exp(m1 - mm))
    valid = labels != IGNORE
    loss = torch.where(valid, lse - (x0 + x1), torch.zeros_like(lse))
    loss_r, grad_r, _, _, lse_r = R.ce_ref(x, labels, IGNORE, CE_SCALE)
    t = R.ce_terms(x, labels, IGNORE, CE_SCALE)
    R.assert_within(loss.float(), loss_r, t["loss"], "ce_stats combined loss")
    for sh, start in shards:
        dops.ce_grad_(sh, ld, lse.float().to(dev), start, IGNORE, CE_SCALE)
    grad = torch.cat([_cpu(shards[0][0]), _cpu(shards[1][0])], 1)
    R.assert_within(grad, grad_r, t["grad"], "ce_grad_ grad")
    assert torch.count_nonzero(grad[~valid]) == 0


def check_ce_empty(dev):
    x = torch.zeros(0, 40, dtype=BF, device=dev)
    lab = torch.zeros(0, dtype=torch.int64, device=dev)
    loss = dops.ce_fwd_bwd_(x, lab, IGNORE, 1.0, True)
    assert loss.shape == (0,) and loss.dtype == torch.float32
    m, s, xl = dops.ce_stats(x, lab, 0)
    assert m.shape == s.shape == xl.shape == (0,)
    dops.ce_grad_(x, lab, loss, 0, IGNORE, 1.0)


# ----------------------------------------------------------------------------------- AdamW
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
ADAM_COMBOS = [(gd, sd, ms) for gd in (BF, torch.float32) for sd in (BF, torch.float32) for ms in (False, True)]
ADAM_IDS = [f"grad_{'bf16' if gd == BF else 'f32'}-state_{'bf16' if sd == BF else 'f32'}-{'master' if ms else 'nomaster'}"
            for gd, sd, ms in ADAM_COMBOS]
ADAM_LAYOUTS = {"vector": 1000, "scalar": 1001, "misaligned": 1000}
ADAM_BIG_N = 2 * 8388608 + 3 * 2048 + 8  # the unrolled loop, the remainder loop and idle lanes


def adam_inputs(n, gdt, sdt, seed=0):
    g = _gen(seed)
    master = torch.randn(n, generator=g)
    grad = (0.1 * torch.randn(n, generator=g)).to(gdt)
    m = (0.05 * torch.randn(n, generator=g)).to(sdt)
    v = (0.01 * torch.rand(n, generator=g)).to(sdt)
    return master, grad, m, v


def _place(t, dev, misaligned):
    """On the device; `misaligned` puts it one element into a larger buffer (off 16 bytes)."""
    if not misaligned:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 or dev.type == "cpu"
    return view


def check_adamw_steps(dev, master0, grad, m0, v0, use_master, steps, misaligned=False, grad_scale=0.5, tag="adamw_",
                      **hyper):
    """Each step is compared with adamw_ref started from the state the op itself stored before it,
    so every comparison is one step with one rounding on store, at that step's bias correction."""
    hp = dict(ADAM, **hyper)
    p = _place(master0.to(BF), dev, misaligned)
    master = _place(master0.clone(), dev, misaligned) if use_master else None
    g, m, v = (_place(t, dev, misaligned) for t in (grad, m0.clone(), v0.clone()))
    sname = "bf16" if m0.dtype == BF else "f32"
    for step in steps:
        before = [_cpu(master if use_master else p).clone(), _cpu(m).clone(), _cpu(v).clone()]
        dops.adamw_(p, master, g, m, v, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], step, grad_scale)
        p_r, m_r, v_r, t = R.adamw_ref(before[0], grad, before[1], before[2], hp["lr"], hp["beta1"], hp["beta2"],
                                       hp["eps"], hp["wd"], step, grad_scale)
        R.assert_within(m, m_r, t["m"], f"{tag} exp_avg ({sname})")
        R.assert_within(v, v_r, t["v"], f"{tag} exp_avg_sq ({sname})")
        if use_master:
            R.assert_within(master, p_r, t["p"], f"{tag} master (f32)")
            assert torch.equal(p, master.to(BF)), "p is not the bf16 rounding of the master"
        R.assert_within(p, p_r, t["p"], f"{tag} p (bf16)")


def check_adamw_combo(dev, gdt, sdt, use_master, layout):
    n = ADAM_LAYOUTS[layout]
    master, grad, m, v = adam_inputs(n, gdt, sdt, seed=n)
    check_adamw_steps(dev, master, grad, m, v, use_master, (1, 2, 3), misaligned=layout == "misaligned")


ADAM_EDGE_CASES = [dict(wd=0.0, step=1, grad_scale=1.0), dict(wd=0.01, step=100000, grad_scale=1.0),
                   dict(wd=0.01, step=3, grad_scale=0.0)]


def check_adamw_edges(dev, sdt, use_master, wd, step, grad_scale):
    """One vector holding g = 0 with v = 0 (m = 0 and m != 0: the denominator is eps alone) and v at
    the smallest normal (with and without a gradient), run with wd = 0, step = 100000 and
    grad_scale = 0."""
    master, grad, m, v = adam_inputs(16, BF, sdt, seed=5)
    grad[:2] = 0
    v[:2] = 0
    m[0] = 0
    v[2:4] = R.TINY
    grad[3] = 0
    check_adamw_steps(dev, master, grad, m, v, use_master, (step,), grad_scale=grad_scale, tag="adamw_ edges", wd=wd)


def check_adamw_big(dev):
    master, grad, m, v = adam_inputs(ADAM_BIG_N, BF, BF, seed=9)
    check_adamw_steps(dev, master, grad, m, v, False, (1,), tag="adamw_ 16.8M")
