"""Cases, float64 references and f32 error terms of the per-head QK RMSNorm + RoPE operators
(csrc/kernels/qk_norm.hip, dtg.ops._cpu), shared by test_qk_norm_cpu.py and test_qk_norm_gpu.py.

Reference: the f64 norm  y = w x rsqrt(mean(x^2) + eps)  then the f64 rotation of the bf16 inputs, one
rounding.  Bounds follow tests/_refs.py: half a bf16 ulp for the single store plus an f32 term of
U = 2^-24 per operation on the magnitudes combined, times the reduction length, times K = 8.  The
derivations sit beside each reference below; nothing comes from a run of the code under test.
"""
import functools

import torch

import dtg.ops  # noqa: F401  (defines torch.ops.dtg)
from _refs import K, U, assert_within, f64

EPS = 1e-6
MAX_POS = 40960

DIMS = (64, 128)
HEADS = ((1, 1), (3, 1), (4, 2), (32, 8))
TOKENS = (1, 3, 65, 1031)
# every shape in the plain form; the strided and the norm-only forms where rows, heads per wave and dw
# partial blocks are all ragged
CASES = [(D, nq, nkv, T, "plain") for D in DIMS for nq, nkv in HEADS for T in TOKENS]
CASES += [(D, nq, nkv, T, v) for D in DIMS for nq, nkv, T in ((3, 1, 65), (4, 2, 1031)) for v in ("strided", "norm_only")]


def case_id(c):
    return f"D{c[0]}-h{c[1]}x{c[2]}-T{c[3]}-{c[4]}"


@functools.lru_cache(maxsize=None)
def tables(D):
    """f32 cos / sin [MAX_POS, D/2] (rope_theta 1e6, as the bundled Qwen3 configs)."""
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    return fr.cos().float().contiguous(), fr.sin().float().contiguous()


def positions(T):
    """Packed rows: position ids restart mid-batch; the last token sits on the table's last row."""
    if T == 0:
        return torch.zeros(0, dtype=torch.long)
    cut = max(1, (2 * T) // 5)
    pos = torch.cat([torch.arange(cut), torch.arange(T - cut)]).long()
    pos[-1] = MAX_POS - 1
    return pos


@functools.lru_cache(maxsize=2)
def make_case(D, nq, nkv, T, variant):
    """Inputs (CPU, bf16) and every reference of one case; computed once, shared, never modified."""
    g = torch.Generator().manual_seed(1000 * D + 100 * nq + 10 * nkv + T)
    nh, C = nq + nkv, (nq + 2 * nkv) * D
    pad = 24 if variant == "strided" else 0  # a column slice of a wider buffer: row stride > width
    buf = (2.0 * torch.randn(T, C + pad, generator=g)).to(torch.bfloat16)
    dbuf = torch.randn(T, C + pad, generator=g).to(torch.bfloat16)
    qkv, dqkv = buf[:, 8:8 + C] if pad else buf, dbuf[:, 8:8 + C] if pad else dbuf
    if T:
        qkv[0, :D] = 0                                       # an all-zero head: eps-dominated
        qkv[-1, (nh - 1) * D: nh * D] *= 1e-3 / 2.0          # a head of magnitude 1e-3
    wq = (1.0 + 0.5 * torch.randn(D, generator=g)).to(torch.bfloat16)
    wk = (1.0 + 0.5 * torch.randn(D, generator=g)).to(torch.bfloat16)
    wq[3] = 0.0                                              # exact zeros: x is not y / w
    wk[D // 2 + 1] = 0.0
    rope = variant != "norm_only"
    pos = positions(T)
    cos, sin = tables(D) if rope else (torch.empty(0), torch.empty(0))
    c = dict(D=D, nq=nq, nkv=nkv, T=T, nh=nh, C=C, qkv=qkv, dqkv=dqkv, wq=wq, wk=wk, cos=cos, sin=sin,
             pos=pos if rope else torch.empty(0, dtype=torch.long), rope=rope)
    c.update(_reference(c))
    return c


def _reference(c):
    D, nq, nh, T = c["D"], c["nq"], c["nh"], c["T"]
    half = D // 2
    x = f64(c["qkv"])[:, : nh * D].reshape(T, nh, D)
    w = torch.cat([f64(c["wq"])[None].expand(nq, D), f64(c["wk"])[None].expand(nh - nq, D)], 0)
    if c["rope"]:
        cs, sn = f64(c["cos"])[c["pos"]][:, None, :], f64(c["sin"])[c["pos"]][:, None, :]
    else:
        cs, sn = torch.ones(T, 1, half, dtype=torch.float64), torch.zeros(T, 1, half, dtype=torch.float64)
    rstd = torch.rsqrt((x * x).mean(-1) + EPS)
    # rstd: U per square and D U for the D-term sum, relative to the sum; the mean, the + eps and the
    # rsqrt add 3 U; rstd moves by half the relative error of its argument (as rmsnorm_terms)
    rel_r = D / 2 + 4
    y = w * x * rstd[..., None]
    y1, y2 = y[..., :half], y[..., half:]
    out = torch.cat([y1 * cs - y2 * sn, y2 * cs + y1 * sn], -1)
    # y = w (x rstd): rstd's error and two products; the rotation: two products and an add on the
    # magnitudes it combines (as rope_ref).  Without the rotation cs = 1, sn = 0 and the same holds.
    mag = torch.cat([(y1 * cs).abs() + (y2 * sn).abs(), (y2 * cs).abs() + (y1 * sn).abs()], -1)
    y_term = K * U * (rel_r + 4) * mag

    # backward: dy = R(-theta) g,  xh = x rstd,  dx = rstd (w dy - xh mean(w dy xh)),  dw = sum dy xh
    gr = f64(c["dqkv"])[:, : nh * D].reshape(T, nh, D)
    g1, g2 = gr[..., :half], gr[..., half:]
    dy = torch.cat([g1 * cs + g2 * sn, g2 * cs - g1 * sn], -1)
    # in units of U: two products and an add on the rotated magnitudes
    e_dy = 2 * torch.cat([(g1 * cs).abs() + (g2 * sn).abs(), (g2 * cs).abs() + (g1 * sn).abs()], -1)
    r = rstd[..., None]
    xh = x * r
    rel_xh = rel_r + 1                                       # the stored f32 rstd and one product
    wdy = w * dy
    e_wdy = w.abs() * e_dy + wdy.abs()
    dot = (wdy * xh).mean(-1, keepdim=True)
    # D products and a D-term reduction of |w dy xh|, the / D, and the errors its factors carry
    e_dot = (D + 2) * (wdy * xh).abs().mean(-1, keepdim=True) + \
        (e_wdy * xh.abs() + (wdy * xh).abs() * rel_xh).mean(-1, keepdim=True)
    dx = r * (wdy - xh * dot)
    # xh dot: both factors' errors and the product; the subtraction on |w dy| + |xh dot|; the final
    # product carries rstd's error and its own roundoff
    e_dx = r * (e_wdy + xh.abs() * e_dot + (xh * dot).abs() * (rel_xh + 1) + wdy.abs() + (xh * dot).abs()) + \
        dx.abs() * (rel_r + 1)
    dx_term = K * U * e_dx
    s = dy * xh
    e_s = e_dy * xh.abs() + s.abs() * (rel_xh + 1)

    def dw_of(h0, h1):
        n = T * (h1 - h0)                                    # reduction length: T x heads
        return s[:, h0:h1].sum((0, 1)), K * U * (e_s[:, h0:h1].sum((0, 1)) + n * s[:, h0:h1].abs().sum((0, 1)))

    dwq, dwq_term = dw_of(0, nq)
    dwk, dwk_term = dw_of(nq, nh)
    return dict(ref_y=out.reshape(T, nh * D), y_term=y_term.reshape(T, nh * D), ref_rstd=rstd,
                rstd_term=K * U * rel_r * rstd, ref_dx=dx.reshape(T, nh * D), dx_term=dx_term.reshape(T, nh * D),
                ref_dwq=dwq, dwq_term=dwq_term, ref_dwk=dwk, dwk_term=dwk_term)


def _place(t, dev):
    """A copy of `t` on `dev` with the same strides (the strided form keeps its wider buffer)."""
    base = t._base if t._base is not None else t
    b = base.clone().to(dev)
    return b.as_strided(t.shape, t.stride(), t.storage_offset())


def check_ops(c, dev):
    """Forward and backward operators on `dev` against the references of case `c`."""
    ops = torch.ops.dtg
    D, nq, nkv, nh, T = c["D"], c["nq"], c["nkv"], c["nh"], c["T"]
    name = case_id((D, nq, nkv, T, "rope" if c["rope"] else "norm_only"))
    wq, wk, cos, sin, pos = (c[k].to(dev) for k in ("wq", "wk", "cos", "sin", "pos"))
    qkv = _place(c["qkv"], dev)
    xqk, rstd = ops.qk_norm_rope_fwd_(qkv, wq, wk, cos, sin, pos, nq, nkv, D, EPS)
    assert xqk.shape == (T, nh * D) and xqk.is_contiguous() and rstd.shape == (T, nh)
    assert torch.equal(xqk.cpu().view(torch.int16), c["qkv"][:, : nh * D].contiguous().view(torch.int16)), "xqk bits"
    assert torch.equal(qkv[:, nh * D:].cpu().view(torch.int16), c["qkv"][:, nh * D:].contiguous().view(torch.int16)), "v"
    assert_within(qkv[:, : nh * D], c["ref_y"], c["y_term"], f"qk_norm y {name}")
    assert_within(rstd, c["ref_rstd"], c["rstd_term"], f"qk_norm rstd {name}")
    if c["qkv"]._base is not None:  # nothing outside the slice was written
        full, orig = qkv._base.cpu(), c["qkv"]._base
        assert torch.equal(full[:, :8].view(torch.int16), orig[:, :8].view(torch.int16))
        assert torch.equal(full[:, 8 + c["C"]:].view(torch.int16), orig[:, 8 + c["C"]:].view(torch.int16))

    # the backward takes the f64-exact rstd's f32 rounding, so its check does not hang on the forward
    rstd_in = c["ref_rstd"].float().to(dev)
    xqk_in = c["qkv"][:, : nh * D].contiguous().to(dev)
    runs = []
    for _ in range(2):
        dqkv = _place(c["dqkv"], dev)
        dwq, dwk = ops.qk_norm_rope_bwd_(dqkv, xqk_in, rstd_in, wq, wk, cos, sin, pos, nq, nkv, D)
        runs.append((dqkv, dwq, dwk))
    dqkv, dwq, dwk = runs[0]
    assert dwq.dtype == wq.dtype and dwq.shape == (D,) and dwk.shape == (D,)
    assert torch.equal(dqkv[:, nh * D:].cpu().view(torch.int16), c["dqkv"][:, nh * D:].contiguous().view(torch.int16)), "dv"
    assert_within(dqkv[:, : nh * D], c["ref_dx"], c["dx_term"], f"qk_norm dx {name}")
    assert_within(dwq, c["ref_dwq"], c["dwq_term"], f"qk_norm dwq {name}")
    assert_within(dwk, c["ref_dwk"], c["dwk_term"], f"qk_norm dwk {name}")
    for a, b in zip(runs[0], runs[1]):  # bitwise reproducible
        assert torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16))


def check_public_op(c, dev, fused, monkeypatch):
    """ops.qk_norm_rope (fused kernel or the composed DTG_QKNORM_FUSED=0 path) with autograd, held to
    the same references and bounds: the two paths agree within them."""
    from dtg import ops
    from dtg.ops import functional

    monkeypatch.setattr(functional, "_QKNORM_FUSED", fused)
    D, nq, nkv, nh, T = c["D"], c["nq"], c["nkv"], c["nh"], c["T"]
    name = case_id((D, nq, nkv, T, "fused" if fused else "composed"))
    wq, wk = (c[k].clone().to(dev).requires_grad_() for k in ("wq", "wk"))  # clones: the case stays as it is
    cos, sin, pos = (c[k].to(dev) for k in ("cos", "sin", "pos"))
    x = c["qkv"].clone().to(dev).requires_grad_()
    y = ops.qk_norm_rope(x, wq, wk, EPS, nq, nkv, D, *((cos, sin, pos) if c["rope"] else ()))
    assert torch.equal(x.detach().cpu().view(torch.int16), c["qkv"].contiguous().view(torch.int16)), "leaf input kept"
    dy = c["dqkv"].contiguous().to(dev)
    y.backward(dy.clone())
    assert torch.equal(y[:, nh * D:].detach().cpu().view(torch.int16), c["qkv"][:, nh * D:].contiguous().view(torch.int16))
    assert_within(y[:, : nh * D].detach(), c["ref_y"], c["y_term"], f"qk_norm_rope y {name}")
    # the forward's own f32 rstd (not the reference's) enters dx: its error is part of dx_term already
    assert_within(x.grad[:, : nh * D], c["ref_dx"], c["dx_term"], f"qk_norm_rope dx {name}")
    assert torch.equal(x.grad[:, nh * D:].cpu().view(torch.int16), c["dqkv"][:, nh * D:].contiguous().view(torch.int16))
    assert_within(wq.grad, c["ref_dwq"], c["dwq_term"], f"qk_norm_rope dwq {name}")
    assert_within(wk.grad, c["ref_dwk"], c["dwk_term"], f"qk_norm_rope dwk {name}")
