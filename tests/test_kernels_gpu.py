"""T6: every gfx950 HIP kernel against the f32 PyTorch reference of the same op (CPU impl).

Inputs are generated once on the CPU, the kernel runs on cuda:0, the reference on the CPU, and
outputs are compared in f32 with bf16-appropriate tolerances.
"""
import math

import pytest
import torch

import dtg  # noqa: F401
from dtg import ops
from dtg.ops import _native

pytestmark = pytest.mark.gpu
dops = torch.ops.dtg


def _close(a, b, atol, rtol=0.0, name=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{name}: {bad} elems off, max err {err.max().item():.4g}"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_native_loaded(cuda):
    assert _native.LOADED, "gfx950 extension must be loaded on a GPU box"


@pytest.mark.parametrize("T,H", [(257, 4096), (64, 3072), (4096, 3072), (1024, 896), (33, 128), (8, 16384)])
def test_rmsnorm(cuda, T, H):
    torch.manual_seed(0)
    x = torch.randn(T, H).bfloat16()
    r = torch.randn(T, H).bfloat16()
    w = (1 + 0.1 * torch.randn(H)).bfloat16()
    dy = torch.randn(T, H).bfloat16()
    dres = torch.randn(T, H).bfloat16()
    y_ref, rstd_ref = dops.rmsnorm_fwd(x, w, 1e-5)
    y, rstd = dops.rmsnorm_fwd(x.to(cuda), w.to(cuda), 1e-5)
    _close(y, y_ref, 2e-2, 1e-2, "rmsnorm y")
    _close(rstd, rstd_ref, 1e-4, 1e-4, "rstd")
    y2_ref, h_ref, _ = dops.add_rmsnorm_fwd(x, r, w, 1e-5)
    y2, h, rstd2 = dops.add_rmsnorm_fwd(x.to(cuda), r.to(cuda), w.to(cuda), 1e-5)
    _close(h, h_ref, 0, 0, "residual sum")
    _close(y2, y2_ref, 2e-2, 1e-2, "add_rmsnorm y")
    dx_ref, dw_ref = dops.rmsnorm_bwd(dy, x, w, rstd_ref, dres)
    dx, dw = dops.rmsnorm_bwd(dy.to(cuda), x.to(cuda), w.to(cuda), rstd, dres.to(cuda))
    _close(dx, dx_ref, 3e-2, 2e-2, "dx")
    assert _rel(dw, dw_ref) < 1e-2


@pytest.mark.parametrize("D,nh", [(128, 40), (64, 6)])
def test_rope(cuda, D, nh):
    torch.manual_seed(0)
    T = 300
    cols = nh * D + 2 * D  # an extra (v-like) head region the kernel must not touch
    qkv = torch.randn(T, cols).bfloat16()
    cos, sin = ops.rope_tables(D, 500000.0, 4096, {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                    "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    pos = torch.randint(0, 4096, (T,))
    ref = qkv.clone()
    dops.rope_(ref, cos, sin, pos, nh, D, False)
    g = qkv.to(cuda)
    dops.rope_(g, cos.to(cuda), sin.to(cuda), pos.to(cuda), nh, D, False)
    _close(g[:, : nh * D], ref[:, : nh * D], 2e-2, 1e-2, "rope")
    assert torch.equal(g[:, nh * D:].cpu(), qkv[:, nh * D:]), "rope touched the pass-through columns"
    dops.rope_(g, cos.to(cuda), sin.to(cuda), pos.to(cuda), nh, D, True)
    _close(g[:, : nh * D], qkv[:, : nh * D], 3e-2, 2e-2, "rope inverse")
    assert torch.equal(g[:, nh * D:].cpu(), qkv[:, nh * D:]), "rope inverse touched the pass-through columns"


def test_swiglu(cuda):
    torch.manual_seed(0)
    T, I = 77, 1792
    gu = (2 * torch.randn(T, 2 * I)).bfloat16()
    dh = torch.randn(T, I).bfloat16()
    _close(dops.swiglu_fwd(gu.to(cuda)), dops.swiglu_fwd(gu), 2e-2, 1e-2, "swiglu")
    _close(dops.swiglu_bwd(dh.to(cuda), gu.to(cuda)), dops.swiglu_bwd(dh, gu), 3e-2, 2e-2, "swiglu bwd")


@pytest.mark.parametrize("R,C,ld", [(64, 64, 64), (4096, 6144, 6144), (1000, 520, 528), (8, 8, 8), (136, 7000, 7000)])
def test_transpose2d(cuda, R, C, ld):
    x = torch.randn(R, ld).bfloat16()[:, :C]
    y = dops.transpose2d(x.to(cuda))
    assert y.shape == (C, R) and y.is_contiguous()
    assert torch.equal(y.cpu(), x.t().contiguous())


def test_transpose_mats_batched(cuda):
    """One launch transposing several matrices of a flat buffer (ZeRO's per-bucket W^T rebuild)
    == per-matrix transposes, ragged edge tiles included; a descriptor out of range is refused
    on the host before any launch."""
    torch.manual_seed(0)
    shapes = [(64, 128), (520, 136), (8, 4096), (4096, 8)]
    n = sum(r * c for r, c in shapes)
    x = torch.randn(n).bfloat16()
    desc, so, do, t0 = [], 0, 0, 0
    for r, c in shapes:
        desc.append([so, r, c, n - do - r * c, t0])  # destinations in reverse order
        so += r * c
        do += r * c
        t0 += -(-r // 64) * -(-c // 64)
    h = torch.tensor(desc, dtype=torch.long)
    out = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    torch.ops.dtg.transpose_mats_(x.to(cuda), out, h.to(cuda), h, t0)
    ref = torch.zeros(n, dtype=torch.bfloat16)
    torch.ops.dtg.transpose_mats_(x, ref, h, h, t0)
    assert torch.equal(out.cpu(), ref)
    bad = h.clone()
    bad[1, 3] = n  # destination past the end
    with pytest.raises(RuntimeError, match="out of range"):
        torch.ops.dtg.transpose_mats_(x.to(cuda), out, bad.to(cuda), bad, t0)


@pytest.mark.parametrize("T,I", [(64, 64), (4096, 1792), (520, 136), (8, 8)])
def test_swiglu_bwd_t(cuda, T, I):
    torch.manual_seed(0)
    gu = (2 * torch.randn(T, 2 * I)).bfloat16()
    dh = torch.randn(T, I).bfloat16()
    dgu, dgu_t, h_t = dops.swiglu_bwd_t(dh.to(cuda), gu.to(cuda))
    ref = dops.swiglu_bwd(dh, gu)
    _close(dgu, ref, 3e-2, 2e-2, "dgu")
    _close(dgu_t, ref.t(), 3e-2, 2e-2, "dgu^T")
    _close(h_t, dops.swiglu_fwd(gu).t(), 2e-2, 1e-2, "h^T")
    assert torch.equal(dgu_t.cpu(), dgu.cpu().t())


@pytest.mark.parametrize("mode", ["native", "tn"])
def test_swiglu_mlp_bwd(cuda, mode, monkeypatch):
    """Fused MLP node (TN path with the transposing SwiGLU backward) vs an f32 autograd reference."""
    from dtg.ops import functional as F_

    monkeypatch.setattr(F_, "_LINEAR_BWD", mode)
    torch.manual_seed(0)
    T, H, I = 4096, 256, 704
    x = torch.randn(T, H).bfloat16()
    wgu = (0.06 * torch.randn(2 * I, H)).bfloat16()
    wd = (0.04 * torch.randn(H, I)).bfloat16()
    dy = torch.randn(T, H).bfloat16()
    xs = [t.to(cuda).requires_grad_() for t in (x, wgu, wd)]
    y = F_.swiglu_mlp(*xs)
    y.backward(dy.to(cuda))
    rs = [t.float().requires_grad_() for t in (x, wgu, wd)]
    gu = rs[0] @ rs[1].t()
    g, u = gu.chunk(2, 1)
    yr = (torch.nn.functional.silu(g) * u) @ rs[2].t()
    yr.backward(dy.float())
    assert _rel(y, yr) < 1e-2
    for a, b in zip(xs, rs):
        assert _rel(a.grad, b.grad) < 2e-2


@pytest.mark.parametrize("mode", ["native", "tn", "auto"])
def test_linear_bwd_layouts(cuda, mode, monkeypatch):
    """The transposed-operand (TN) backward GEMMs give the same dX / dW as the strided forms."""
    from dtg.ops import functional as F_

    monkeypatch.setattr(F_, "_LINEAR_BWD", mode)
    torch.manual_seed(0)
    T, n_in, n_out = 4096, 512, 1536
    x = torch.randn(T, n_in).bfloat16()
    w = (0.05 * torch.randn(n_out, n_in)).bfloat16()
    dy = torch.randn(T, n_out).bfloat16()
    xg = x.to(cuda).requires_grad_()
    wg = w.to(cuda).requires_grad_()
    F_.linear(xg, wg).backward(dy.to(cuda))
    dx_ref = dy.float() @ w.float()
    dw_ref = dy.float().t() @ x.float()
    assert _rel(xg.grad, dx_ref) < 1e-2
    assert _rel(wg.grad, dw_ref) < 1e-2


@pytest.mark.parametrize("V", [50257, 1000, 128256, 156939])
def test_cross_entropy(cuda, V):
    torch.manual_seed(0)
    t = 37
    full = (3 * torch.randn(t, V + 3)).bfloat16()
    logits = full[:, 1:V + 1]  # misaligned rows exercise the scalar head/tail
    labels = torch.randint(0, V, (t,))
    labels[3] = -100
    labels[10] = -100
    ref = logits.clone()
    loss_ref = dops.ce_fwd_bwd_(ref, labels, -100, 0.25, True)
    gl = logits.to(cuda)
    loss = dops.ce_fwd_bwd_(gl, labels.to(cuda), -100, 0.25, True)
    _close(loss, loss_ref, 2e-3, 1e-3, "ce loss")
    _close(gl, ref, 2e-4, 2e-2, "ce grad")
    # vocab-parallel pieces: two shards combined on the host equal the fused result
    half = V // 2
    lg = logits.to(cuda)
    m0, s0, x0 = dops.ce_stats(lg[:, :half], labels.to(cuda), 0)
    m1, s1, x1 = dops.ce_stats(lg[:, half:], labels.to(cuda), half)
    gm = torch.maximum(m0, m1)
    lse = gm + torch.log(s0 * torch.exp(m0 - gm) + s1 * torch.exp(m1 - gm))
    valid = labels.to(cuda) != -100
    loss_vp = torch.where(valid, lse - (x0 + x1), torch.zeros_like(lse))
    _close(loss_vp, loss_ref, 2e-3, 1e-3, "vocab-parallel loss")
    a, b = lg[:, :half].clone(), lg[:, half:].clone()
    dops.ce_grad_(a, labels.to(cuda), lse.contiguous(), 0, -100, 0.25)
    dops.ce_grad_(b, labels.to(cuda), lse.contiguous(), half, -100, 0.25)
    _close(torch.cat([a, b], 1), ref, 2e-4, 2e-2, "vocab-parallel grad")


@pytest.mark.parametrize("state_dtype,master", [(torch.bfloat16, False), (torch.float32, False), (torch.float32, True)])
@pytest.mark.parametrize("n", [1 << 20, 1001])
def test_adamw(cuda, state_dtype, master, n):
    torch.manual_seed(0)
    p = torch.randn(n).bfloat16()
    g = torch.randn(n).bfloat16()
    m = (0.1 * torch.randn(n)).to(state_dtype)
    v = (0.01 * torch.rand(n)).to(state_dtype)
    mw = p.float() if master else None
    P = [t.clone() if t is not None else None for t in (p, g, m, v, mw)]
    G = [t.to(cuda) if t is not None else None for t in (p, g, m, v, mw)]
    for step in (1, 2, 3):
        dops.adamw_(P[0], P[4], P[1], P[2], P[3], 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.5)
        dops.adamw_(G[0], G[4], G[1], G[2], G[3], 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.5)
    _close(G[0], P[0], 1e-2, 1e-2, "param")
    _close(G[2], P[2], 1e-3, 1e-2, "exp_avg")
    _close(G[3], P[3], 1e-5, 1e-2, "exp_avg_sq")
    # match torch's own fused AdamW (the reference's optimizer) on bf16 params/states
    if state_dtype == torch.bfloat16 and not master:
        tp = torch.nn.Parameter(p.clone().to(cuda))
        opt = torch.optim.AdamW([tp], lr=1e-3, fused=True)
        pm = p.clone().to(cuda)
        mm = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
        vv = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
        for step in (1, 2, 3):
            tp.grad = g.to(cuda)
            opt.step()
            dops.adamw_(pm, None, g.to(cuda), mm, vv, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0)
        assert (tp.detach().float() - pm.float()).abs().max().item() <= 2 * 2**-7 * tp.detach().float().abs().max().item()


@pytest.mark.parametrize("tile_cols", [64, 128, 256])
@pytest.mark.parametrize("state_dtype,master", [(torch.bfloat16, False), (torch.float32, True)])
def test_adamw_t_matches_adamw_and_transposes(cuda, state_dtype, master, tile_cols):
    """adamw_t_ (update + W^T of every listed matrix in register-blocked 8 x 8 blocks; edge
    tiles, [1, n] rows and a 13-row matrix without a copy) == adamw_ on the same elements,
    bitwise; copies == W^T exactly; elements outside the listed matrices untouched."""
    torch.manual_seed(0)
    shapes = [(192, 320), (1, 136), (72, 200), (1024, 64), (13, 128)]  # 72 x 200: partial edge tiles
    offs, o = [], 0
    for r, c in shapes:
        offs.append(o)
        o += (r * c + 15) // 16 * 16 + 16  # 16 gap elements that must stay untouched
    n = o
    p = torch.randn(n, device=cuda).bfloat16()
    g = torch.randn(n, device=cuda).bfloat16()
    m = (0.1 * torch.randn(n, device=cuda)).to(state_dtype)
    v = (0.01 * torch.rand(n, device=cuda)).to(state_dtype)
    mw = p.float() if master else None
    ref = [t.clone() if t is not None else None for t in (p, g, m, v, mw)]
    desc, toff, tile0 = [], 0, 0
    for (r, c), off in zip(shapes, offs):
        t = toff if r > 1 and r % 8 == 0 else -1  # W^T copies only for whole 8-row blocks
        desc.append([off, r, c, t, tile0])
        tile0 += -(-r // 64) * -(-c // tile_cols)
        if t >= 0:
            toff += r * c
    pt = torch.zeros(toff, dtype=torch.bfloat16, device=cuda)
    mats = torch.tensor(desc, dtype=torch.long, device=cuda)
    for step in (1, 2):
        dops.adamw_t_(p, mw, g, m, v, pt, mats, tile0, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.5, None, tile_cols)
        for (r, c), off in zip(shapes, offs):
            sl = slice(off, off + r * c)
            dops.adamw_(ref[0][sl], None if ref[4] is None else ref[4][sl], ref[1][sl], ref[2][sl], ref[3][sl],
                        1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.5)
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[2]) and torch.equal(v, ref[3])
    for (r, c), off, d in zip(shapes, offs, desc):
        if d[3] >= 0:
            assert torch.equal(pt[d[3]:d[3] + r * c].view(c, r), p[off:off + r * c].view(r, c).t())


@pytest.mark.parametrize("engine_mode", ["single"])
def test_engine_weight_t_bitwise_and_fewer_transposes(cuda, engine_mode, monkeypatch):
    """Llama on the GPU with the TN backward (T = 4096 tokens): persistent W^T written by the
    optimizer gives bitwise the same training as per-backward weight transposes, with 4 fewer
    transpose launches per layer (+1 for the tied/untied loss-head weight)."""
    import dtg.ops.functional as F_
    from dtg.models import build_model, resolve_config
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    cfg = resolve_config("llama-tiny-d128")
    g = torch.Generator().manual_seed(0)
    batches = [torch.randint(0, cfg.vocab_size, (4, 1024), generator=g).to(cuda) for _ in range(3)]
    res = {}
    for wt in (False, True, "again"):  # "again": plain once more, the run-to-run control
        torch.manual_seed(0)
        m = build_model(cfg, device=cuda)
        eng = DataParallel(m, mode=engine_mode, weight_t=wt is True)
        opt = FlatAdamW(eng, lr=1e-3)
        calls = [0]
        real = torch.ops.dtg.transpose2d

        class _Ops:
            def __getattr__(self, k):
                return getattr(torch.ops.dtg, k)

            @staticmethod
            def transpose2d(x):
                calls[0] += 1
                return real(x)

        monkeypatch.setattr(F_, "ops", _Ops())
        for ids in batches:
            opt.zero_grad()
            out = m(input_ids=ids, labels=ids)
            eng.backward(out.loss)
            opt.step()
        monkeypatch.undo()
        torch.cuda.synchronize()
        res[wt] = ({n: p.detach().clone() for n, p in m.named_parameters()}, calls[0])
    deterministic = all(torch.equal(res["again"][0][n], v) for n, v in res[False][0].items())
    for n, v in res[False][0].items():
        if deterministic:
            assert torch.equal(res[True][0][n], v), n
        else:  # the GEMM library is not bitwise reproducible run to run: stay within that spread
            spread = (res["again"][0][n].float() - v.float()).abs().max().item()
            assert (res[True][0][n].float() - v.float()).abs().max().item() <= max(2 * spread, 1e-6), n
    per_step = (res[False][1] - res[True][1]) / len(batches)
    assert per_step == 4 * cfg.num_hidden_layers + 1, (res[False][1], res[True][1])


def _attn_case(cuda, seqlens, hq, hkv, D, causal, stride_extra=0, qscale=1.0, window=0):
    torch.manual_seed(0)
    T = sum(seqlens)
    cu = torch.tensor([0] + list(torch.tensor(seqlens).cumsum(0).tolist()), dtype=torch.int32)
    cols = (hq + 2 * hkv) * D + stride_extra
    qkv = torch.randn(T, cols)
    qkv[:, : hq * D] *= qscale
    qkv = qkv.bfloat16()
    q = qkv[:, : hq * D].view(T, hq, D)
    k = qkv[:, hq * D:(hq + hkv) * D].view(T, hkv, D)
    v = qkv[:, (hq + hkv) * D:(hq + 2 * hkv) * D].view(T, hkv, D)
    scale = 1 / math.sqrt(D)
    o_ref, lse_ref = dops.flash_attn_fwd(q, k, v, cu, max(seqlens), scale, causal, window)
    g = qkv.to(cuda)
    gq = g[:, : hq * D].view(T, hq, D)
    gk = g[:, hq * D:(hq + hkv) * D].view(T, hkv, D)
    gv = g[:, (hq + hkv) * D:(hq + 2 * hkv) * D].view(T, hkv, D)
    o, lse = dops.flash_attn_fwd(gq, gk, gv, cu.to(cuda), max(seqlens), scale, causal, window)
    _close(o, o_ref, 2e-2, 2e-2, "attn out")
    _close(lse, lse_ref, 2e-3, 1e-3, "lse")
    do = torch.randn(T, hq, D).bfloat16()
    dq_ref, dk_ref, dv_ref = dops.flash_attn_bwd(do, q, k, v, o_ref, lse_ref, cu, max(seqlens), scale, causal, window)
    dq, dk, dv = dops.flash_attn_bwd(do.to(cuda), gq, gk, gv, o, lse, cu.to(cuda), max(seqlens), scale, causal, window)
    for a, b, n in ((dq, dq_ref, "dq"), (dk, dk_ref, "dk"), (dv, dv_ref, "dv")):
        assert _rel(a, b) < 2e-2, f"{n} rel err {_rel(a, b)}"
    return qkv, cu


@pytest.mark.parametrize("D,hq,hkv,seqlens", [(64, 12, 12, [1024, 1024]), (64, 4, 4, [100, 257, 3, 667]),
                                               (128, 8, 2, [300, 131]), (128, 2, 1, [2048])])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_flash_attn_dropout_matches_masked_reference(cuda, D, hq, hkv, seqlens, causal, p, monkeypatch):
    """Attention-probability dropout inside the kernels (GPT-2's attn_pdrop) against the f32
    reference that applies the SAME Philox keep mask (dtg.ops._cpu.dropout_keep): forward, and
    the backward that regenerates the mask in both the query-stationary dQ kernel and the
    key-stationary dK/dV kernel (also with its query items split over workgroups).  A mask that
    differed in even a few elements per row would move the outputs far beyond the tolerance."""
    torch.manual_seed(1)
    T = sum(seqlens)
    cu = torch.tensor([0] + list(torch.tensor(seqlens).cumsum(0).tolist()), dtype=torch.int32)
    q = torch.randn(T, hq, D).bfloat16()
    k = torch.randn(T, hkv, D).bfloat16()
    v = torch.randn(T, hkv, D).bfloat16()
    do = torch.randn(T, hq, D).bfloat16()
    scale = 1 / math.sqrt(D)
    seed, off = 0x123456789AB, 77
    rng = torch.tensor([seed, off], dtype=torch.int64)
    o_ref, lse_ref = dops.flash_attn_fwd_drop(q, k, v, cu, max(seqlens), scale, causal, p, rng)
    o, lse = dops.flash_attn_fwd_drop(q.to(cuda), k.to(cuda), v.to(cuda), cu.to(cuda), max(seqlens), scale, causal, p,
                                      rng.to(cuda))
    _close(o, o_ref, 3e-2, 2e-2, "attn out (dropout)")
    _close(lse, lse_ref, 2e-3, 1e-3, "lse")
    ref = dops.flash_attn_bwd_drop(do, q, k, v, o_ref, lse_ref, cu, max(seqlens), scale, causal, p, rng)
    for split in (1, 3):
        with ops.fa_tuning(cuda, kv_split=split):
            got = dops.flash_attn_bwd_drop(do.to(cuda), q.to(cuda), k.to(cuda), v.to(cuda), o, lse, cu.to(cuda),
                                           max(seqlens), scale, causal, p, rng.to(cuda))
        for a, b, n in zip(got, ref, ("dq", "dk", "dv")):
            assert _rel(a, b) < 2e-2, f"{n} (split {split}) rel err {_rel(a, b)}"
    # another offset is another mask
    o2, _ = dops.flash_attn_fwd_drop(q.to(cuda), k.to(cuda), v.to(cuda), cu.to(cuda), max(seqlens), scale, causal, p,
                                     torch.tensor([seed, off + 1], dtype=torch.int64, device=cuda))
    assert _rel(o2, o_ref) > 5e-2
    # an offset past 2^32 keys the generator with its high word: the same mask as the CPU
    # reference, and not the mask of its low word alone
    big = torch.tensor([seed, off + (1 << 32)], dtype=torch.int64)
    o3_ref, _ = dops.flash_attn_fwd_drop(q, k, v, cu, max(seqlens), scale, causal, p, big)
    o3, _ = dops.flash_attn_fwd_drop(q.to(cuda), k.to(cuda), v.to(cuda), cu.to(cuda), max(seqlens), scale, causal, p,
                                     big.to(cuda))
    _close(o3, o3_ref, 3e-2, 2e-2, "attn out (dropout, offset >= 2^32)")
    assert _rel(o3, o_ref) > 5e-2


def test_gpt2_trains_through_the_dropout_kernels(cuda):
    """GPT-2 in train mode (attn_pdrop 0.1) runs its attention through the flash kernels
    (no [S, S] materialisation) and its loss decreases on a repeated batch."""
    from dtg.models import build_model, resolve_config
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    torch.manual_seed(0)
    cfg = resolve_config("gpt2")
    m = build_model(cfg, device=cuda)
    m.train()
    eng = DataParallel(m, mode="single")
    opt = FlatAdamW(eng, lr=1e-3)
    ids = torch.randint(0, cfg.vocab_size, (4, 1024), device=cuda)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        out = m(input_ids=ids, labels=ids)
        eng.backward(out.loss)
        opt.step()
        losses.append(out.loss.item())
    torch.cuda.synchronize()
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0] - 0.5, losses


@pytest.mark.parametrize("seqlens", [[1024], [100, 257, 667], [64, 1, 129, 130]])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_attn_d128_gqa(cuda, seqlens, causal):
    _attn_case(cuda, seqlens, hq=8, hkv=2, D=128, causal=causal, stride_extra=8)


@pytest.mark.parametrize("seqlens", [[512, 300]])
def test_flash_attn_d64_mha(cuda, seqlens):
    _attn_case(cuda, seqlens, hq=4, hkv=4, D=64, causal=True)


@pytest.mark.parametrize("causal", [True, False])
def test_flash_attn_fwd_large_logit_range(cuda, causal):
    """The forward against the fp32 reference on logits with a large dynamic range (qscale 8:
    the running max keeps growing by more than the lazy-rescale threshold, so the rescale path
    runs on many tiles), GQA and MHA, head_dim 128 and 64."""
    _attn_case(cuda, [1024, 77], hq=4, hkv=2, D=128, causal=causal, qscale=8.0)
    _attn_case(cuda, [512, 300], hq=4, hkv=4, D=64, causal=causal, qscale=8.0)


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_attn_bwd_kv_split(cuda, split, causal):
    """dK/dV with each key block's query items split over workgroups (f32 partials summed in
    split order, kv_split): matches the fp32 reference, is bitwise reproducible, and the
    single-GPU default (no split) is unchanged."""
    with ops.fa_tuning(cuda, kv_split=split):
        qkv, cu = _attn_case(cuda, [1024, 77, 300], hq=8, hkv=2, D=128, causal=causal, stride_extra=8)
        T, D, hq, hkv = qkv.shape[0], 128, 8, 2
        g = qkv.to(cuda)
        q, k, v = (g[:, a * D:b * D].view(T, b - a, D) for a, b in ((0, hq), (hq, hq + hkv), (hq + hkv, hq + 2 * hkv)))
        o, lse = dops.flash_attn_fwd(q, k, v, cu.to(cuda), 1024, D ** -0.5, causal, 0)
        torch.manual_seed(3)
        do = torch.randn(T, hq, D, device=cuda).bfloat16()
        a = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
        b = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with ops.fa_tuning(cuda, kv_split=1):
        ref = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
    assert torch.equal(a[0], ref[0])  # dQ is not affected
    for x, y in zip(a[1:], ref[1:]):
        assert _rel(x, y) < 1e-2


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D,hq,hkv", [(128, 8, 2), (64, 4, 4)])
def test_flash_attn_bwd_kv_qb64(cuda, D, hq, hkv, causal, split):
    """dK/dV with 64-query items (two-half software pipeline, kv_qb 64): the fp32 reference on
    varlen sequences whose lengths are not multiples of 64, alone and split; dQ is untouched and
    dK/dV agree with the 32-row items to summation-order rounding."""
    with ops.fa_tuning(cuda, kv_split=split, kv_qb=64):
        qkv, cu = _attn_case(cuda, [1024, 77, 300], hq=hq, hkv=hkv, D=D, causal=causal, stride_extra=8)
        T = qkv.shape[0]
        g = qkv.to(cuda)
        q, k, v = (g[:, a * D:b * D].view(T, b - a, D) for a, b in ((0, hq), (hq, hq + hkv), (hq + hkv, hq + 2 * hkv)))
        o, lse = dops.flash_attn_fwd(q, k, v, cu.to(cuda), 1024, D ** -0.5, causal, 0)
        torch.manual_seed(3)
        do = torch.randn(T, hq, D, device=cuda).bfloat16()
        a = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
        b = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    with ops.fa_tuning(cuda, kv_split=split, kv_qb=32):
        ref = dops.flash_attn_bwd(do, q, k, v, o, lse, cu.to(cuda), 1024, D ** -0.5, causal, 0)
    assert torch.equal(a[0], ref[0])
    for x, y in zip(a[1:], ref[1:]):
        assert _rel(x, y) < 1e-2


@pytest.mark.parametrize("window", [2, 64, 200, 5000])
@pytest.mark.parametrize("D,hq,hkv", [(128, 8, 2), (64, 4, 4)])
def test_flash_attn_sliding_window(cuda, window, D, hq, hkv):
    """Causal sliding window (query i sees keys i - window < j <= i): forward and both backward
    kernels vs the fp32 reference, windows inside one tile (2; a window of 1 makes dQ exactly 0), crossing tiles (64, 200) and
    longer than every sequence (5000 == full causal); varlen sequences, GQA and MHA."""
    _attn_case(cuda, [1024, 77, 300], hq=hq, hkv=hkv, D=D, causal=True, window=window)


@pytest.mark.parametrize("d", [80, 96])
def test_attention_padded_head_dims(cuda, d):
    """ops.attention with head dims the kernels are not instantiated for (zero-padded to 128 on
    the GPU) vs the fp32 CPU reference: output and the fused qkv gradient, RoPE on."""
    from dtg import ops as fops

    torch.manual_seed(0)
    lens = [300, 77]
    T, hq, hkv = sum(lens), 8, 2
    cu = torch.tensor([0, 300, 377], dtype=torch.int32)
    cos, sin = fops.rope_tables(d, 10000.0, 512)
    pos = torch.cat([torch.arange(n) for n in lens])
    qkv = torch.randn(T, (hq + 2 * hkv) * d).bfloat16()
    do = torch.randn(T, hq * d).bfloat16()
    ref_in = qkv.float().requires_grad_()
    o_ref = fops.attention(ref_in.clone(), hq, hkv, d, cu, 300, cos, sin, pos)
    o_ref.backward(do.float())
    g_in = qkv.to(cuda).requires_grad_()
    o = fops.attention(g_in, hq, hkv, d, cu.to(cuda), 300, cos.to(cuda), sin.to(cuda), pos.to(cuda))
    o.backward(do.to(cuda))
    _close(o, o_ref, 2e-2, 2e-2, "padded attn out")
    assert _rel(g_in.grad, ref_in.grad) < 2e-2, _rel(g_in.grad, ref_in.grad)


def test_flash_attn_bwd_qkv_fused(cuda):
    torch.manual_seed(0)
    T, hq, hkv, D = 384, 4, 1, 128
    cu = torch.tensor([0, 200, 384], dtype=torch.int32)
    qkv = torch.randn(T, (hq + 2 * hkv) * D).bfloat16()
    do = torch.randn(T, hq, D).bfloat16()
    scale = 1 / math.sqrt(D)
    views = lambda t: (t[:, : hq * D].view(T, hq, D), t[:, hq * D:(hq + hkv) * D].view(T, hkv, D), t[:, (hq + hkv) * D:].view(T, hkv, D))
    g = qkv.to(cuda)
    o, lse = dops.flash_attn_fwd(*views(g), cu.to(cuda), 200, scale, True)
    ref = torch.cat([t.reshape(T, -1) for t in dops.flash_attn_bwd(do.to(cuda), *views(g), o, lse, cu.to(cuda), 200, scale, True)], 1)
    fused = dops.flash_attn_bwd_qkv(do.to(cuda), g, hq, hkv, D, o, lse, cu.to(cuda), 200, scale, True)
    _close(fused, ref, 0, 0, "fused dqkv layout")


@pytest.mark.parametrize("name", ["llama-tiny-d128", "qwen2-tiny", "mistral-tiny"])
def test_llama_tiny_gpu_matches_cpu(cuda, name):
    """Whole model on the GPU kernels (bf16) vs the fp32 CPU model: loss and gradient norm
    (qwen2-tiny adds the q/k/v bias through the fused linear-with-bias backward; mistral-tiny
    runs 256-token rows through its 64-token sliding window)."""
    from dtg.models import build_model

    torch.manual_seed(0)
    cpu = build_model(name, device="cpu", dtype=torch.float32)
    with torch.no_grad():
        for n, p in cpu.named_parameters():
            if n.endswith(".bias"):
                p.normal_(0, 0.1)
    gpu = build_model(name, device=cuda)
    gpu.load_state_dict({k: v.bfloat16() for k, v in cpu.state_dict().items()})
    ids = torch.randint(0, cpu.config.vocab_size, (2, 256))
    lc = cpu(input_ids=ids, labels=ids).loss
    lg = gpu(input_ids=ids.to(cuda), labels=ids.to(cuda)).loss
    assert abs(lc.item() - lg.item()) < 0.05
    lg.backward()
    gn = torch.stack([p.grad.float().norm() for p in gpu.parameters()]).norm().item()
    lc.backward()
    cn = torch.stack([p.grad.float().norm() for p in cpu.parameters()]).norm().item()
    assert abs(gn - cn) / cn < 0.05


@pytest.mark.parametrize("T,V,H", [(4096, 50, 256), (1000, 32000, 4096), (77, 7, 520)])
def test_embedding_bwd_deterministic(cuda, T, V, H):
    """Sorted segment-sum embedding backward: matches the f32 index_add reference (rounded once
    per row) and is bitwise reproducible run to run (heavy id repetition at V=7/50)."""
    torch.manual_seed(0)
    ids = torch.randint(0, V, (T,))
    dy = torch.randn(T, H).bfloat16()
    base = torch.randn(V, H).bfloat16()
    ref = base.clone()
    dops.embedding_bwd_(ref, ids, dy)  # CPU f32 reference
    outs = []
    for _ in range(2):
        o = base.to(cuda)
        dops.embedding_bwd_(o, ids.to(cuda), dy.to(cuda))
        outs.append(o.cpu())
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], ref, atol=2e-2, rtol=1e-2, name="embedding_bwd")


@pytest.mark.parametrize("T,V,H,skip", [(16384, 16032, 4096, 7 / 8), (20001, 3, 520, 0.0), (4100, 64, 1032, 0.5)])
def test_embedding_bwd_long_runs_and_skipped_ids(cuda, T, V, H, skip):
    """Runs far longer than one chunk (a frequent token; T = 20001 over 3 ids) and ids of -1
    (vocab-parallel out-of-shard tokens, 7/8 of them at TP = 8): chunked partial sums merged in
    order match the f32 reference, skipped ids add nothing, and two calls agree bit for bit."""
    torch.manual_seed(1)
    ids = torch.randint(0, V, (T,))
    ids[torch.rand(T) < skip] = -1
    dy = torch.randn(T, H).bfloat16()
    base = torch.randn(V, H).bfloat16()
    ref = base.clone()
    dops.embedding_bwd_(ref, ids, dy)  # CPU f32 reference (skips ids outside [0, V))
    outs = []
    for _ in range(2):
        o = base.to(cuda)
        dops.embedding_bwd_(o, ids.to(cuda), dy.to(cuda))
        torch.cuda.synchronize()
        outs.append(o.cpu())
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], ref, atol=5e-2, rtol=1e-2, name="embedding_bwd_long")
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids[ids >= 0].unique()] = False
    assert torch.equal(outs[0][untouched], base[untouched])


@pytest.mark.parametrize("D,hq,hkv", [(128, 8, 2), (64, 4, 4)])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_attn_varlen_key_ranges(cuda, D, hq, hkv, causal):
    """Per-sequence key ranges (context parallelism): query sequences of len_q attend to
    disjoint key ranges of len_k >= len_q in a separate K/V tensor, causal mask bottom-right
    aligned; against the f32 reference, forward and backward (dK/dV zero outside the ranges)."""
    torch.manual_seed(0)
    qlens = [64, 200, 33, 128]
    klens = [192, 200, 161, 384]  # offsets 128, 0, 128, 256
    gaps = [5, 0, 17, 3]          # keys no sequence uses
    cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32)
    ks, pos = [], 0
    for g, n in zip(gaps, klens):
        pos += g
        ks.append(pos)
        pos += n
    Tk = pos + 7
    kstart = torch.tensor(ks, dtype=torch.int32)
    klen = torch.tensor(klens, dtype=torch.int32)
    T = int(cu[-1])
    q = torch.randn(T, hq, D).bfloat16()
    k = torch.randn(Tk, hkv, D).bfloat16()
    v = torch.randn(Tk, hkv, D).bfloat16()
    do = torch.randn(T, hq, D).bfloat16()
    scale = 1 / math.sqrt(D)
    args = (max(qlens), max(klens), scale, causal)
    o_ref, lse_ref = dops.flash_attn_varlen_fwd(q, k, v, cu, kstart, klen, *args)
    g = lambda t: t.to(cuda)
    o, lse = dops.flash_attn_varlen_fwd(g(q), g(k), g(v), g(cu), g(kstart), g(klen), *args)
    _close(o, o_ref, 2e-2, 2e-2, "varlen out")
    _close(lse, lse_ref, 2e-3, 1e-3, "varlen lse")
    ref = dops.flash_attn_varlen_bwd(do, q, k, v, o_ref, lse_ref, cu, kstart, klen, *args)
    got = dops.flash_attn_varlen_bwd(g(do), g(q), g(k), g(v), o, lse, g(cu), g(kstart), g(klen), *args)
    for a, b, n in zip(got, ref, ("dq", "dk", "dv")):
        assert _rel(a, b) < 2e-2, f"{n} rel err {_rel(a, b)}"
    assert float(got[1][:ks[0]].float().abs().max()) == 0.0  # untouched keys: zero gradient


@pytest.mark.parametrize("V", [1003, 50257, 1024])
@pytest.mark.parametrize("direct", [False, True])
def test_fused_linear_ce_odd_vocab(cuda, V, direct, monkeypatch):
    """Loss head with a vocabulary that is not a multiple of 8 (GPT-2, rime): the zero-padded
    weight / logits path gives the f32 loss, dH and dW (direct: dW written into main_grad in the
    forward, the engine-owned-loss path)."""
    from dtg.ops import functional as F_
    from dtg.ops import grad_routing as gr

    monkeypatch.setattr(F_, "_LINEAR_BWD", "tn")
    torch.manual_seed(0)
    T, H = 2048, 256
    h = torch.randn(T, H).bfloat16()
    w = (0.05 * torch.randn(V, H)).bfloat16()
    lab = torch.randint(0, V, (T,))
    lab[::7] = -100
    hg = h.to(cuda).requires_grad_()
    wg = w.to(cuda).requires_grad_()
    if direct:
        wg.main_grad = torch.zeros(V, H, dtype=torch.bfloat16, device=cuda)
        monkeypatch.setattr(gr, "_DIRECT_LOSS_GRAD", True)
    loss = F_.fused_linear_cross_entropy(hg, wg, lab.to(cuda), chunk=1024)
    loss.backward()
    hr, wr = h.float().requires_grad_(), w.float().requires_grad_()
    ref = torch.nn.functional.cross_entropy(hr @ wr.t(), lab, ignore_index=-100)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-3 * abs(ref.item())
    assert _rel(hg.grad, hr.grad) < 2e-2
    assert _rel(wg.main_grad if direct else wg.grad, wr.grad) < 2e-2
