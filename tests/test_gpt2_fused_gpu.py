"""GPT-2 through the fused LayerNorm / dropout-add-LayerNorm / GELU-MLP path (models/gpt2.py FUSED)
on gpt2-tiny with 2 x 128 tokens: accuracy against an f32 CPU run with the ATen path's own error as
the yardstick, dropout determinism, HIP-graph replays, and FUSED = False against the ATen calls in
sequence.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, S = 2, 128
MAX_RATIO = 1.5  # the fused path places its roundings differently: at most 1.5 x the ATen path's error


def _ids(cfg):
    return torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(3))


def _build(cuda, **overrides):
    from dtg.models import build_model, resolve_config

    torch.manual_seed(0)
    cfg = resolve_config("gpt2-tiny", **overrides)
    return cfg, build_model(cfg, device=cuda)


def _loss_and_grads(model, ids):
    for p in model.parameters():
        p.grad = None
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    return loss.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}


def _rel(a, ref):
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def test_eval_fused_is_as_close_to_f32_as_aten(cuda, monkeypatch):
    from dtg.models import build_model, gpt2

    cfg, model = _build(cuda)
    model.eval()
    ids = _ids(cfg)
    ref_model = build_model(cfg, device="cpu", dtype=torch.float32, init=False)
    ref_model.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    ref_model.eval()
    loss_r, grads_r = _loss_and_grads(ref_model, ids)
    errs = {}
    for fused in (False, True):
        monkeypatch.setattr(gpt2, "FUSED", fused)
        loss, grads = _loss_and_grads(model, ids.to(cuda))
        errs[fused] = {"loss": abs((loss - loss_r).item()) / abs(loss_r.item())}
        errs[fused].update({n: _rel(g, grads_r[n]) for n, g in grads.items()})
    worst = 0.0
    for n in errs[True]:
        ratio = errs[True][n] / max(errs[False][n], 1e-30)
        worst = max(worst, ratio) if n != "loss" else worst
        print(f"[gpt2 fused] {n}: fused {errs[True][n]:.3e} aten {errs[False][n]:.3e} ratio {ratio:.2f}")
    print(f"[gpt2 fused] worst gradient ratio {worst:.2f}")
    for n in errs[True]:
        assert errs[True][n] <= MAX_RATIO * errs[False][n], (n, errs[True][n], errs[False][n])


def _train_loss(model, ids, seed):
    torch.manual_seed(seed)
    return _loss_and_grads(model, ids)


def test_train_residual_dropout_is_seeded(cuda):
    cfg, model = _build(cuda, resid_pdrop=0.5)
    model.train()
    ids = _ids(cfg).to(cuda)
    l0, g0 = _train_loss(model, ids, 11)
    assert math.isfinite(l0.item()) and all(torch.isfinite(g).all() for g in g0.values())
    l1, _ = _train_loss(model, ids, 11)
    l2, _ = _train_loss(model, ids, 12)
    assert l0.item() == l1.item(), (l0, l1)
    assert l0.item() != l2.item(), (l0, l2)


def test_graphed_gpt2_residual_dropout_redraws_every_replay(cuda):
    """As test_graphed_gpt2_attention_dropout_redraws_every_replay, with the randomness in the fused
    dropout + add + LayerNorm (and the MLP branch's ATen dropout) instead of the attention: lr = 0,
    one repeated batch, so the replayed losses differ only through the masks."""
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW
    from dtg.train.graph import GraphedStep

    cfg, model = _build(cuda, resid_pdrop=0.5, embd_pdrop=0.0, attn_pdrop=0.0)
    model.train()
    eng = DataParallel(model, mode="single")
    opt = FlatAdamW(eng, lr=0.0, weight_decay=0.0)
    b = _ids(cfg).to(cuda)
    step = GraphedStep(model, eng, opt, None, warmup=2, num_valid=B * (S - 1))
    losses = [step({"input_ids": b, "labels": b}).item() for _ in range(6)]
    assert step.graph is not None
    replays = losses[2:]
    assert len(set(replays)) == len(replays), losses


def _aten_forward(model, ids):
    """The forward of models/gpt2.py before the fused path existed: the ATen calls in sequence."""
    from dtg import ops

    cfg = model.config
    T = ids.numel()
    dev = ids.device
    pos = torch.arange(S, device=dev).repeat(B)
    cu = torch.arange(0, (B + 1) * S, S, device=dev, dtype=torch.int32)
    training = model.training
    x = ops.embedding(ids.reshape(-1), model.wte.weight) + F.embedding(pos, model.wpe.weight)
    x = F.dropout(x, cfg.embd_pdrop if training else 0.0, training)

    def ln(m, t):
        return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, m.eps)

    for blk in model.h:
        p_attn = cfg.attn_pdrop if training else 0.0
        p_res = cfg.resid_pdrop if training else 0.0
        qkv = ops.linear(ln(blk.ln_1, x), blk.c_attn.weight, blk.c_attn.bias)
        a = ops.attention(qkv, blk.nh, blk.nh, blk.d, cu, S, dropout_p=p_attn)
        x = x + F.dropout(ops.linear(a, blk.c_proj.weight, blk.c_proj.bias), p_res, training)
        m = F.gelu(ops.linear(ln(blk.ln_2, x), blk.c_fc.weight, blk.c_fc.bias), approximate="tanh")
        x = x + F.dropout(ops.linear(m, blk.mlp_proj.weight, blk.mlp_proj.bias), p_res, training)
    h = ln(model.ln_f, x)
    shifted = torch.full_like(ids, -100)
    shifted[:, :-1] = ids[:, 1:]
    return ops.fused_linear_cross_entropy(h, model.wte.weight, shifted.reshape(-1), num_valid=B * (S - 1))


@pytest.mark.parametrize("train", [False, True])
def test_fused_off_is_the_aten_sequence(cuda, monkeypatch, train):
    from dtg.models import gpt2

    monkeypatch.setattr(gpt2, "FUSED", False)
    cfg, model = _build(cuda, resid_pdrop=0.5 if train else 0.0)
    model.train(train)
    ids = _ids(cfg).to(cuda)
    with torch.no_grad():
        torch.manual_seed(5)
        got = model(input_ids=ids, labels=ids).loss
        torch.manual_seed(5)
        want = _aten_forward(model, ids)
    assert torch.equal(got, want), (got, want)


def test_gelu_mlp_tn_path_matches_the_unfused_layers(cuda):
    """T = 4096 takes the gelu_bwd_t path (transposed operands written by the kernel).  Output and
    gradients against an f32 CPU evaluation, with the unfused layers (ops.linear + F.gelu) as the
    yardstick, as in the model-level test."""
    _gelu_mlp_against_the_unfused_layers(cuda)


def test_gelu_mlp_native_path_matches_the_unfused_layers(cuda, monkeypatch):
    """The same with DTG_LINEAR_BWD=native: gelu_fwd + gelu_bwd and the strided GEMMs, the unfused
    branch of the MLP backward (test_swiglu_mlp_bwd[native] is its SwiGLU twin)."""
    from dtg.ops import functional as F_

    monkeypatch.setattr(F_, "_LINEAR_BWD", "native")
    _gelu_mlp_against_the_unfused_layers(cuda)


def _gelu_mlp_against_the_unfused_layers(cuda):
    from dtg import ops

    T, Hd, I = 4096, 64, 256
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, Hd, generator=g)
    w_fc, b_fc = 0.1 * torch.randn(I, Hd, generator=g), 0.1 * torch.randn(I, generator=g)
    w_pr, b_pr = 0.1 * torch.randn(Hd, I, generator=g), 0.1 * torch.randn(Hd, generator=g)
    dy = torch.randn(T, Hd, generator=g)
    bf = [t.to(torch.bfloat16) for t in (x, w_fc, b_fc, w_pr, b_pr, dy)]

    def run(fn, tensors):
        *ins, d = tensors
        ins = [t.clone().requires_grad_() for t in ins]
        y = fn(*ins)
        y.backward(d)
        return [y.detach().double().cpu()] + [t.grad.double().cpu() for t in ins]

    def unfused(a, w1, b1, w2, b2):
        return ops.linear(F.gelu(ops.linear(a, w1, b1), approximate="tanh"), w2, b2)

    def f32(a, w1, b1, w2, b2):
        return F.linear(F.gelu(F.linear(a, w1, b1), approximate="tanh"), w2, b2)

    ref = run(f32, [t.float() for t in bf])
    dev = [t.to(cuda) for t in bf]
    fused, plain = run(ops.gelu_mlp, dev), run(unfused, dev)
    for name, a, c, r in zip(("y", "dx", "dw_fc", "db_fc", "dw_proj", "db_proj"), fused, plain, ref):
        ef, ep = _rel(a, r), _rel(c, r)
        print(f"[gelu_mlp] {name}: fused {ef:.3e} unfused {ep:.3e}")
        assert ef <= MAX_RATIO * ep, (name, ef, ep)
