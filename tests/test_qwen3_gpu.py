"""qwen3-tiny in bf16 on the GPU through the fused QK-norm + RoPE kernel: accuracy against an f32 CPU
run of the same weights with the composed path's own error as the yardstick (the method and margin of
test_gpt2_fused_gpu.py), and the chapter-01 engine under a captured HIP graph.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 2, 128
MAX_RATIO = 1.5  # the fused path's worst error: at most 1.5 x the composed path's


def _ids(cfg):
    return torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(3))


def _randomize_norms(model):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_((1.0 + 0.3 * torch.randn(p.shape, generator=g)).to(p.dtype))


def _loss_and_grads(model, ids):
    for p in model.parameters():
        p.grad = None
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    return loss.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}


def _rel(a, ref):
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("head_dim", [64, 128])
def test_fused_is_as_close_to_f32_as_composed(cuda, monkeypatch, head_dim):
    from dtg.models import build_model, resolve_config
    from dtg.ops import functional

    torch.manual_seed(0)
    cfg = resolve_config("qwen3-tiny", head_dim=head_dim)
    model = build_model(cfg, device=cuda)
    _randomize_norms(model)
    ids = _ids(cfg)
    ref_model = build_model(cfg, device="cpu", dtype=torch.float32, init=False)
    ref_model.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    loss_r, grads_r = _loss_and_grads(ref_model, ids)
    errs = {}
    for fused in (False, True):
        monkeypatch.setattr(functional, "_QKNORM_FUSED", fused)
        loss, grads = _loss_and_grads(model, ids.to(cuda))
        assert math.isfinite(loss.item())
        errs[fused] = {"loss": abs((loss - loss_r).item()) / abs(loss_r.item())}
        errs[fused].update({n: _rel(g, grads_r[n]) for n, g in grads.items()})
    worst = max(errs[True][n] / max(errs[False][n], 1e-30) for n in errs[True] if n != "loss")
    for n in errs[True]:
        print(f"[qwen3 fused D{head_dim}] {n}: fused {errs[True][n]:.3e} composed {errs[False][n]:.3e} "
              f"ratio {errs[True][n] / max(errs[False][n], 1e-30):.2f}")
    print(f"[qwen3 fused D{head_dim}] worst gradient ratio {worst:.2f}")
    for n in errs[True]:
        assert errs[True][n] <= MAX_RATIO * errs[False][n], (n, errs[True][n], errs[False][n])


def _setup(dev):
    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    torch.manual_seed(0)
    model = build_model("qwen3-tiny", device=dev)
    _randomize_norms(model)
    eng = DataParallel(model, mode="single")
    return model, eng, FlatAdamW(eng, lr=1e-3)


def test_graphed_steps_match_eager_and_loss_falls(cuda):
    """The chapter-01 engine (single-GPU DataParallel + FlatAdamW) on one repeated batch: two eager
    warm-up steps, then three replays of the captured step; same losses as the eager loop."""
    from dtg.train.graph import GraphedStep

    b = torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(1)).to(cuda)
    nv = B * (S - 1)
    model, eng, opt = _setup(cuda)
    eager = []
    for _ in range(5):
        opt.zero_grad()
        out = model(input_ids=b, labels=b, num_valid=nv)
        eng.backward(out.loss)
        opt.step()
        eager.append(out.loss.item())
    model, eng, opt = _setup(cuda)
    step = GraphedStep(model, eng, opt, None, warmup=2, num_valid=nv)
    losses = [step({"input_ids": b, "labels": b}).item() for _ in range(5)]
    assert step.graph is not None and step.steps == 5
    torch.cuda.synchronize()
    print(f"[qwen3 graph] eager {eager} graphed {losses}")
    assert all(math.isfinite(x) for x in losses)
    assert all(b_ <= a_ for a_, b_ in zip(losses, losses[1:])), losses
    for a_, e_ in zip(losses, eager):
        assert abs(a_ - e_) <= 2e-3 * abs(e_), (losses, eager)
