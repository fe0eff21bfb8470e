"""Qwen3 (Llama layout + per-head q/k RMSNorm before RoPE, explicit head_dim) on the CPU: against
transformers' Qwen3ForCausalLM, through HF conversion, the bundled configs, and every place that names
parameters -- tensor / context / Ulysses parallel training against one process, TP sharding, the
DCP checkpoint across TP layouts and the safetensors loader.  The q/k norm weights are drawn at random
everywhere, so that ones cannot hide a swapped or dropped weight.
"""
import os

import pytest
import torch

import dtg  # noqa: F401

from _dist import run_distributed

MODEL = "qwen3-tiny"
TOL = dict(atol=3e-4, rtol=1e-3)


def _randomize_norms(model, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))


def _full_model(seed=0):
    from dtg.models import build_model, resolve_config

    cfg = resolve_config(MODEL)
    torch.manual_seed(seed)
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    _randomize_norms(m)
    return cfg, m


def _batches(n=3, rows=4, S=32):
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, 512, (rows, S), generator=g) for _ in range(n)]


def test_config_resolves_and_counts_parameters():
    from dtg.models import resolve_config

    cfg = resolve_config("Qwen/Qwen3-8B")
    assert cfg.model_type == "qwen3" and cfg.qk_norm and not cfg.attention_bias and cfg.sliding_window is None
    assert cfg.head_dim == 128 and cfg.num_attention_heads * cfg.head_dim == cfg.hidden_size
    assert abs(cfg.num_params() - 8.19e9) < 0.01 * 8.19e9
    small = resolve_config("Qwen/Qwen3-0.6B")
    assert small.head_dim == 128 and small.head_dim != small.hidden_size // small.num_attention_heads
    assert abs(small.num_params() - 0.596e9) < 0.01 * 0.596e9
    assert abs(small.num_params() - small.vocab_size * small.hidden_size - 0.44e9) < 0.01 * 0.44e9
    tiny = resolve_config(MODEL)
    assert tiny.head_dim == 64 != tiny.hidden_size // tiny.num_attention_heads
    assert resolve_config(MODEL, qk_norm=False).num_params() == tiny.num_params() - 2 * 2 * 64
    assert not resolve_config("llama-tiny").qk_norm and not resolve_config("qwen2-tiny").qk_norm


def test_model_has_hf_named_norm_weights_initialised_to_one():
    from dtg.models import build_model

    m = build_model(MODEL, device="cpu", dtype=torch.float32)
    sd = m.state_dict()
    for i in range(2):
        for nm in ("q_norm", "k_norm"):
            w = sd[f"layers.{i}.self_attn.{nm}.weight"]
            assert w.shape == (64,) and torch.equal(w, torch.ones(64))
    assert sum(p.numel() for p in m.parameters()) == m.config.num_params()


def test_qwen3_matches_hf_loss_logits_grads():
    from dtg.models.hf_compat import hf_causal_lm_class, hf_llama_config, llama_to_hf

    cfg, m = _full_model()
    hf = hf_causal_lm_class(cfg)(hf_llama_config(cfg)).float()
    assert type(hf).__name__ == "Qwen3ForCausalLM"
    hf.load_state_dict(llama_to_hf(m.state_dict(), cfg), strict=True)
    ids = torch.randint(0, cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(1))
    a = m(input_ids=ids, labels=ids, return_logits=True)
    b = hf(input_ids=ids, labels=ids)
    torch.testing.assert_close(a.logits, b.logits, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(a.loss, b.loss, atol=1e-5, rtol=1e-5)
    a.loss.backward()
    b.loss.backward()
    ga = llama_to_hf({n: p.grad for n, p in m.named_parameters()}, cfg)
    seen = 0
    for n, p in hf.named_parameters():
        if n == "lm_head.weight" and cfg.tie_word_embeddings:
            continue
        seen += n.endswith(("q_norm.weight", "k_norm.weight"))
        torch.testing.assert_close(ga[n], p.grad, atol=1e-4, rtol=1e-3, msg=n)
    assert seen == 2 * cfg.num_hidden_layers


def test_hf_state_dict_roundtrip():
    from dtg.models.hf_compat import llama_from_hf, llama_to_hf

    cfg, m = _full_model()
    sd = m.state_dict()
    hf = llama_to_hf(sd, cfg)
    assert "model.layers.1.self_attn.k_norm.weight" in hf
    back = llama_from_hf(hf, cfg)
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k


def test_tp_shard_roundtrip_keeps_norms_replicated():
    from dtg.parallel.tensor_parallel import shard_full_state_dict, unshard_state_dicts

    cfg, m = _full_model()
    sd = m.state_dict()
    shards = [shard_full_state_dict(sd, cfg, r, 2) for r in range(2)]
    for s in shards:
        assert torch.equal(s["layers.0.self_attn.q_norm.weight"], sd["layers.0.self_attn.q_norm.weight"])
        assert s["layers.0.self_attn.qkv_proj.weight"].shape[0] == (2 + 2 * 1) * 64
    full = unshard_state_dicts(shards, cfg)
    for k, v in sd.items():
        assert torch.equal(full[k], v), k


# ------------------------------------------------------------------------------ parallel training
def _train(rank, world, batches, kind):
    """`kind` = single | tp | cp | ulysses on `world` ranks: parameters after training, and losses."""
    import torch.distributed as dist

    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    cfg, full = _full_model()
    W = dist.group.WORLD if world > 1 else None
    if kind == "tp":
        from dtg.parallel.tensor_parallel import make_mesh, shard_full_state_dict

        _, tp_group, _, tp_rank, _ = make_mesh(world)
        model = build_model(cfg, device="cpu", dtype=torch.float32, tp_group=tp_group, init=False)
        model.load_state_dict(shard_full_state_dict(full.state_dict(), cfg, tp_rank, world))
        eng = DataParallel(model, mode="single", group=None, tp_group=tp_group, broadcast_from_rank0=False)
    elif kind in ("cp", "ulysses") and world > 1:
        model = build_model(cfg, device="cpu", dtype=torch.float32, init=False,
                            **({"cp_group": W} if kind == "cp" else {"sp_group": W}))
        model.load_state_dict(full.state_dict())
        eng = DataParallel(model, mode="ddp", bucket_mb=1, grad_divisor=1)
    else:
        model, eng = full, DataParallel(full, mode="single")
    opt = FlatAdamW(eng, lr=1e-2, eps=1e-3)
    losses = []
    for ids in batches:
        opt.zero_grad()
        if kind == "cp" and world > 1:
            from dtg.parallel.context_parallel import cp_batch

            x, lab, pos, nv = cp_batch(ids, rank, world)
            out = model(input_ids=x, labels=lab, position_ids=pos, num_valid=nv)
        elif kind == "ulysses" and world > 1:
            from dtg.parallel.ulysses import ulysses_batch

            x, lab, pos, nv = ulysses_batch(ids, rank, world, None)
            out = model(input_ids=x, labels=lab, position_ids=pos, num_valid=nv)
        else:
            out = model(input_ids=ids, labels=ids)
        eng.backward(out.loss)
        opt.step()
        losses.append(out.loss.item())
    return {n: p.detach().clone() for n, p in model.named_parameters()}, losses, rank


@pytest.fixture(scope="module")
def single_run():
    return _train(0, 1, _batches(), "single")


def _norm_moved(ref):
    w = ref["layers.0.self_attn.q_norm.weight"]
    g = torch.Generator().manual_seed(11)
    start = 1.0 + 0.3 * torch.randn(w.shape, generator=g)
    return (w - start).abs().max() > 1e-3


def test_tp2_training_matches_single(single_run):
    """Three AdamW steps at tp 2: every parameter, the TP-replicated q/k norm weights among them (their
    gradients are sums over each rank's local heads, all-reduced over the TP group), as on one process."""
    from dtg.models import resolve_config
    from dtg.parallel.tensor_parallel import unshard_state_dicts

    ref, ref_losses, _ = single_run
    assert _norm_moved(ref)
    res = run_distributed(_train, 2, _batches(), "tp")
    for r in res:  # replicated weights identical on both ranks
        for nm in ("q_norm", "k_norm"):
            k = f"layers.1.self_attn.{nm}.weight"
            assert torch.equal(r[0][k], res[0][0][k])
    full = unshard_state_dicts([r[0] for r in sorted(res, key=lambda r: r[2])], resolve_config(MODEL))
    for n, v in ref.items():
        torch.testing.assert_close(full[n], v, **TOL, msg=n)
    torch.testing.assert_close(torch.tensor(res[0][1]), torch.tensor(ref_losses), atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("kind", ["cp", "ulysses"])
def test_context_and_ulysses_parallel_match_single(single_run, kind):
    ref, ref_losses, _ = single_run
    res = run_distributed(_train, 2, _batches(), kind)
    assert abs(sum(r[1][0] for r in res) - ref_losses[0]) < 1e-4 * abs(ref_losses[0])
    for r in res:
        for n, v in ref.items():
            torch.testing.assert_close(r[0][n], v, **TOL, msg=f"{kind} rank {r[2]} {n}")


# ------------------------------------------------------------------------------ checkpoints, loading
def _dcp_engine(tp):
    import torch.distributed as dist

    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    cfg, full = _full_model()
    tp_group = None
    if tp > 1:
        from dtg.parallel.tensor_parallel import make_mesh, shard_full_state_dict

        _, tp_group, _, tp_rank, _ = make_mesh(tp)
        model = build_model(cfg, device="cpu", dtype=torch.float32, tp_group=tp_group, init=False)
        model.load_state_dict(shard_full_state_dict(full.state_dict(), cfg, tp_rank, tp))
    else:
        model = full
    assert tp == 1 or dist.is_initialized()
    eng = DataParallel(model, mode="single", tp_group=tp_group, broadcast_from_rank0=False)
    return cfg, model, eng, FlatAdamW(eng, lr=1e-2, eps=1e-3)


def _norm_state(eng, cfg):
    """{hf name: (param, exp_avg, exp_avg_sq)} of the q/k norm weights, via the DCP chunk geometry."""
    from dtg.train.dcp_ckpt import _chunks

    out = {}
    for hf, hshape, offs, sizes, views in _chunks(eng, cfg, keep=lambda n: n.endswith(("q_norm.weight", "k_norm.weight"))):
        assert list(hshape) == [cfg.head_dim] and list(offs) == [0] and list(sizes) == [cfg.head_dim], (hf, hshape, offs, sizes)
        out[hf] = tuple(views[k].clone() for k in ("p", "m", "v"))
    return out


def _dcp_save_tp2(rank, world, d):
    from dtg.train.dcp_ckpt import save_dcp

    cfg, model, eng, opt = _dcp_engine(2)
    for ids in _batches(2):
        opt.zero_grad()
        eng.backward(model(input_ids=ids, labels=ids).loss)
        opt.step()
    save_dcp(os.path.join(d, "checkpoint"), eng, opt, cfg, global_step=2)
    return _norm_state(eng, cfg)


def test_dcp_saved_at_tp2_resumes_at_tp1_with_norm_weights_and_moments(tmp_path):
    from dtg.train.dcp_ckpt import load_dcp

    d = str(tmp_path)
    saved = run_distributed(_dcp_save_tp2, 2, d)
    assert len(saved[0]) == 4 and set(saved[0]) == set(saved[1])
    cfg, model, eng, opt = _dcp_engine(1)
    for p in model.parameters():  # only the load may bring the values back
        p.data.zero_()
    meta = load_dcp(os.path.join(d, "checkpoint"), eng, cfg)
    assert meta["global_step"] == 2
    got = _norm_state(eng, cfg)
    for hf, (p, m, v) in saved[0].items():
        assert hf.startswith("model.layers.") and ".self_attn." in hf
        assert m.abs().max() > 0 and v.abs().max() > 0
        for a, b in zip(got[hf], (p, m, v)):
            assert torch.equal(a, b), hf


def test_load_pretrained_reads_norm_weights_from_safetensors(tmp_path):
    from safetensors.torch import save_file

    from dtg.models import build_model
    from dtg.models.hf_compat import llama_to_hf
    from dtg.models.loading import load_pretrained
    from dtg.parallel.data_parallel import DataParallel

    cfg, src = _full_model(seed=123)
    ref = {k: v.clone() for k, v in src.state_dict().items()}
    hf = llama_to_hf(ref, cfg)
    hf.pop("lm_head.weight")  # tied: stored once
    save_file({k: v.contiguous() for k, v in hf.items()}, str(tmp_path / "model.safetensors"))
    torch.manual_seed(7)
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    eng = DataParallel(m, mode="single")
    load_pretrained(eng, str(tmp_path), cfg)
    sd = m.state_dict()
    assert not torch.equal(ref["layers.1.self_attn.k_norm.weight"], torch.ones(64))
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k
