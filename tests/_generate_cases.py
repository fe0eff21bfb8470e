"""Tiny random-init models (2 layers, hidden 256, head dim 64) of every supported type and the checks
of the KV-cache generation path shared by test_generate_cpu.py and test_generate_gpu.py.

The tolerances are measured, not fixed: an f32 reference of the same model (weights upcast, CPU ops)
gives e_full, the largest logit error of the EXISTING bf16 full forward; the cached path must stay
within 2 * e_full of the same reference (its GEMMs run at M = B instead of M = T and its softmax is
split in another order), and greedy ids must agree wherever the reference's top-1 / top-2 gap exceeds
4 * e_full (two paths, each up to 2 * e_full off, in opposite directions)."""
import functools

import torch

from dtg.models import build_model, resolve_config
from dtg.models.generation import KVCache, decode_step, generate, prefill

VOCAB = 512
# type -> (bundled tiny config, overrides, seed).
#
# A plain random-init head has top-1 / top-2 gaps of the size of the bf16 error at a third of the
# positions, far over the 10 % cap of the gap rule; a tied head makes every model repeat its last token
# for ever, and on a constant sequence a loop that fed back the wrong token would go unseen.  So the
# head is untied and its rows are the embedding rows moved along one random cycle through the whole
# vocabulary (head row succ(i) = embedding row i), with the embedding drawn EMB_GAIN times wider than
# the config's initializer_range: the residual stream is led by the last token's embedding, succ(last
# token) is the clear favourite, and greedy ids walk the cycle -- every id is new, and is right only if
# exactly the previous id was fed back.  check_greedy asserts that the ids do not repeat.  The layer
# weights are drawn LAYER_GAIN times wider, so attention and the MLP still move the logits by several
# times the bf16 error (the teacher-forced check is the one that is sensitive to them: with the decode
# attention zeroed, or its newest key dropped, it fails for every model type, while greedy ids on
# this head mostly survive).  Gains and seed were chosen on the CPU so that the reference's gaps leave no
# position under the gap rule (wider layers, LAYER_GAIN 2 with EMB_GAIN 6, left 2-4 of 48 there: too
# close to the cap of 4); the tests fail if the cap is exceeded.
LAYER_GAIN = 1.5
EMB_GAIN = 6.0
MODELS = {
    "llama": ("llama-tiny", dict(num_attention_heads=4, num_key_value_heads=2), 24),
    "qwen2": ("qwen2-tiny", dict(num_attention_heads=4, num_key_value_heads=1), 24),
    "qwen3": ("qwen3-tiny", dict(num_attention_heads=4, num_key_value_heads=2), 24),
    "mistral": ("mistral-tiny", dict(num_attention_heads=4, num_key_value_heads=2, sliding_window=16), 24),
}
SEQ, PREFIX, STEPS = 48, 8, 40       # teacher forcing: prefill on 8 tokens, then 40 decode steps
SHORTER = 3                          # the second sequence of the batch is this much shorter
NEW_TOKENS, MAX_EXCLUDED = 24, 0.10  # greedy equality
SAMPLE_T = 4.0                       # the favourite leads by about 10: at temperature 1 sampling would be greedy


def config(kind):
    name, over, _ = MODELS[kind]
    return resolve_config(name, num_hidden_layers=2, hidden_size=256, intermediate_size=512, head_dim=64,
                          vocab_size=VOCAB, tie_word_embeddings=False, **over)


def successor(kind):
    """succ [VOCAB]: one cycle through every id, drawn from the model's seed."""
    order = torch.randperm(VOCAB, generator=torch.Generator().manual_seed(1000 + MODELS[kind][2]))
    succ = torch.empty(VOCAB, dtype=torch.long)
    succ[order] = order.roll(-1)
    return succ


@functools.lru_cache(maxsize=None)
def models(kind, dev):
    """(bf16 model on `dev`, its f32 upcast on the CPU)."""
    cfg = config(kind)
    torch.manual_seed(MODELS[kind][2])
    m = build_model(cfg, dtype=torch.bfloat16)
    with torch.no_grad():
        for layer in m.layers:
            for w in (layer.self_attn.qkv_proj.weight, layer.self_attn.o_proj.weight, layer.mlp.gate_up_proj.weight,
                      layer.mlp.down_proj.weight):
                w.mul_(LAYER_GAIN)
        m.embed_tokens.weight.mul_(EMB_GAIN)
        m.lm_head.weight[successor(kind)] = m.embed_tokens.weight
    if cfg.attention_bias:  # zero-init biases would not test the bias path
        for layer in m.layers:
            layer.self_attn.qkv_proj.bias.data.normal_(0.0, 0.1)
    ref = build_model(cfg, dtype=torch.float32, init=False)
    ref.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    return m.to(dev).eval(), ref.eval()


def sequences(kind):
    g = torch.Generator().manual_seed(100 + MODELS[kind][2])
    return torch.randint(0, VOCAB, (SEQ,), generator=g), torch.randint(0, VOCAB, (SEQ - SHORTER,), generator=g)


@torch.no_grad()
def full_logits(model, ids):
    """Logits [L, V] (f32, CPU) of the existing full forward; row t = last position of prefix t + 1."""
    dev = next(model.parameters()).device
    return model(input_ids=ids[None].to(dev), return_logits=True).logits[0].float().cpu()


def check_teacher_forced(kind, dev):
    model, ref = models(kind, dev)
    seqs = sequences(kind)
    pre = [PREFIX, PREFIX - SHORTER]
    cache = KVCache(model.config, 2, SEQ, device=dev)
    got = [[lg] for lg in prefill(model, [s[:p] for s, p in zip(seqs, pre)], cache).float().cpu()]
    for t in range(STEPS):
        lg = decode_step(model, torch.stack([s[p + t] for s, p in zip(seqs, pre)]), cache).float().cpu()
        for i in range(2):
            got[i].append(lg[i])
    e_full = e_cached = 0.0
    for s, p, g in zip(seqs, pre, got):
        r = full_logits(ref, s)[p - 1: p + STEPS]
        e_full = max(e_full, (full_logits(model, s)[p - 1: p + STEPS] - r).abs().max().item())
        e_cached = max(e_cached, (torch.stack(g) - r).abs().max().item())
    print(f"[generate] {kind} teacher-forced: e_full {e_full:.5f}, e_cached {e_cached:.5f} (allowed {2 * e_full:.5f})")
    assert e_full > 0
    assert e_cached <= 2 * e_full, f"{kind}: cached path error {e_cached} > 2 * {e_full}"


def check_greedy(kind, dev):
    model, ref = models(kind, dev)
    prompts = [s[:p] for s, p in zip(sequences(kind), (PREFIX, PREFIX - SHORTER))]
    outs = generate(model, prompts, NEW_TOKENS, temperature=0.0)
    # generate()'s loop is prefill + decode_step fed with its own argmax, nothing else: the same ids
    # bit for bit from the two functions the teacher-forced check holds to the full forward
    cache = KVCache(model.config, 2, max(len(p) for p in prompts) + NEW_TOKENS, device=dev)
    nxt = prefill(model, prompts, cache).argmax(-1)
    manual = [nxt.cpu()]
    for _ in range(NEW_TOKENS - 1):
        nxt = decode_step(model, nxt, cache).argmax(-1)
        manual.append(nxt.cpu())
    assert torch.equal(torch.stack(outs), torch.stack(manual, 1)), "generate() differs from prefill + decode_step"
    excluded = total = 0
    for pr, out in zip(prompts, outs):
        assert out.shape == (NEW_TOKENS,) and out.dtype == torch.long
        distinct = len(set(out.tolist()))
        print(f"[generate] {kind} greedy ids ({distinct} distinct): {out.tolist()}")
        assert distinct >= NEW_TOKENS - 2, f"{kind}: degenerate continuation {out.tolist()}"
        ids = torch.cat([pr, out])
        sl = slice(len(pr) - 1, len(ids) - 1)        # positions whose argmax is a generated id
        r, f = full_logits(ref, ids)[sl], full_logits(model, ids)[sl]
        e_full = (f - r).abs().max().item()
        top = r.topk(2, -1).values
        sure = (top[:, 0] - top[:, 1]) > 4 * e_full
        recompute = f.argmax(-1)                     # greedy by full recompute on the same prefixes
        bad = sure & (recompute != out)
        assert not bad.any(), f"{kind}: cached ids {out[bad].tolist()} != recomputed {recompute[bad].tolist()} at {bad.nonzero().flatten().tolist()}"
        excluded += int((~sure).sum())
        total += NEW_TOKENS
    print(f"[generate] {kind} greedy: {excluded} of {total} positions under the gap rule")
    assert excluded <= MAX_EXCLUDED * total, f"{kind}: {excluded} of {total} positions excluded by the gap rule"


def check_eos(kind, dev):
    """Sampled ids with and without an EOS id (same seed, so the same draws): each sequence ends with its
    first EOS, and the two sequences stop at different steps."""
    model, _ = models(kind, dev)
    prompts = [s[:n] for s, n in zip(sequences(kind), (6, 4))]
    n = 40
    free = generate(model, prompts, n, temperature=SAMPLE_T, seed=5)

    def first(seq, tok):
        hit = (seq == tok).nonzero()
        return int(hit[0]) + 1 if len(hit) else n

    eos = next((int(t) for t in free[0][:-1] if first(free[0], t) != first(free[1], t)), None)
    assert eos is not None, "no id stops the two sequences at different steps"
    got = generate(model, prompts, n, temperature=SAMPLE_T, seed=5, eos_token_id=eos)
    lens = [first(f, eos) for f in free]
    assert lens[0] != lens[1] and lens[0] < n
    for f, g, k in zip(free, got, lens):
        assert torch.equal(g, f[:k]), (g.tolist(), f[:k].tolist())


def check_sampling_seeds(kind, dev):
    model, _ = models(kind, dev)
    prompts = [s[:n] for s, n in zip(sequences(kind), (6, 4))]
    a = generate(model, prompts, 12, temperature=SAMPLE_T, top_k=50, top_p=0.95, seed=1)
    b = generate(model, prompts, 12, temperature=SAMPLE_T, top_k=50, top_p=0.95, seed=1)
    c = generate(model, prompts, 12, temperature=SAMPLE_T, top_k=50, top_p=0.95, seed=2)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "same seed, different ids"
    assert any(not torch.equal(x, y) for x, y in zip(a, c)), "different seeds, same ids"
    assert all(0 <= int(t) < VOCAB for x in a for t in x)
