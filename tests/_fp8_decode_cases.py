"""Checks of the weight-only FP8 decode mode (linear="skinny-fp8"), shared by test_fp8_decode_cpu.py and
test_fp8_decode_gpu.py.  Models, sequences and measures are those of tests/_generate_cases.py and
tests/_decode_graph_cases.py (read only).

The oracle is the dequantised twin: a deep copy of the bf16 model with every quantised matrix replaced by
Fp8DecodeWeights.dequantized(name), and the twin's f32 upcast on the CPU.  With power-of-two scales
float(wq) * scale is exactly a bf16 value, so the FP8 decode path on the original model and the bf16 paths on
the twin compute the same mathematical function, and the twin's errors are measured with code this change
does not touch.  "The FP8 path" includes the prefill of such a run, prefill(model, ..., fp8=weights): hipBLASLt on
the dequantised matrices.  A prefill on the model's own weights fills the cache from another model than the
twin, and the decode steps that attend to it then miss the 2 * e_full margin (0.20-0.27 against e_full
0.07-0.09 on the CPU operators)."""
import copy
import functools

import torch

import _decode_graph_cases as dc
import _generate_cases as gc
from dtg.models import Fp8DecodeWeights, build_model
from dtg.models.decode_graph import GraphedDecode
from dtg.models.generation import KVCache, decode_step, generate, prefill

NEW, S_MAX = dc.NEW, dc.S_MAX


@functools.lru_cache(maxsize=None)
def twins(kind, dev):
    """(the bf16 model on `dev`, its Fp8DecodeWeights, the dequantised twin on `dev`, the twin's f32 upcast on the CPU)."""
    model, _ = gc.models(kind, dev)
    fp8 = Fp8DecodeWeights(model)
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for name in fp8.names():
            twin.get_submodule(name).weight.copy_(fp8.dequantized(name))
    ref = build_model(gc.config(kind), dtype=torch.float32, init=False)
    ref.load_state_dict({k: v.float().cpu() for k, v in twin.state_dict().items()})
    return model, fp8, twin.eval(), ref.eval()


def check_teacher_forced(kind, dev):
    """dc.check_teacher_forced_skinny with the decode steps in ops.skinny_linear_fp8, measured against the
    twin's f32 model; e_full is the error of the twin's bf16 full forward against the same reference."""
    model, fp8, twin, ref = twins(kind, dev)
    seqs = gc.sequences(kind)
    pre = [gc.PREFIX, gc.PREFIX - gc.SHORTER]
    cache = KVCache(model.config, 2, gc.SEQ, device=dev)
    got = [[lg] for lg in prefill(model, [s[:p] for s, p in zip(seqs, pre)], cache, fp8=fp8).float().cpu()]
    for t in range(gc.STEPS):
        tok = torch.stack([s[p + t] for s, p in zip(seqs, pre)])
        lg = decode_step(model, tok, cache, linear="skinny-fp8", fp8=fp8).float().cpu()
        for i in range(2):
            got[i].append(lg[i])
    e_full = e_cached = e_prefill = 0.0
    for s, p, g in zip(seqs, pre, got):
        r = gc.full_logits(ref, s)[p - 1: p + gc.STEPS]
        e_full = max(e_full, (gc.full_logits(twin, s)[p - 1: p + gc.STEPS] - r).abs().max().item())
        e = (torch.stack(g) - r).abs().amax(-1)
        e_prefill, e_cached = max(e_prefill, e[0].item()), max(e_cached, e.max().item())
    print(f"[fp8-decode] {kind} teacher-forced skinny-fp8: e_full {e_full:.5f}, e_cached {e_cached:.5f} "
          f"(allowed {2 * e_full:.5f}; the prefill's own logits {e_prefill:.5f})")
    assert e_full > 0
    assert e_cached <= 2 * e_full, f"{kind}: skinny-fp8 cached path error {e_cached} > 2 * {e_full}"


def check_greedy(kind, dev):
    """generate(linear="skinny-fp8") against the twin's full recompute under gc.check_greedy's gap rule."""
    model, fp8, twin, ref = twins(kind, dev)
    prompts = [s[:p] for s, p in zip(gc.sequences(kind), (gc.PREFIX, gc.PREFIX - gc.SHORTER))]
    outs = generate(model, prompts, gc.NEW_TOKENS, linear="skinny-fp8", fp8=fp8)
    excluded = total = 0
    for pr, out in zip(prompts, outs):
        assert out.shape == (gc.NEW_TOKENS,) and out.dtype == torch.long
        distinct = len(set(out.tolist()))
        print(f"[fp8-decode] {kind} greedy ids ({distinct} distinct): {out.tolist()}")
        assert distinct >= gc.NEW_TOKENS - 2, f"{kind}: degenerate continuation {out.tolist()}"
        ids = torch.cat([pr, out])
        sl = slice(len(pr) - 1, len(ids) - 1)
        r, f = gc.full_logits(ref, ids)[sl], gc.full_logits(twin, ids)[sl]
        e_full = (f - r).abs().max().item()
        top = r.topk(2, -1).values
        sure = (top[:, 0] - top[:, 1]) > 4 * e_full
        recompute = f.argmax(-1)
        bad = sure & (recompute != out)
        assert not bad.any(), f"{kind}: fp8 ids {out[bad].tolist()} != the twin's {recompute[bad].tolist()} at {bad.nonzero().flatten().tolist()}"
        excluded += int((~sure).sum())
        total += gc.NEW_TOKENS
        print(f"[fp8-decode] {kind} greedy: e_full {e_full:.5f}")
    print(f"[fp8-decode] {kind} greedy: {excluded} of {total} positions under the gap rule")
    assert excluded <= gc.MAX_EXCLUDED * total, f"{kind}: {excluded} of {total} positions excluded by the gap rule"


def _pair(model, prompts, gd, **kw):
    graph = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny-fp8", decode=gd, fp8=gd.fp8, **kw)
    eager = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny-fp8", decode="eager", bucketed=True, fp8=gd.fp8, **kw)
    return graph, eager


def check_graph_bitwise(kind, dev):
    """The captured loop returns the bucketed eager loop's ids bit for bit: greedy, and under the fused sampler
    with one greedy and one sampled row.  2 captures (one per length bucket) per sampler kind."""
    model, fp8, _, _ = twins(kind, dev)
    prompts = dc.long_prompts(kind)
    gd = GraphedDecode(model, 2, S_MAX, linear="skinny-fp8", fp8=fp8)
    assert gd.fp8 is fp8
    graph, eager = _pair(model, prompts, gd)
    assert gd.captures == 2 and gd.replays >= 18, (gd.captures, gd.replays, gd.eager_steps)
    for g, e in zip(graph, eager):
        assert g.shape == (NEW,) and torch.equal(g, e), (g.tolist(), e.tolist())
        assert len(set(g.tolist())) >= NEW - 2, f"degenerate continuation {g.tolist()}"
    fused = dict(sampler="fused", temperature=[0.0, gc.SAMPLE_T], top_k=[0, 50], top_p=[1.0, 0.95], seed=5)
    graph2, eager2 = _pair(model, prompts, gd, **fused)
    assert gd.captures == 4
    for g, e in zip(graph2, eager2):
        assert torch.equal(g, e), (g.tolist(), e.tolist())
    assert torch.equal(graph2[0], graph[0]), "the greedy row depends on its neighbour"
    built = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny-fp8", decode="graph")  # quantises for itself
    assert all(torch.equal(a, b) for a, b in zip(built, graph))


def check_model_untouched(kind, dev, monkeypatch):
    """Building the FP8 copies and generating with them leaves the model and the other modes as they were, and
    weights that are handed in are used as they are."""
    model, _ = gc.models(kind, dev)
    prompts = [s[:p] for s, p in zip(gc.sequences(kind), (gc.PREFIX, gc.PREFIX - gc.SHORTER))]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    skinny = generate(model, prompts, 8, linear="skinny")

    def same_model():
        after = model.state_dict()
        assert list(after) == list(before)
        for k, v in before.items():
            assert after[k].dtype == v.dtype and torch.equal(after[k].view(torch.uint8), v.view(torch.uint8)), k

    fp8 = Fp8DecodeWeights(model)
    same_model()
    held = {name: fp8.tensors[name] for name in fp8.names()}
    layers = len(model.layers)
    assert len(held) == 4 * layers + 1 and fp8.has_head
    assert fp8.nbytes == sum(q.numel() + 4 * s.numel() for q, s in held.values())
    assert fp8.nbytes == sum(p.numel() + 4 * p.shape[0] for n, p in model.named_parameters()
                             if n.endswith("_proj.weight") or n == "lm_head.weight")
    for name, (q, s) in held.items():
        w = model.get_submodule(name).weight
        assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape and s.shape == (w.shape[0],) and q.device == w.device
        d = fp8.dequantized(name)
        assert d.dtype == torch.bfloat16 and torch.equal(d.float(), q.float() * s[:, None])
    nohead = Fp8DecodeWeights(model, head=False)
    assert not nohead.has_head and len(nohead.names()) == 4 * layers
    assert nohead.nbytes == fp8.nbytes - sum(t.numel() * t.element_size() for t in fp8.head())

    first = generate(model, prompts, 8, linear="skinny-fp8", fp8=fp8)
    same_model()
    import dtg.models.quantized as qz

    def refuse(*a, **k):
        raise AssertionError("weights that were handed in were quantised again")

    monkeypatch.setattr(qz.ops, "quantize_fp8_rows", refuse)
    second = generate(model, prompts, 8, linear="skinny-fp8", fp8=fp8)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for name, (q, s) in held.items():
        assert fp8.tensors[name][0] is q and fp8.tensors[name][1] is s, f"{name} was replaced"
    built = generate(model, prompts, 8, linear="skinny-fp8")  # fp8=None: quantised for the call
    assert all(torch.equal(a, b) for a, b in zip(first, built))
    head_bf16 = generate(model, prompts, 8, linear="skinny-fp8", fp8=nohead)
    assert all(o.shape == (8,) for o in head_bf16)
    same_model()
    again = generate(model, prompts, 8, linear="skinny")
    assert all(torch.equal(a, b) for a, b in zip(skinny, again)), 'linear="skinny" changed'


def check_argument_errors(dev):
    import pytest

    model, _ = gc.models("llama", dev)
    fp8 = Fp8DecodeWeights(model)
    with pytest.raises(ValueError, match="at most 16"):
        generate(model, [torch.arange(3)] * 17, 2, linear="skinny-fp8", fp8=fp8)
    cache = KVCache(model.config, 17, 8, device=dev)
    with pytest.raises(ValueError, match="at most 16"):
        decode_step(model, torch.zeros(17, dtype=torch.long), cache, linear="skinny-fp8", fp8=fp8)
    cache = KVCache(model.config, 2, 8, device=dev)
    prefill(model, [torch.arange(3), torch.arange(2)], cache, fp8=fp8)
    with pytest.raises(ValueError, match="fp8="):
        decode_step(model, torch.zeros(2, dtype=torch.long), cache, linear="skinny-fp8")
    with pytest.raises(ValueError, match="skinny-fp8"):
        decode_step(model, torch.zeros(2, dtype=torch.long), cache, linear="skinny", fp8=fp8)
    with pytest.raises(ValueError, match="skinny-fp8"):
        generate(model, [torch.arange(3)], 2, linear="blas", fp8=fp8)
    with pytest.raises(ValueError, match="linear must be"):
        generate(model, [torch.arange(3)], 2, linear="fp8")
