"""Checks of the skinny-GEMM decode step and of the captured decode loop, shared by
test_decode_graph_cpu.py and test_decode_graph_gpu.py.  Models, sequences and measures are those of
tests/_generate_cases.py (tiny 2-layer models of the four kinds, the cycle head)."""
import functools

import torch

import _generate_cases as gc
from dtg.models.decode_graph import GraphedDecode
from dtg.models.generation import KVCache, decode_bucket, decode_step, generate, prefill

PROMPT_LENS = (250, 247)   # 24 new tokens cross the 256 bucket's edge: lengths 251 ... 273
S_MAX = 512                # the second bucket is a full 512: 2 splits of 256 keys, the shorter row's second one empty at first
NEW = gc.NEW_TOKENS


def long_prompts(kind):
    g = torch.Generator().manual_seed(300 + gc.MODELS[kind][2])
    return [torch.randint(0, gc.VOCAB, (n,), generator=g) for n in PROMPT_LENS]


def check_teacher_forced_skinny(kind, dev):
    """gc.check_teacher_forced with the decode steps' projections in ops.skinny_linear: the cached path
    within 2 * e_full of the f32 model, e_full being the error of the existing bf16 full forward."""
    model, ref = gc.models(kind, dev)
    seqs = gc.sequences(kind)
    pre = [gc.PREFIX, gc.PREFIX - gc.SHORTER]
    cache = KVCache(model.config, 2, gc.SEQ, device=dev)
    got = [[lg] for lg in prefill(model, [s[:p] for s, p in zip(seqs, pre)], cache).float().cpu()]
    for t in range(gc.STEPS):
        tok = torch.stack([s[p + t] for s, p in zip(seqs, pre)])
        lg = decode_step(model, tok, cache, linear="skinny").float().cpu()
        for i in range(2):
            got[i].append(lg[i])
    e_full = e_cached = 0.0
    for s, p, g in zip(seqs, pre, got):
        r = gc.full_logits(ref, s)[p - 1: p + gc.STEPS]
        e_full = max(e_full, (gc.full_logits(model, s)[p - 1: p + gc.STEPS] - r).abs().max().item())
        e_cached = max(e_cached, (torch.stack(g) - r).abs().max().item())
    print(f"[decode-graph] {kind} teacher-forced skinny: e_full {e_full:.5f}, e_cached {e_cached:.5f} "
          f"(allowed {2 * e_full:.5f})")
    assert e_full > 0
    assert e_cached <= 2 * e_full, f"{kind}: skinny cached path error {e_cached} > 2 * {e_full}"


@functools.lru_cache(maxsize=None)
def gap_rule(kind, ids_key):
    """(sure [n, NEW] bool, excluded share): where the f32 reference's top-1 / top-2 gap exceeds 4 * e_full on
    the sequences prompt + ids (the measure of gc.check_greedy), computed on the CPU."""
    model, ref = gc.models(kind, "cpu")
    sure, excluded = [], 0
    for pr, out in zip(long_prompts(kind), ids_key):
        ids = torch.cat([pr, torch.tensor(out)])
        sl = slice(len(pr) - 1, len(ids) - 1)
        r, f = gc.full_logits(ref, ids)[sl], gc.full_logits(model, ids)[sl]
        e_full = (f - r).abs().max().item()
        top = r.topk(2, -1).values
        s = (top[:, 0] - top[:, 1]) > 4 * e_full
        sure.append(s)
        excluded += int((~s).sum())
    return torch.stack(sure), excluded / (len(ids_key) * NEW)


def check_reference_gaps(kind):
    """The cycle head keeps the reference's gaps clear of the rule at 250-token prompts too."""
    model, _ = gc.models(kind, "cpu")
    outs = generate(model, long_prompts(kind), NEW, s_max=S_MAX)
    _, share = gap_rule(kind, tuple(tuple(o.tolist()) for o in outs))
    print(f"[decode-graph] {kind}: {share:.3f} of the positions under the gap rule at {PROMPT_LENS}-token prompts")
    assert share <= gc.MAX_EXCLUDED


def _pair(model, prompts, gd, **kw):
    graph = generate(model, prompts, NEW, s_max=S_MAX, linear=gd.linear, decode=gd, **kw)
    eager = generate(model, prompts, NEW, s_max=S_MAX, linear=gd.linear, decode="eager", bucketed=True, **kw)
    return graph, eager


def check_graph_bitwise(kind, dev):
    """linear="skinny": the captured loop returns the bucketed eager loop's ids bit for bit -- greedy, under
    the fused sampler with one greedy and one sampled row, and with an EOS id that stops the rows apart."""
    model, _ = gc.models(kind, dev)
    prompts = long_prompts(kind)
    gd = GraphedDecode(model, 2, S_MAX, linear="skinny")
    graph, eager = _pair(model, prompts, gd)
    assert gd.captures == 2 and gd.replays >= 18, (gd.captures, gd.replays, gd.eager_steps)
    assert gd.eager_steps == gd.warmup
    for g, e in zip(graph, eager):
        assert g.shape == (NEW,) and torch.equal(g, e), (g.tolist(), e.tolist())
        assert len(set(g.tolist())) >= NEW - 2, f"degenerate continuation {g.tolist()}"

    fused = dict(sampler="fused", temperature=[0.0, gc.SAMPLE_T], top_k=[0, 50], top_p=[1.0, 0.95], seed=5)
    graph, eager = _pair(model, prompts, gd, **fused)
    assert gd.captures == 4  # the fused sampler's step is another graph per bucket
    for g, e in zip(graph, eager):
        assert torch.equal(g, e), (g.tolist(), e.tolist())
    assert torch.equal(graph[0], _pair(model, prompts, gd)[0][0]), "the greedy row depends on its neighbour"

    free = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny", decode="eager", bucketed=True,
                    sampler="fused", temperature=gc.SAMPLE_T, seed=5)

    def first(seq, tok):
        hit = (seq == tok).nonzero()
        return int(hit[0]) + 1 if len(hit) else NEW

    eos = next((int(t) for t in free[0][:-1] if first(free[0], t) != first(free[1], t)), None)
    assert eos is not None, "no id stops the two sequences at different steps"
    graph, eager = _pair(model, prompts, gd, sampler="fused", temperature=gc.SAMPLE_T, seed=5, eos_token_id=eos)
    for f, g, e in zip(free, graph, eager):
        assert torch.equal(g, e) and torch.equal(g, f[: first(f, eos)]), (g.tolist(), e.tolist(), f.tolist())
    assert gd.captures == 4, "an EOS id or new sampling parameters must not re-capture"


def check_graph_blas(kind, dev):
    """linear="blas": hipBLASLt may pick other algorithms under capture, so the ids agree only where the f32
    reference's gap exceeds 4 * e_full (at most MAX_EXCLUDED of the positions excluded)."""
    model, _ = gc.models(kind, dev)
    prompts = long_prompts(kind)
    gd = GraphedDecode(model, 2, S_MAX, linear="blas")
    graph, eager = _pair(model, prompts, gd)
    assert gd.captures == 2 and gd.replays >= 18
    sure, share = gap_rule(kind, tuple(tuple(o.tolist()) for o in eager))
    assert share <= gc.MAX_EXCLUDED, f"{kind}: {share} of the positions excluded by the gap rule"
    g, e = torch.stack(graph), torch.stack(eager)
    # ids after a first disagreement follow another sequence: compare up to it, and it must be unsure
    for i in range(2):
        diff = (g[i] != e[i]).nonzero().flatten()
        if len(diff):
            assert not sure[i, int(diff[0])], f"{kind}: row {i} differs at the sure position {int(diff[0])}"


def check_graph_reuse(kind, dev):
    """A second generate() call on the same GraphedDecode resets the counters, reuses cache and graphs (no
    capture, no warm-up) and returns the first call's ids."""
    model, _ = gc.models(kind, dev)
    prompts = long_prompts(kind)
    gd = GraphedDecode(model, 2, S_MAX, linear="skinny")
    a = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny", decode=gd)
    caps, reps, eag = gd.captures, gd.replays, gd.eager_steps
    b = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny", decode=gd)
    assert gd.captures == caps == 2 and gd.eager_steps == eag and gd.replays == reps + NEW - 1
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = generate(model, prompts, NEW, s_max=S_MAX, linear="skinny", decode="graph")  # a fresh object
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def bucket_properties():
    for s_max in (1, 100, 256, 257, 1000, 4096, 5000, 131072):
        prev, seen = 0, set()
        for length in list(range(0, min(s_max, 3000) + 1)) + [s_max]:
            b = decode_bucket(length, s_max)
            assert length <= b <= s_max and b >= prev
            prev = b
            seen.add(b)
        limit = max(0, (max(s_max, 256) - 1) // 256).bit_length() + 1  # ceil(log2(s_max / 256)) + 1
        assert len(seen) <= limit, (s_max, sorted(seen), limit)
