"""Checks of speculative decoding (dtg.models.speculative, generate(..., speculate=...)), shared by
test_speculative_cpu.py and test_speculative_gpu.py.  Models are the tiny 2-layer ones of
tests/_generate_cases.py (the cycle head); prompts and S_MAX those of tests/_decode_graph_cases.py: lengths
250 / 247 in a cache of 512, so the fixed plan is the 512 bucket with two splits and the rows cross key 256.

The reference is written here from prefill + decode_step(plan_len=P) + argmax / ops.sample_logits with the
fixed P = decode_bucket(longest prompt + budget, s_max): the plain loop, never the code under test.  With
linear="skinny" / "skinny-fp8" on the GPU the speculative ids must equal it bit for bit whatever the drafter
proposes.  Where no row independence is promised (the CPU operators, a sliding window's tile origin) the ids
must agree up to the first position under the gap rule of _decode_graph_cases.gap_rule."""
import functools

import torch

import _decode_graph_cases as dc
import _generate_cases as gc
from dtg import ops
from dtg.models import Fp8DecodeWeights, Speculative
from dtg.models.generation import KVCache, decode_bucket, decode_step, generate, prefill

NEW, S_MAX = dc.NEW, dc.S_MAX
ODD_NEW = 23           # 22 ids after the prefill's: no multiple of k = 4
STRETCH, TAIL = 40, 8  # the repeating prompt: a stretch of the successor cycle, then its first TAIL ids again

MIXED = dict(temperature=(0.0, gc.SAMPLE_T), top_k=(0, 50), top_p=(1.0, 0.95), seed=5)   # one greedy, one sampled row
SAMPLED = dict(temperature=(gc.SAMPLE_T, gc.SAMPLE_T), top_k=(0, 0), top_p=(1.0, 1.0), seed=5)


def repeating_prompts(kind):
    """Random ids, then STRETCH ids of the successor cycle, then the stretch's first TAIL ids again: greedy
    decoding continues the stretch, and the n-gram drafter finds that continuation earlier in the row."""
    succ = gc.successor(kind)
    g = torch.Generator().manual_seed(700 + gc.MODELS[kind][2])
    out = []
    for n in dc.PROMPT_LENS:
        walk = [int(torch.randint(0, gc.VOCAB, (1,), generator=g))]
        for _ in range(STRETCH - 1):
            walk.append(int(succ[walk[-1]]))
        head = torch.randint(0, gc.VOCAB, (n - STRETCH - TAIL,), generator=g)
        out.append(torch.cat([head, torch.tensor(walk), torch.tensor(walk[:TAIL])]))
    return out


def prompts_of(kind, which):
    return dc.long_prompts(kind) if which == "long" else repeating_prompts(kind)


@functools.lru_cache(maxsize=None)
def fp8_weights(kind, dev):
    return Fp8DecodeWeights(gc.models(kind, dev)[0])


def _fp8(kind, dev, linear):
    return fp8_weights(kind, dev) if linear == "skinny-fp8" else None


@functools.lru_cache(maxsize=None)
def reference(kind, dev, linear, new=NEW, s_max=S_MAX, sampling=None, which="long"):
    """ids [n, new] (CPU) of the plain loop planned for P throughout; `sampling`: None = argmax, else a sorted
    tuple of (name, per-row values / seed) items for ops.sample_logits."""
    model, _ = gc.models(kind, dev)
    prompts = prompts_of(kind, which)
    n = len(prompts)
    fp8 = _fp8(kind, dev, linear)
    P = decode_bucket(max(len(p) for p in prompts) + new, s_max)
    cache = KVCache(model.config, n, s_max, device=dev)
    logits = prefill(model, prompts, cache, fp8=fp8)
    par = None
    if sampling is not None:
        s = dict(sampling)
        par = dict(seed=s["seed"], stream=torch.arange(n, dtype=torch.int64, device=dev),
                   temperature=torch.tensor(s["temperature"], dtype=torch.float32, device=dev),
                   top_k=torch.tensor(s["top_k"], dtype=torch.int32, device=dev),
                   top_p=torch.tensor(s["top_p"], dtype=torch.float32, device=dev))
    ids = []
    for step in range(new):
        if par is None:
            nxt = logits.argmax(-1)
        else:
            nxt, _ = ops.sample_logits(logits, step=torch.full((n,), step, dtype=torch.int64, device=dev), **par)
        ids.append(nxt.cpu())
        if step + 1 < new:
            logits = decode_step(model, nxt, cache, linear=linear, plan_len=P, fp8=fp8)
    return torch.stack(ids, 1)


class Oracle:
    """Proposes the ids `ids` [n, new] from where each row stands; `wrong_at` = j spoils the draft with index j
    of every proposal (j = 0: nothing is ever accepted)."""

    def __init__(self, ids, prompts, wrong_at=None):
        self.ids, self.base, self.wrong_at = ids.tolist(), [len(p) for p in prompts], wrong_at
        self.calls = 0

    def propose(self, history, want):
        self.calls += 1
        out = []
        for row, h, w, b in zip(self.ids, history, want, self.base):
            d = row[len(h) - b: len(h) - b + w]
            if self.wrong_at is not None and self.wrong_at < len(d):
                d[self.wrong_at] = (d[self.wrong_at] + 1) % gc.VOCAB
            out.append(d)
        return out


def _spec_run(kind, dev, linear, spec, new=NEW, s_max=S_MAX, sampling=None, which="long", **kw):
    model, _ = gc.models(kind, dev)
    if sampling is not None:
        s = dict(sampling)
        kw.update(sampler="fused", temperature=list(s["temperature"]), top_k=list(s["top_k"]), top_p=list(s["top_p"]),
                  seed=s["seed"])
    return generate(model, prompts_of(kind, which), new, s_max=s_max, linear=linear, fp8=_fp8(kind, dev, linear),
                    speculate=spec, **kw)


def _key(sampling):
    return None if sampling is None else tuple(sorted(sampling.items()))


def _same(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == torch.long and torch.equal(g, r), f"{what}: row {i} {g.tolist()} != plain loop {r.tolist()}"


def check_oracle(kind, dev, linear, k=4, new=NEW, s_max=S_MAX, sampling=None):
    """Everything proposed is right: the plain loop's ids, all drafts accepted, ceil((new - 1) / k) passes."""
    ref = reference(kind, dev, linear, new, s_max, _key(sampling))
    assert all(len(set(r.tolist())) >= new - 2 for r in ref) or sampling is not None, f"degenerate reference {ref.tolist()}"
    spec = Speculative(Oracle(ref, prompts_of(kind, "long")), k=k)
    _same(_spec_run(kind, dev, linear, spec, new, s_max, _key(sampling)), ref, f"{kind} oracle k={k}")
    st = spec.stats
    assert st["accepted"] == st["proposed"] > 0, st
    assert st["steps"] == -(-(new - 1) // k) and st["tokens"] == 2 * new, st
    assert st["proposed"] == 2 * (new - 1 - st["steps"]), st  # every pass emits one id that was not drafted


def check_wrong(kind, dev, linear, k=4, new=NEW, s_max=S_MAX, sampling=None):
    """A draft spoiled at index j, for every j: still the plain loop's ids; j accepted per full proposal.  j = 0 is
    the drafter that is always wrong: nothing accepted, one id per pass."""
    ref = reference(kind, dev, linear, new, s_max, _key(sampling))
    for j in range(k - 1):
        spec = Speculative(Oracle(ref, prompts_of(kind, "long"), wrong_at=j), k=k)
        _same(_spec_run(kind, dev, linear, spec, new, s_max, _key(sampling)), ref, f"{kind} wrong at {j}, k={k}")
        st = spec.stats
        assert st["tokens"] == 2 * new and st["accepted"] <= st["steps"] * 2 * j, st
        if j == 0:
            assert st["accepted"] == 0 and st["steps"] == new - 1 and st["proposed"] > 0, st
        else:
            assert 0 < st["accepted"] < st["proposed"], st


def check_eos(kind, dev, linear, k=4):
    """An EOS id that stops the rows at different steps: every row is the free run cut after its first EOS."""
    free = reference(kind, dev, linear, NEW, S_MAX, _key(SAMPLED))

    def first(seq, tok):
        hit = (seq == tok).nonzero()
        return int(hit[0]) + 1 if len(hit) else NEW

    eos = next((int(t) for t in free[0][:-1] if first(free[0], t) != first(free[1], t)), None)
    assert eos is not None, "no id stops the two sequences at different steps"
    for wrong_at in (None, 1):
        spec = Speculative(Oracle(free, prompts_of(kind, "long"), wrong_at=wrong_at), k=k)
        got = _spec_run(kind, dev, linear, spec, sampling=_key(SAMPLED), eos_token_id=eos)
        _same(got, [f[: first(f, eos)] for f in free], f"{kind} eos {eos}")
        assert spec.stats["tokens"] == sum(first(f, eos) for f in free)


def check_ngram(kind, dev, linear, k=4):
    """The built-in prompt-lookup drafter on a prompt whose tail repeats an earlier stretch: the plain loop's ids,
    and some of its drafts are accepted."""
    ref = reference(kind, dev, linear, which="repeat")
    spec = Speculative("ngram", k=k)
    _same(_spec_run(kind, dev, linear, spec, which="repeat"), ref, f"{kind} ngram")
    st = spec.stats
    assert st["accepted"] > 0 and st["steps"] < NEW - 1 and st["tokens"] == 2 * NEW, st


def check_up_to_gaps(kind, dev, linear="blas"):
    """No bitwise promise (CPU operators, a sliding window): against the plain loop's ids the speculative ids may
    differ first only at a position under the gap rule, for an oracle, a spoiled and an n-gram proposal."""
    ref = reference(kind, dev, linear)
    sure, share = dc.gap_rule(kind, tuple(tuple(r.tolist()) for r in ref))
    assert share <= gc.MAX_EXCLUDED, f"{kind}: {share} of the positions excluded by the gap rule"
    for drafter in (Oracle(ref, prompts_of(kind, "long")), Oracle(ref, prompts_of(kind, "long"), wrong_at=1), "ngram"):
        spec = Speculative(drafter, k=4)
        got = _spec_run(kind, dev, linear, spec)
        for i, g in enumerate(got):
            assert g.shape == (NEW,)
            diff = (g != ref[i]).nonzero().flatten()
            if len(diff):
                assert not sure[i, int(diff[0])], f"{kind}: row {i} differs at the sure position {int(diff[0])}"
        assert spec.stats["tokens"] == 2 * NEW and 1 <= spec.stats["steps"] <= NEW - 1


def check_errors(dev):
    import pytest

    model, _ = gc.models("llama", dev)
    prompts = [p[:12] for p in dc.long_prompts("llama")]
    with pytest.raises(ValueError, match='sampler="fused"'):
        generate(model, prompts, 4, temperature=0.7, speculate=Speculative(k=2))
    with pytest.raises(ValueError, match="eager"):
        generate(model, prompts, 4, decode="graph", speculate=Speculative(k=2))
    with pytest.raises(ValueError, match="k must be at least 2"):
        Speculative(k=1)
    with pytest.raises(ValueError, match="drafter"):
        Speculative(drafter="medusa")
    with pytest.raises(ValueError, match="skinny limit"):
        generate(model, prompts, 4, linear="skinny", speculate=Speculative(k=9))
    with pytest.raises(ValueError, match="Speculative"):
        generate(model, prompts, 4, speculate="ngram")


def check_none_is_the_plain_loop(dev):
    """speculate=None: an existing call returns what prefill + decode_step + argmax return."""
    model, _ = gc.models("llama", dev)
    prompts = [p[:12] for p in dc.long_prompts("llama")]
    got = generate(model, prompts, 8, speculate=None)
    cache = KVCache(model.config, 2, 12 + 8, device=dev)
    nxt = prefill(model, prompts, cache).argmax(-1)
    manual = [nxt.cpu()]
    for _ in range(7):
        nxt = decode_step(model, nxt, cache).argmax(-1)
        manual.append(nxt.cpu())
    assert torch.equal(torch.stack(got), torch.stack(manual, 1))
    assert all(torch.equal(a, b) for a, b in zip(got, generate(model, prompts, 8)))


def check_ngram_drafter():
    from dtg.models import NgramDrafter

    d = NgramDrafter(3, 1)
    # the longest suffix wins: (1, 2, 3) at index 0 -> what followed it
    assert d.propose([[1, 2, 3, 9, 8, 1, 2, 3]], [2]) == [[9, 8]]
    # the most recent earlier occurrence: (5,) at index 2, not index 0
    assert d.propose([[5, 1, 5, 2, 5]], [3]) == [[2, 5]]
    # no earlier occurrence, nothing wanted, a one-id row
    assert d.propose([[1, 2, 3], [1, 1], [4]], [3, 0, 2]) == [[], [], []]
    # ngram_min 2: a single matching id is not enough
    assert NgramDrafter(3, 2).propose([[5, 1, 5]], [2]) == [[]]
    assert NgramDrafter(3, 2).propose([[5, 1, 7, 5, 1]], [2]) == [[7, 5]]
