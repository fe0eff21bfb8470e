"""Speculative decoding with exact-match verification: `generate(..., speculate=Speculative(...))`.

A step feeds every row its last accepted id and up to k - 1 drafted ids through one `extend_step` (one pass of
the model over n * k rows, `ops.decode_attention_multi` for the attention), computes the model's OWN id at each
of those positions -- argmax, or the fused sampler's draw with the row's stream and step = the index of the id
in the row's output -- and accepts a drafted id if and only if it equals the id the model produced for the
position before.  A row therefore emits the ids the plain loop would have emitted, a + 1 of them per step (a =
the accepted drafts): not ids "distributed like" them.  With linear="skinny" / "skinny-fp8" every kernel on the
path computes a row's result independently of the other rows of the launch (skinny GEMM, norms, RoPE, the
append, the verify attention against `decode_attn`, the sampler), so the ids equal, bit for bit, those of the
eager loop planned for the same length.  hipBLASLt (linear="blas"), the CPU operators and a sliding window
promise no such independence; there the ids agree up to rounding ties.

Launch plan: every verify pass is planned for one length, decode_bucket(longest prompt + max_new_tokens,
S_max), so rows that advance at different rates still share the plan of the plain loop they are compared with
(`generate(..., bucketed=True)` when the whole call stays inside one bucket).

Host traffic: one read per step (the n * k target ids) feeds the acceptance rule and the drafter, and one small
upload (tokens, q_valid, the draw counters) starts the next step.  The plain loop reads the device every 16
steps; this one trades that for more than one id per pass.

Rollback is positional: rejected keys stay in the cache past `cache.lens` and are overwritten by the next step.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from .. import ops
from ..ops.functional import SKINNY_MAX_M


class NgramDrafter:
    """Prompt lookup on the host: the longest suffix of a row's ids (ngram_max down to ngram_min tokens) that
    occurred earlier in the row, at its most recent earlier occurrence; proposes the ids that followed it."""

    def __init__(self, ngram_max: int = 3, ngram_min: int = 1):
        if not 1 <= int(ngram_min) <= int(ngram_max):
            raise ValueError(f"NgramDrafter: need 1 <= ngram_min <= ngram_max, got {ngram_min}, {ngram_max}")
        self.ngram_max, self.ngram_min = int(ngram_max), int(ngram_min)

    def propose(self, history: List[List[int]], want: List[int]) -> List[List[int]]:
        out = []
        for h, w in zip(history, want):
            found: List[int] = []
            if w > 0:
                for n in range(min(self.ngram_max, len(h) - 1), self.ngram_min - 1, -1):
                    tail = h[-n:]
                    i = next((i for i in range(len(h) - n - 1, -1, -1) if h[i:i + n] == tail), None)
                    if i is not None:
                        found = h[i + n:i + n + w]
                        break
            out.append(found)
        return out


class Speculative:
    """Settings of a speculative `generate` call.  `k`: tokens per verify pass and row (the last accepted id plus
    k - 1 drafted ids).  `drafter`: "ngram" (NgramDrafter(ngram_max, ngram_min)) or any object with
    `propose(history, want) -> drafts`: `history[i]` is row i's prompt and emitted ids, the result at most
    `want[i]` ids for row i (fewer or none is allowed; more are cut).  After a call `.stats` holds `steps`
    (verify passes), `proposed` and `accepted` (drafted ids) and `tokens` (ids emitted, all rows)."""

    def __init__(self, drafter="ngram", k: int = 4, ngram_max: int = 3, ngram_min: int = 1):
        if int(k) < 2:
            raise ValueError(f"Speculative: k must be at least 2 (the last accepted id plus one drafted id), got {k}")
        if drafter == "ngram":
            drafter = NgramDrafter(ngram_max, ngram_min)
        elif isinstance(drafter, str) or not callable(getattr(drafter, "propose", None)):
            raise ValueError(f"Speculative: drafter must be 'ngram' or an object with propose(history, want), got {drafter!r}")
        self.drafter, self.k = drafter, int(k)
        self.stats = dict(steps=0, proposed=0, accepted=0, tokens=0)


def check_speculate(spec, n, linear, graphed, sampler, temperature):
    """The refusals of generate(..., speculate=spec), all ValueError."""
    if not isinstance(spec, Speculative):
        raise ValueError(f"generate: speculate must be a Speculative or None, got {type(spec).__name__}")
    if spec.k < 2:
        raise ValueError(f"generate: speculate.k must be at least 2, got {spec.k}")
    if graphed:
        raise ValueError('generate: speculative decoding runs the eager loop only (decode="eager"); the verify step is '
                         "not captured into HIP graphs")
    if sampler == "torch" and not isinstance(temperature, (list, tuple, torch.Tensor)) and temperature > 0.0:
        raise ValueError('generate: speculative decoding with temperature > 0 needs sampler="fused" (its draw is a '
                         "function of seed, stream and step, so every drafted position can be verified)")
    if linear != "blas" and n * spec.k > SKINNY_MAX_M:
        raise ValueError(f'generate: linear="{linear}" with speculation verifies prompts x k = {n} x {spec.k} = '
                         f"{n * spec.k} rows per step, over the skinny limit of {SKINNY_MAX_M}")


def _accept(drafts: Sequence[int], target: Sequence[int]) -> int:
    """Leading drafted ids that equal the model's id of the position before them."""
    a = 0
    while a < len(drafts) and drafts[a] == target[a]:
        a += 1
    return a


def speculative_loop(model, prompts, max_new_tokens, spec, fused, seed, eos_token_id, s_max, linear, fp8,
                     kv_cache="bf16"):
    """generate()'s loop under `spec`; arguments as generate() has checked them (`fused`: the per-prompt host lists
    of the fused sampler's parameters, or None for argmax)."""
    from .generation import KVCache, decode_bucket, extend_step, prefill

    n, k = len(prompts), spec.k
    dev = model.embed_tokens.weight.device
    stats = spec.stats = dict(steps=0, proposed=0, accepted=0, tokens=0)
    plan_len = decode_bucket(max(p.numel() for p in prompts) + max_new_tokens, s_max)
    cache = KVCache(model.config, n, s_max, device=dev, dtype=model.embed_tokens.weight.dtype, kv_cache=kv_cache)
    if fused is not None:
        col = lambda name, reps: torch.tensor(fused[name], dtype=torch.int32 if name == "top_k" else torch.float32,  # noqa: E731
                                              device=dev).repeat_interleave(reps)
        stream = torch.arange(n, dtype=torch.int64, device=dev)

        def target(logits, reps, step):  # step: host list, one draw counter per logits row
            par = {name: col(name, reps) for name in fused}
            ids, _ = ops.sample_logits(logits, seed=int(seed), stream=stream.repeat_interleave(reps),
                                       step=torch.tensor(step, dtype=torch.int64, device=dev), **par)
            return ids
    else:
        def target(logits, reps, step):
            return logits.argmax(-1)

    history = [p.tolist() for p in prompts]
    base = [len(h) for h in history]          # prompt lengths
    out: List[List[int]] = [[] for _ in range(n)]
    done = [False] * n

    def emit(b, ids):
        for t in ids:
            out[b].append(t)
            history[b].append(t)
            if (eos_token_id is not None and t == int(eos_token_id)) or len(out[b]) >= max_new_tokens:
                done[b] = True
                break

    first = target(prefill(model, prompts, cache, fp8=fp8), 1, [0] * n).tolist()
    for b in range(n):
        emit(b, first[b:b + 1])
    while not all(done):
        # row b holds base[b] + len(out[b]) - 1 keys; its last id is not in the cache yet.  A pass over 1 + w tokens
        # can emit 1 + w ids and writes positions up to base + len(out) - 1 + w: both capped here
        want = [0 if done[b] else min(k - 1, max_new_tokens - len(out[b]) - 1, s_max - base[b] - len(out[b])) for b in range(n)]
        drafts = [list(d)[:w] for d, w in zip(spec.drafter.propose([list(h) for h in history], list(want)), want)]
        tokens = [[0] * k for _ in range(n)]
        for b in range(n):
            if not done[b]:
                tokens[b][:1 + len(drafts[b])] = [out[b][-1]] + drafts[b]
        q_valid = [0 if done[b] else 1 + len(drafts[b]) for b in range(n)]
        logits = extend_step(model, torch.tensor(tokens, dtype=torch.long, device=dev),
                             torch.tensor(q_valid, dtype=torch.long, device=dev), cache, linear=linear, plan_len=plan_len,
                             fp8=fp8)
        ids = target(logits, k, [len(out[b]) + t for b in range(n) for t in range(k)]).reshape(n, k).tolist()  # the host read
        adv = [0] * n
        for b in range(n):
            if done[b]:
                continue
            a = _accept(drafts[b], ids[b])
            stats["proposed"] += len(drafts[b])
            stats["accepted"] += a
            adv[b] = a + 1  # the last id and the accepted drafts are now keys of the row
            emit(b, ids[b][:a + 1])
        cache.lens += torch.tensor(adv, dtype=torch.int32, device=dev)
        cache.max_len = max(base[b] + len(out[b]) - 1 for b in range(n))
        stats["steps"] += 1
    stats["tokens"] = sum(len(o) for o in out)
    return [torch.tensor(o, dtype=torch.long) for o in out]
