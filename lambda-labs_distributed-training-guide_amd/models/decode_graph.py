"""HIP-graph capture of the KV-cache decode loop.

A decode step of a small model is a few hundred short kernels: the loop is bound by launch latency, not
by the GPU.  `GraphedDecode` records one whole step -- embedding of the last ids, the layers, the logits,
the choice of the next id, and the bookkeeping (`out`, `count`, `done`, `cache.lens`) -- into a HIP graph
(`torch.cuda.CUDAGraph` is hipGraph on ROCm) and replays it with one launch per token, as
`train/graph.py` does for a training step.

What makes the step replayable:
  * everything the step reads lives in static device tensors owned by this object: the last ids, the
    cache and its lengths, the position counter of `out`, the sampler's parameters, seed and draw
    counter, the EOS id.  Nothing in the body is built from host data;
  * the attention reads the true lengths from `cache.lens` on the device; only its launch plan needs a
    host length.  A graph is captured with the plan of a whole length bucket (`decode_bucket`: 256, 512,
    1024, ... capped at S_max), which the kernel tolerates (an over-long plan only leaves splits empty),
    so one graph serves every step of its bucket and a run captures at most log2(S_max / 256) + 1 graphs;
  * the host only replays, advances its own `cache.max_len`, and reads `done` every HOST_CHECK_EVERY
    steps, as the eager loop does.

The first `warmup` steps of a run that has no graph for its bucket yet are real eager steps on the
capture stream (lazy initialisation, allocator warm-up); the capture itself executes nothing, so the
cache is not advanced by it.  All work runs on one dedicated stream: the graph is a plain chain of
kernels.  With linear="skinny" (and "skinny-fp8", whose e4m3 weight copies are static device tensors
held by this object) every kernel of the step is this project's and deterministic, and the
captured loop returns the ids of `generate(..., decode="eager", bucketed=True)` bit for bit; with
linear="blas" hipBLASLt may choose other algorithms under capture and the two agree to rounding.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Tuple

import torch

from .. import ops
from . import generation as _g

_NO_EOS = -(2 ** 62)  # no id equals it


class GraphedDecode:
    """The captured decode loop of `model` for `n` sequences and a cache of `s_max` positions."""

    def __init__(self, model, n: int, s_max: int, linear: str = "skinny", warmup: int = 2, fp8=None,
                 kv_cache: str = "bf16"):
        _g._check_model(model)
        _g._check_linear(linear, n)
        dev = model.embed_tokens.weight.device
        if dev.type != "cuda":
            raise ValueError("GraphedDecode needs a GPU (HIP-graph capture)")
        self.model, self.n, self.s_max, self.linear, self.warmup = model, int(n), int(s_max), linear, int(warmup)
        self.fp8 = _g._check_fp8(model, linear, fp8, build=True)  # linear="skinny-fp8": static device tensors
        self.cache = _g.KVCache(model.config, self.n, self.s_max, device=dev, dtype=model.embed_tokens.weight.dtype,
                                kv_cache=kv_cache)  # "fp8": codes and scales are static device tensors too
        i64 = dict(dtype=torch.long, device=dev)
        self.rows = torch.arange(self.n, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(self.n, **i64)             # the ids the next step embeds
        self.out = torch.zeros(self.n, self.s_max, **i64)  # every id chosen, column = step
        self.pos = torch.zeros(1, **i64)                  # the column the next id goes to
        self.count = torch.zeros(self.n, **i64)           # ids kept per sequence
        self.done = torch.zeros(self.n, dtype=torch.bool, device=dev)
        self.eos = torch.full((1,), _NO_EOS, **i64)
        self.seed = torch.zeros(self.n, **i64)
        self.stream_ids = torch.arange(self.n, **i64)
        self.draw = torch.zeros(self.n, **i64)            # the sampler's step counter
        self.params = {"temperature": torch.zeros(self.n, dtype=torch.float32, device=dev),
                       "top_k": torch.zeros(self.n, dtype=torch.int32, device=dev),
                       "top_p": torch.ones(self.n, dtype=torch.float32, device=dev),
                       "min_p": torch.zeros(self.n, dtype=torch.float32, device=dev)}
        self._stream = torch.cuda.Stream(device=dev)
        self.graphs: Dict[Tuple[int, bool], torch.cuda.CUDAGraph] = {}  # (bucket, fused sampler) -> graph
        self.captures = self.replays = self.eager_steps = 0
        self.capture_seconds = 0.0

    # ------------------------------------------------------------------ one step
    def _choose(self, logits, fused: bool):
        """Next ids from `logits` and the bookkeeping of one token, all on the device."""
        if fused:
            nxt, _ = ops.sample_logits(logits, seed=self.seed, stream=self.stream_ids, step=self.draw, **self.params)
            self.draw += 1
        else:
            nxt = logits.argmax(-1)
        self.tok.copy_(nxt)
        self.out.index_copy_(1, self.pos, nxt[:, None])
        self.pos += 1
        self.count += (~self.done).long()
        self.done |= nxt == self.eos

    def _step(self, plan_len: int, fused: bool):
        self._choose(_g._decode_body(self.model, self.tok, self.cache, self.rows, plan_len, self.linear, self.fp8), fused)

    def _capture(self, bucket: int, fused: bool) -> torch.cuda.CUDAGraph:
        """Record one step planned for `bucket` (nothing executes; the first replay performs it)."""
        t0 = time.perf_counter()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._stream):
            self._step(bucket, fused)
        self.graphs[(bucket, fused)] = graph
        self.captures += 1
        self.capture_seconds += time.perf_counter() - t0
        return graph

    # ------------------------------------------------------------------ a whole generate() call
    def reset(self):
        """Empty the cache and the counters; the graphs stay."""
        self.cache.reset()
        for t in (self.pos, self.count, self.draw):
            t.zero_()
        self.done.zero_()

    @torch.no_grad()
    def run(self, prompts, max_new_tokens: int, fused: Optional[dict] = None, seed: int = 0,
            eos_token_id: Optional[int] = None, s_max: Optional[int] = None, linear: Optional[str] = None
            ) -> List[torch.Tensor]:
        """generate()'s loop: prefill, then `max_new_tokens` - 1 captured steps.  `fused`: the per-prompt
        host lists of the fused sampler's parameters (None = greedy argmax)."""
        if len(prompts) != self.n or (s_max is not None and int(s_max) != self.s_max) or \
                (linear is not None and linear != self.linear):
            raise ValueError(f"GraphedDecode: built for {self.n} prompts, S_max = {self.s_max}, linear = {self.linear!r}; "
                             f"got {len(prompts)}, {s_max}, {linear!r}")
        longest = max(int(p.numel()) for p in prompts)
        if longest + max_new_tokens > self.s_max:
            raise ValueError(f"GraphedDecode: prompt ({longest}) + max_new_tokens ({max_new_tokens}) exceeds S_max "
                             f"({self.s_max})")
        dev, cache, side = self.tok.device, self.cache, self._stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.reset()
            self.eos.fill_(_NO_EOS if eos_token_id is None else int(eos_token_id))
            use_fused = fused is not None
            if use_fused:
                for k, v in fused.items():
                    self.params[k].copy_(torch.tensor(v, dtype=self.params[k].dtype), non_blocking=False)
                self.seed.fill_((int(seed) + 2 ** 63) % 2 ** 64 - 2 ** 63)
            self._choose(_g.prefill(self.model, prompts, cache, fp8=self.fp8), use_fused)
            run_eager = 0  # eager steps of this run: the warm-up before its first capture
            for step in range(1, max_new_tokens):
                if eos_token_id is not None and step % _g.HOST_CHECK_EVERY == 0 and bool(self.done.all()):
                    break
                bucket = _g.decode_bucket(cache.max_len + 1, self.s_max)
                graph = self.graphs.get((bucket, use_fused))
                if graph is None and run_eager < self.warmup:
                    self._step(bucket, use_fused)
                    run_eager += 1
                    self.eager_steps += 1
                else:
                    if graph is None:
                        graph = self._capture(bucket, use_fused)
                    graph.replay()
                    self.replays += 1
                cache.max_len += 1
            out, count = self.out[:, :max_new_tokens].cpu(), self.count.tolist()
        torch.cuda.current_stream(dev).wait_stream(side)
        return [out[i, : count[i]].clone() for i in range(self.n)]
