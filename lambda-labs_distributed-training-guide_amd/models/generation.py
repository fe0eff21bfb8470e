"""KV-cache generation for the Llama-family models (llama, mistral, qwen2, qwen3).

`prefill` runs the packed prompts through the layers exactly as the packed training path does
(token-major, cu_seqlens / position ids restarting per prompt, varlen flash attention) while
`ops.kv_cache_append` ropes q / k and fills the cache; `decode_step` runs one token per sequence
through `ops.kv_cache_append` and the split-KV `ops.decode_attention`.  The norms, projections and
MLP are the training ops, unchanged.  Logits are computed for the last token of each sequence only:
no [T, V] tensor exists.

Sampling: `generate(..., sampler="torch")` (default) keeps `sample_next`, a chain of torch ops drawn
from one generator shared by the batch; `sampler="fused"` ends every step in the single-launch
`ops.sample_logits` (top-k, top-p, min-p, per-prompt parameters, a counter-based draw per sequence; see
related-topics/sampling/README.md).  The two draw different ids for one seed.

Not covered (ValueError): GPT-2, and models built with a tensor-, context- or Ulysses-parallel group.
Mistral's sliding window is passed to both attention paths; the cache keeps the full length (no
ring buffer).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import ops
from ..ops.functional import SKINNY_MAX_M
from .gpt2 import GPT2LMHeadModel
from .llama import LlamaForCausalLM

HOST_CHECK_EVERY = 16  # steps between host reads of the device-side done mask


def _check_model(model):
    if isinstance(model, GPT2LMHeadModel):
        raise ValueError("generate: GPT-2 is not supported yet (Llama-family models only)")
    if not isinstance(model, LlamaForCausalLM):
        raise ValueError(f"generate: unsupported model type {type(model).__name__}")
    if model.tp.group is not None or model.cp_group is not None or model.sp_group is not None:
        raise ValueError("generate: models built with a tensor-, context- or Ulysses-parallel group are not supported yet")


class KVCache:
    """Per-layer K / V tensors [rows_max, nkv, S_max, D] (head-major: one kv head's keys are contiguous
    along the sequence), the device-side length of every row, and a host upper bound of those lengths
    for the decode kernel's launch plan.

    kv_cache="fp8": K / V are float8_e4m3fn with one f32 power-of-two scale per (row, kv head, position) in the
    lists `k_scale` / `v_scale` ([rows_max, nkv, S_max] per layer; None for "bf16"): (D + 4) / (2 D) of the bf16
    cache's bytes.  `ops.kv_cache_append` quantises what it writes and the decode attention reads the codes; the
    cache is exactly some bf16 cache, and prompt and decode steps attend the same quantised values."""

    def __init__(self, cfg, rows_max: int, s_max: int, device=None, dtype=torch.bfloat16, kv_cache: str = "bf16"):
        if rows_max < 1 or s_max < 1:
            raise ValueError(f"KVCache: rows_max ({rows_max}) and S_max ({s_max}) must be positive")
        _check_kv_cache(kv_cache)
        self.rows_max, self.s_max, self.kv_cache = int(rows_max), int(s_max), kv_cache
        shape = (self.rows_max, cfg.num_key_value_heads, self.s_max, cfg.head_dim)
        layers = range(cfg.num_hidden_layers)
        if kv_cache == "fp8":
            def codes():
                return torch.zeros(shape, device=device, dtype=torch.uint8).view(torch.float8_e4m3fn)

            self.k, self.v = [codes() for _ in layers], [codes() for _ in layers]
            self.k_scale = [torch.ones(shape[:3], device=device, dtype=torch.float32) for _ in layers]
            self.v_scale = [torch.ones(shape[:3], device=device, dtype=torch.float32) for _ in layers]
        else:
            self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in layers]
            self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in layers]
            self.k_scale = self.v_scale = None
        self.lens = torch.zeros(self.rows_max, dtype=torch.int32, device=device)
        self.max_len = 0  # host: no row is longer than this

    @property
    def nbytes(self) -> int:
        """Bytes of the K / V tensors and, for an FP8 cache, their scales."""
        ts = self.k + self.v + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in ts)

    def scales(self, i):
        """The keyword arguments of layer i's scales for the cache ops (empty for a bf16 cache)."""
        return {} if self.k_scale is None else dict(k_scale=self.k_scale[i], v_scale=self.v_scale[i])

    def reset(self):
        self.lens.zero_()
        self.max_len = 0


LINEAR_MODES = ("blas", "skinny", "skinny-fp8")
KV_CACHE_MODES = ("bf16", "fp8")


def _check_kv_cache(kv_cache):
    if kv_cache not in KV_CACHE_MODES:
        raise ValueError(f"kv_cache must be one of {KV_CACHE_MODES}, got {kv_cache!r}")


def _check_linear(linear, n=None):
    if linear not in LINEAR_MODES:
        raise ValueError(f"linear must be one of {LINEAR_MODES}, got {linear!r}")
    if linear != "blas" and n is not None and n > SKINNY_MAX_M:
        raise ValueError(f'linear="{linear}" decodes at most {SKINNY_MAX_M} sequences per step, got {n}')


def _check_fp8(model, linear, fp8, build=False):
    """The FP8 weight copies of a linear="skinny-fp8" call: `fp8` as given, built when `build` allows it."""
    if linear != "skinny-fp8":
        if fp8 is not None:
            raise ValueError(f'fp8 weights were given with linear={linear!r}; they need linear="skinny-fp8"')
        return None
    if fp8 is None:
        if not build:
            raise ValueError('linear="skinny-fp8" needs fp8=Fp8DecodeWeights(model)')
        from .quantized import Fp8DecodeWeights

        return Fp8DecodeWeights(model)
    fp8.check(model)
    return fp8


def _projections(model, linear, fp8):
    """The matrix products of one pass through the model, chosen once per call: proj(x, i, name, w, bias) is
    the product with layer i's matrix `w`, which Fp8DecodeWeights calls `name`; mlp(x, i, m) the SwiGLU MLP `m`
    of layer i; head(h) the LM head.  linear="skinny" (a decode step of at most 16 rows): ops.skinny_linear
    instead of hipBLASLt, gate_up with its SwiGLU epilogue; linear="skinny-fp8": ops.skinny_linear_fp8 on the
    e4m3 copies `fp8` (models/quantized.py; the bf16 kernel for a head without a copy).  linear="blas" with
    `fp8` is the prefill of an FP8 run: hipBLASLt on the bf16 matrices the copies stand for (`fp8.dequantized`,
    made where they are used and dropped), so the keys and values the prompt leaves in the cache belong to the
    same quantised model as the decode steps that read them."""
    fp8_head = fp8 is not None and fp8.has_head

    if linear == "blas":
        def proj(x, i, name, w, bias=None):
            w = w if fp8 is None else fp8.dequantized(f"layers.{i}.{name}")
            return ops.linear(x, w, None if bias is None else bias.view(-1))

        def mlp(x, i, m):
            if fp8 is None:
                return m(x)
            return ops.swiglu_mlp(x, fp8.dequantized(f"layers.{i}.mlp.gate_up_proj"), fp8.dequantized(f"layers.{i}.mlp.down_proj"))

        def head(h):
            return ops.linear(h, fp8.dequantized("lm_head") if fp8_head else model.lm_head_weight())
    else:
        def proj(x, i, name, w, bias=None, act=None):
            if fp8 is None:
                return ops.skinny_linear(x, w, bias, act)
            return ops.skinny_linear_fp8(x, *fp8.layer(i, name), bias, act)

        def mlp(x, i, m):
            h = proj(x, i, "mlp.gate_up_proj", m.gate_up_proj.weight, act="swiglu")
            return proj(h, i, "mlp.down_proj", m.down_proj.weight)

        def head(h):
            return ops.skinny_linear_fp8(h, *fp8.head()) if fp8_head else ops.skinny_linear(h, model.lm_head_weight())
    return proj, mlp, head


def _run_layers(model, x, append_and_attend, linear="blas", fp8=None):
    """The decoder stack around a caller-supplied attention (qkv -> attention output); see _projections."""
    proj, mlp, _ = _projections(model, linear, fp8)
    res = None
    for i, layer in enumerate(model.layers):
        if res is None:
            n, res = ops.rms_norm(x, layer.input_layernorm.weight, layer.eps), x
        else:
            n, res = ops.add_rms_norm(x, res, layer.input_layernorm.weight, layer.eps)
        attn = layer.self_attn
        qkv = proj(n, i, "self_attn.qkv_proj", attn.qkv_proj.weight, getattr(attn.qkv_proj, "bias", None))
        a = proj(append_and_attend(i, attn, qkv), i, "self_attn.o_proj", attn.o_proj.weight)
        n2, res = ops.add_rms_norm(a, res, layer.post_attention_layernorm.weight, layer.eps)
        x = mlp(n2, i, layer.mlp)
    return x, res


def _append(attn, qkv, cache, i, cos, sin, pos, rows, pos_max, rope_pos=None):
    """RoPE (after the per-head norm for Qwen3, whose fused pass ropes itself) and the cache write.
    `pos_max`: the host's largest position of the call, checked by the op (rows were checked by _rows).
    `rope_pos`: in-table positions for Qwen3's pass where `pos` marks tokens to skip with -1 (extend_step);
    the append itself skips them."""
    if attn.qk_norm:
        qkv = ops.qk_norm_rope(qkv, attn.q_norm.weight, attn.k_norm.weight, attn.eps, attn.nq, attn.nkv, attn.d,
                               cos, sin, pos if rope_pos is None else rope_pos)
        return ops.kv_cache_append(qkv, cache.k[i], cache.v[i], pos, rows, attn.nq, attn.nkv, attn.d, pos_max=pos_max,
                                   **cache.scales(i))
    return ops.kv_cache_append(qkv, cache.k[i], cache.v[i], pos, rows, attn.nq, attn.nkv, attn.d, cos, sin,
                               pos_max=pos_max, **cache.scales(i))


def _last_logits(model, x, res, linear="blas", fp8=None):
    h, _ = ops.add_rms_norm(x, res, model.norm.weight, model.config.rms_norm_eps)
    return _projections(model, linear, fp8)[2](h)


def _rows(cache, n, rows, device):
    if rows is None:
        rows_host = list(range(n))
    else:
        rows_host = [int(r) for r in rows]
    if len(rows_host) != n or len(set(rows_host)) != n or any(not 0 <= r < cache.rows_max for r in rows_host):
        raise ValueError(f"cache rows {rows_host} must be {n} distinct rows in [0, {cache.rows_max})")
    return torch.tensor(rows_host, dtype=torch.int32, device=device)


@torch.no_grad()
def prefill(model, prompts: Sequence[torch.Tensor], cache: KVCache, rows: Optional[Sequence[int]] = None, fp8=None):
    """Run the prompts (1-D id tensors of any lengths >= 1) packed token-major, fill cache rows `rows`
    (default 0..n-1) from position 0 and return the logits [n, V] of each prompt's last token.

    `fp8` (an `Fp8DecodeWeights` of this model): the prefill of a linear="skinny-fp8" run.  The GEMMs stay
    hipBLASLt in bf16, on the matrices the e4m3 copies stand for instead of the model's own, so prompt and
    decode steps see one and the same (quantised) model."""
    _check_model(model)
    if fp8 is not None:
        fp8.check(model)
    lens = [int(p.numel()) for p in prompts]
    if not lens or min(lens) < 1:
        raise ValueError("prefill: every prompt needs at least one token")
    if max(lens) > cache.s_max:
        raise ValueError(f"prefill: a prompt of {max(lens)} tokens does not fit the cache (S_max = {cache.s_max})")
    dev = cache.lens.device
    rows_t = _rows(cache, len(lens), rows, dev)
    ids = torch.cat([p.reshape(-1) for p in prompts]).to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    pos = torch.cat([torch.arange(n, dtype=torch.long) for n in lens]).to(dev)
    cu = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    tok_rows = torch.repeat_interleave(rows_t, lens_t.long(), output_size=sum(lens))
    cos, sin = model._rope_tables(cache.s_max, dev)
    max_seqlen = max(lens)

    def attend(i, attn, qkv):
        qkv = _append(attn, qkv, cache, i, cos, sin, pos, tok_rows, max_seqlen - 1)
        return ops.attention(qkv, attn.nq, attn.nkv, attn.d, cu, max_seqlen, window=attn.window)  # q, k roped already

    x, res = _run_layers(model, ops.embedding(ids, model.embed_tokens.weight), attend, "blas", fp8)
    last = (cu[1:] - 1).long()
    cache.lens[rows_t.long()] = lens_t
    cache.max_len = max(cache.max_len, max_seqlen)
    return _last_logits(model, x[last], res[last], "blas", fp8)


def _decode_body(model, tokens, cache, rows_t, plan_len, linear, fp8=None):
    """One decode step on device tensors only (`tokens` [n] ids, `rows_t` [n] int32 cache rows): nothing is
    built from host data and nothing is read back, so a HIP graph can record it.  `plan_len` is the host
    length of the attention's launch plan and of the append's position check.  Advances cache.lens, not the
    host's cache.max_len; returns the logits [n, V]."""
    dev = cache.lens.device
    pos = cache.lens[rows_t.long()].long()
    new_lens = (pos + 1).to(torch.int32)
    cos, sin = model._rope_tables(cache.s_max, dev)

    def attend(i, attn, qkv):
        qkv = _append(attn, qkv, cache, i, cos, sin, pos, rows_t, plan_len - 1)
        return ops.decode_attention(qkv, cache.k[i], cache.v[i], rows_t, new_lens, attn.nq, attn.nkv, attn.d, plan_len,
                                    window=attn.window, **cache.scales(i))

    x, res = _run_layers(model, ops.embedding(tokens, model.embed_tokens.weight), attend, linear, fp8)
    cache.lens[rows_t.long()] = new_lens
    return _last_logits(model, x, res, linear, fp8)


@torch.no_grad()
def decode_step(model, tokens: torch.Tensor, cache: KVCache, rows: Optional[Sequence[int]] = None,
                linear: str = "blas", plan_len: Optional[int] = None, fp8=None):
    """One new token per active sequence (`tokens` [n], for cache rows `rows`, default 0..n-1): appends
    it at the row's current length and returns the next-token logits [n, V].

    linear="skinny": the five projections of the step (qkv, o, gate_up with its SwiGLU, down, LM head)
    run in `ops.skinny_linear` (at most 16 sequences); linear="skinny-fp8": in `ops.skinny_linear_fp8` on
    the e4m3 weight copies `fp8` (an `Fp8DecodeWeights` of this model, required).  `plan_len`: the host length the attention's
    launch plan is made for, cache.max_len + 1 <= plan_len <= S_max (default cache.max_len + 1, the
    tightest); a captured step is planned for its whole length bucket, and an eager step given the same
    `plan_len` runs the same launches."""
    _check_model(model)
    if cache.max_len + 1 > cache.s_max:
        raise ValueError(f"decode_step: the cache is full (S_max = {cache.s_max})")
    dev = cache.lens.device
    tokens = tokens.reshape(-1).to(dev)
    _check_linear(linear, tokens.numel())
    fp8 = _check_fp8(model, linear, fp8)
    max_len = cache.max_len + 1
    if plan_len is None:
        plan_len = max_len
    if not max_len <= int(plan_len) <= cache.s_max:
        raise ValueError(f"decode_step: plan_len {plan_len} outside [cache.max_len + 1 = {max_len}, S_max = {cache.s_max}]")
    rows_t = _rows(cache, tokens.numel(), rows, dev)
    logits = _decode_body(model, tokens, cache, rows_t, int(plan_len), linear, fp8)
    cache.max_len = max_len
    return logits


@torch.no_grad()
def extend_step(model, tokens: torch.Tensor, q_valid: torch.Tensor, cache: KVCache, rows: Optional[Sequence[int]] = None,
                linear: str = "blas", plan_len: Optional[int] = None, fp8=None):
    """Up to Q new tokens per active sequence in one pass (`tokens` [n, Q] ids, `q_valid` [n]: how many of a
    row's Q are real): the verify pass of speculative decoding.  Token t < q_valid[b] of row b is appended at
    position cache.lens[b] + t and attends the keys up to and including its own (`ops.decode_attention_multi`
    with lens = pos + 1); a token t >= q_valid[b] is written nowhere (pos = -1) and attends nothing (len = 0), its
    logits mean nothing.  Returns the logits [n * Q, V], row b * Q + t = the prediction after token t.

    Built from device tensors only (`q_valid` is not read on the host).  Does NOT advance cache.lens or
    cache.max_len: the caller does, by the number of tokens it accepts; what it rejects stays past lens and is
    overwritten later.  `plan_len` as in `decode_step` (default: cache.max_len + Q, capped at S_max); it must
    cover the largest length the pass attends.  linear="skinny" / "skinny-fp8" run all n * Q rows in one
    skinny GEMM, so n * Q may not exceed its row limit."""
    _check_model(model)
    dev = cache.lens.device
    if tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError(f"extend_step: tokens must be [n, Q] with Q >= 1, got {tuple(tokens.shape)}")
    n, Q = tokens.shape
    if q_valid.dim() != 1 or q_valid.numel() != n:
        raise ValueError(f"extend_step: q_valid must be [{n}], got {tuple(q_valid.shape)}")
    _check_linear(linear)
    if linear != "blas" and n * Q > SKINNY_MAX_M:
        raise ValueError(f'extend_step: linear="{linear}" takes at most {SKINNY_MAX_M} rows per pass, got '
                         f"{n} sequences x {Q} tokens = {n * Q}")
    fp8 = _check_fp8(model, linear, fp8)
    if cache.max_len + 1 > cache.s_max:
        raise ValueError(f"extend_step: the cache is full (S_max = {cache.s_max})")
    if plan_len is None:
        plan_len = min(cache.max_len + Q, cache.s_max)
    plan_len = int(plan_len)
    if not cache.max_len + 1 <= plan_len <= cache.s_max:
        raise ValueError(f"extend_step: plan_len {plan_len} outside [cache.max_len + 1 = {cache.max_len + 1}, "
                         f"S_max = {cache.s_max}]")
    rows_t = _rows(cache, n, rows, dev)
    t = torch.arange(Q, device=dev)
    base = cache.lens[rows_t.long()].long()
    live = t[None] < q_valid.to(dev)[:, None]
    pos = torch.where(live, base[:, None] + t[None], torch.full((), -1, dtype=torch.long, device=dev)).reshape(-1)
    lens = (pos + 1).to(torch.int32)
    rope_pos = pos.clamp(0, cache.s_max - 1)
    tok_rows = rows_t.repeat_interleave(Q)
    cos, sin = model._rope_tables(cache.s_max, dev)

    def attend(i, attn, qkv):
        qkv = _append(attn, qkv, cache, i, cos, sin, pos, tok_rows, plan_len - 1, rope_pos)
        return ops.decode_attention_multi(qkv, cache.k[i], cache.v[i], rows_t, lens, Q, attn.nq, attn.nkv, attn.d,
                                          plan_len, window=attn.window, **cache.scales(i))

    x, res = _run_layers(model, ops.embedding(tokens.reshape(-1).to(dev), model.embed_tokens.weight), attend, linear, fp8)
    return _last_logits(model, x, res, linear, fp8)


def decode_bucket(length: int, s_max: int) -> int:
    """The length bucket a captured decode step is planned for: the smallest of 256, 512, 1024, ... that is
    >= `length`, capped at `s_max`.  256 is the decode plan's smallest chunk (decode::kMinChunk): below it
    the plan never splits, so shorter buckets would only add graphs."""
    if not 0 <= length <= s_max:
        raise ValueError(f"decode_bucket: length {length} outside [0, S_max = {s_max}]")
    b = 256
    while b < length:
        b *= 2
    return min(b, int(s_max))


def sample_next(logits, temperature=0.0, top_k=0, top_p=1.0, generator=None):
    """Next ids [n] from logits [n, V]: argmax at temperature 0, else a draw from the softmax of
    logits / temperature restricted to the top_k ids and the smallest set whose mass reaches top_p."""
    if temperature <= 0.0:
        return logits.argmax(-1)
    z = logits.float() / float(temperature)
    if top_k and top_k < z.shape[-1]:
        kth = z.topk(int(top_k), -1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    if top_p < 1.0:
        sz, si = z.sort(-1, descending=True)
        p = torch.softmax(sz, -1)
        drop = (p.cumsum(-1) - p) >= float(top_p)  # mass before this id already reaches top_p; the top id stays
        z = z.masked_fill(torch.zeros_like(drop).scatter(-1, si, drop), float("-inf"))
    return torch.multinomial(torch.softmax(z, -1), 1, generator=generator).squeeze(-1)


def _fused_params(n, **given):
    """Per-prompt host lists of the fused sampler's parameters; every value passes the scalar rules."""
    out = {}
    for name, v in given.items():
        vals = v.tolist() if isinstance(v, torch.Tensor) else (list(v) if isinstance(v, (list, tuple)) else [v] * n)
        if len(vals) != n:
            raise ValueError(f"generate: {name} has {len(vals)} values for {n} prompts")
        for x in vals:
            ops.check_sample_scalar(name, x)
        out[name] = vals
    return out


@torch.no_grad()
def generate(model, prompts: Sequence[torch.Tensor], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
             top_p: float = 1.0, eos_token_id: Optional[int] = None, seed: int = 0, s_max: Optional[int] = None,
             min_p: float = 0.0, sampler: str = "torch", linear: str = "blas", decode="eager",
             bucketed: bool = False, fp8=None, speculate=None, kv_cache: str = "bf16") -> List[torch.Tensor]:
    """Continue every prompt by up to `max_new_tokens` ids; returns the new ids of each sequence (1-D
    int64 tensors on the CPU), ending with `eos_token_id` where the sequence produced it.

    sampler="torch" (default): greedy at temperature 0, else `sample_next` with one torch.Generator
    seeded with `seed` for the whole batch.  sampler="fused": every step is one `ops.sample_logits`
    call (seed = `seed`, stream = the prompt's index, step = a device counter), so what a sequence
    draws does not depend on the other prompts of the batch; `temperature`, `top_k`, `top_p` and `min_p`
    may then each be a sequence with one value per prompt (a temperature of 0 makes that prompt greedy
    while the others sample).  The two samplers draw different ids for the same seed.  The per-sequence
    done mask lives on the device and is read on the host every HOST_CHECK_EVERY steps only; finished
    sequences keep running (their ids are discarded) until all are done or the budget is spent.
    `s_max` sizes the cache (default: longest prompt + max_new_tokens); prompt + max_new_tokens beyond
    it is an error.

    linear="skinny": the decode steps' projections run in `ops.skinny_linear` (at most 16 prompts; the
    prefill keeps hipBLASLt).  linear="skinny-fp8": they run in `ops.skinny_linear_fp8` on weight-only FP8
    copies of the matrices (models/quantized.py).  The model is not modified and keeps its bf16 weights; the
    prefill stays hipBLASLt in bf16 on the dequantised matrices, so the whole call computes one quantised
    model.  `fp8` is an `Fp8DecodeWeights` of this model to reuse, None quantises the model for this call.  decode="graph" (GPU only): the decode loop is captured into one HIP graph
    per length bucket (`decode_bucket`) and replayed, see models/decode_graph.py; sampling then needs
    sampler="fused", whose draw counter lives on the device.  `decode` may also be a `GraphedDecode`
    built for this model, batch size and `s_max`: its graphs and cache are reused.  decode="eager" with
    `bucketed=True` runs the eager loop with the launch plans of the captured one (plan_len = the
    bucket): with linear="skinny" the two loops return the same ids bit for bit.

    `speculate` (a `Speculative`, models/speculative.py; None leaves everything above as it is): speculative
    decoding with exact-match verification.  Every step runs the last accepted id and up to k - 1 drafted ids
    of each row through one `extend_step` and keeps the drafted ids that equal the model's own id of their
    position.  Eager only; sampling needs sampler="fused".  With linear="skinny" / "skinny-fp8" (at most
    SKINNY_MAX_M rows: prompts x k) the ids are those of the plain loop planned for the same length, bit for bit.

    kv_cache="fp8": the KV cache is e4m3 with one power-of-two scale per key vector (`KVCache`), about half the
    bytes; it composes with every `linear`, `decode` and `speculate` choice, and the bitwise promises above hold
    among the runs that use it."""
    _check_model(model)
    _check_kv_cache(kv_cache)
    prompts = [p.reshape(-1) for p in prompts]
    if not prompts or min(p.numel() for p in prompts) < 1:
        raise ValueError("generate: every prompt needs at least one token")
    if sampler not in ("torch", "fused"):
        raise ValueError(f"generate: sampler must be 'torch' or 'fused', got {sampler!r}")
    _check_linear(linear, len(prompts))
    if linear != "skinny-fp8" and fp8 is not None:
        raise ValueError(f'generate: fp8 weights were given with linear={linear!r}; they need linear="skinny-fp8"')
    graphed = not isinstance(decode, str)
    if not graphed and decode not in ("eager", "graph"):
        raise ValueError(f"generate: decode must be 'eager', 'graph' or a GraphedDecode, got {decode!r}")
    graphed = graphed or decode == "graph"
    if speculate is not None:
        from .speculative import check_speculate

        check_speculate(speculate, len(prompts), linear, graphed, sampler, temperature)
    if graphed:
        sampled = any(float(t) > 0.0 for t in (temperature.tolist() if isinstance(temperature, torch.Tensor) else
                                               temperature if isinstance(temperature, (list, tuple)) else [temperature]))
        if sampled and sampler != "fused":
            raise ValueError('generate: decode="graph" with temperature > 0 needs sampler="fused" (the torch sampler '
                             "draws from a host-side generator, which a captured step cannot advance)")
        if model.embed_tokens.weight.device.type != "cuda":
            raise ValueError('generate: decode="graph" needs a GPU (HIP-graph capture)')
    fused = None
    if sampler == "fused":
        fused = _fused_params(len(prompts), temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)
        if max_new_tokens < 0:
            raise ValueError("generate: need max_new_tokens >= 0")
    else:
        if any(isinstance(v, (list, tuple, torch.Tensor)) for v in (temperature, top_k, top_p, min_p)):
            raise ValueError('generate: per-prompt sampling parameters need sampler="fused"')
        if not 0.0 <= min_p <= 1.0:
            raise ValueError("generate: need 0 <= min_p <= 1")
        if min_p > 0.0:
            raise ValueError('generate: min_p needs sampler="fused"')
        if max_new_tokens < 0 or temperature < 0.0 or not 0.0 < top_p <= 1.0 or top_k < 0:
            raise ValueError("generate: need max_new_tokens >= 0, temperature >= 0, 0 < top_p <= 1, top_k >= 0")
    longest = max(p.numel() for p in prompts)
    if s_max is None:
        s_max = longest + max_new_tokens
    if longest + max_new_tokens > s_max:
        raise ValueError(f"generate: prompt ({longest}) + max_new_tokens ({max_new_tokens}) exceeds S_max ({s_max})")
    n = len(prompts)
    if max_new_tokens == 0:
        return [torch.empty(0, dtype=torch.long) for _ in range(n)]
    dev = model.embed_tokens.weight.device
    if graphed:
        from .decode_graph import GraphedDecode

        gd = decode if isinstance(decode, GraphedDecode) else GraphedDecode(model, n, s_max, linear=linear, fp8=fp8,
                                                                            kv_cache=kv_cache)
        if fp8 is not None and gd.fp8 is not fp8:
            raise ValueError("generate: the GraphedDecode was captured with other fp8 weights")
        if gd.cache.kv_cache != kv_cache:
            raise ValueError(f"generate: the GraphedDecode holds a {gd.cache.kv_cache} cache, kv_cache={kv_cache!r} was asked for")
        return gd.run(prompts, max_new_tokens, fused, seed, eos_token_id, s_max=s_max, linear=linear)
    fp8 = _check_fp8(model, linear, fp8, build=True)
    if speculate is not None:
        from .speculative import speculative_loop

        return speculative_loop(model, prompts, max_new_tokens, speculate, fused, seed, eos_token_id, s_max, linear, fp8,
                                kv_cache)
    gen = None
    if fused is not None:
        fused = {k: torch.tensor(v, dtype=torch.int32 if k == "top_k" else torch.float32, device=dev)
                 for k, v in fused.items()}
        stream = torch.arange(n, dtype=torch.int64, device=dev)
        step_t = torch.zeros(n, dtype=torch.int64, device=dev)  # the draw counter, advanced on the device
    elif temperature > 0.0:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
    cache = KVCache(model.config, n, s_max, device=dev, dtype=model.embed_tokens.weight.dtype, kv_cache=kv_cache)
    out = torch.zeros(n, max_new_tokens, dtype=torch.long, device=dev)
    count = torch.zeros(n, dtype=torch.long, device=dev)  # ids kept per sequence
    done = torch.zeros(n, dtype=torch.bool, device=dev)
    logits = prefill(model, prompts, cache, fp8=fp8)
    for step in range(max_new_tokens):
        if fused is not None:
            nxt, _ = ops.sample_logits(logits, seed=int(seed), stream=stream, step=step_t, **fused)
            step_t += 1
        else:
            nxt = sample_next(logits, temperature, top_k, top_p, gen)
        out[:, step] = nxt
        count += (~done).long()
        if eos_token_id is not None:
            done |= nxt == int(eos_token_id)
            if (step + 1) % HOST_CHECK_EVERY == 0 and bool(done.all()):
                break
        if step + 1 < max_new_tokens:
            plan_len = decode_bucket(cache.max_len + 1, s_max) if bucketed else None
            logits = decode_step(model, nxt, cache, linear=linear, plan_len=plan_len, fp8=fp8)
    out, count = out.cpu(), count.tolist()
    return [out[i, : count[i]].clone() for i in range(n)]
