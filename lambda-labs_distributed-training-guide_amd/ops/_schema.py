"""Operator schemas of the `dtg` library.

Schemas are declared once here; implementations register against them:
  * CUDA (= HIP on ROCm): the gfx950 kernels in csrc/kernels/*.hip (`_C.so`)
  * CPU: fp32 PyTorch reference implementations in `dtg.ops._cpu` (tests, CPU plumbing runs)
PyTorch's dispatcher picks the implementation from the tensors' device.
"""
import torch

LIB = torch.library.Library("dtg", "DEF")

_DEFS = [
    "rmsnorm_fwd(Tensor x, Tensor w, float eps) -> (Tensor, Tensor)",
    "add_rmsnorm_fwd(Tensor x, Tensor residual, Tensor w, float eps) -> (Tensor, Tensor, Tensor)",
    "rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd, Tensor? dres) -> (Tensor, Tensor)",
    # LayerNorm (GPT-2): y, mean, rstd; the fused form first makes h = residual + dropout(x) (keep mask
    # from Philox(rng), nothing stored; rng = None iff p == 0) and returns y, h, mean, rstd.  The
    # backward returns dh, dx (the dropped branch's gradient; dh itself when p == 0), dw, db.
    "layernorm_fwd(Tensor x, Tensor w, Tensor b, float eps) -> (Tensor, Tensor, Tensor)",
    "dropout_add_layernorm_fwd(Tensor x, Tensor residual, Tensor w, Tensor b, float eps, float p, Tensor? rng) "
    "-> (Tensor, Tensor, Tensor, Tensor)",
    "layernorm_bwd(Tensor dy, Tensor h, Tensor w, Tensor mean, Tensor rstd, Tensor? dres, float p, Tensor? rng) "
    "-> (Tensor, Tensor, Tensor, Tensor)",
    # GELU-tanh; gelu_bwd_t also returns dx^T and gelu(x)^T (the TN operands of the MLP's dW GEMMs)
    "gelu_fwd(Tensor x) -> Tensor",
    "gelu_bwd(Tensor dh, Tensor x) -> Tensor",
    "gelu_bwd_t(Tensor dh, Tensor x) -> (Tensor, Tensor, Tensor)",
    "rope_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos, int nheads, int head_dim, bool inverse) -> ()",
    # per-head RMSNorm of the q and k heads of a fused QKV activation + RoPE, in place (Qwen3); empty
    # cos / sin = norm only.  fwd returns (xqk: the pre-norm q|k [T, (nq + nkv) * D], rstd f32 [T, nq + nkv]);
    # bwd turns the gradient w.r.t. the rotated q / k into dx in place and returns (dwq, dwk)
    "qk_norm_rope_fwd_(Tensor(a!) qkv, Tensor wq, Tensor wk, Tensor cos, Tensor sin, Tensor pos, int nq, int nkv, "
    "int head_dim, float eps) -> (Tensor, Tensor)",
    "qk_norm_rope_bwd_(Tensor(a!) dqkv, Tensor xqk, Tensor rstd, Tensor wq, Tensor wk, Tensor cos, Tensor sin, "
    "Tensor pos, int nq, int nkv, int head_dim) -> (Tensor, Tensor)",
    # KV-cache generation (csrc/kernels/decode_attn.hip); caches are bf16 [rows_max, nkv, S_max, D].
    # append: RoPE at pos[t] on the q and k heads of qkv in place (empty cos / sin = already roped, copy
    # only), then the roped k and the v go to cache[rows[t], :, pos[t], :]; pos int64 [T], rows int32 [T];
    # a token whose pos / rows lie outside the cache is skipped
    "kv_cache_append_(Tensor(a!) qkv, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor cos, Tensor sin, Tensor pos, "
    "Tensor rows, int nq, int nkv, int head_dim) -> ()",
    # one query token per sequence (its q heads read out of the fused qkv row b) against keys
    # [max(0, lens[b] - window), lens[b]) of cache row rows[b]; rows / lens int32 [B] on the device,
    # max_len a host upper bound of lens (launch plan only), splits = 0 takes the plan's split count
    "decode_attn(Tensor qkv, Tensor k_cache, Tensor v_cache, Tensor rows, Tensor lens, int nq, int nkv, int head_dim, "
    "float scale, int max_len, int window=0, int splits=0) -> Tensor",
    # q_len new tokens per sequence (speculative verification): qkv [B * q_len, ...] sequence-major, rows int32 [B],
    # lens int32 [B * q_len], one attended length per token; token (b, t) attends keys [max(0, len - window), len)
    # of cache row rows[b] (len <= 0 or a bad row: a row of zeros).  Causality among the new tokens is the
    # caller's (it passes pos + 1).  At window 0 a token's output row is bit for bit decode_attn's for that token
    # alone with the same max_len and splits.  The keys between the ranges of one sequence's tokens are read too.
    "decode_attn_multi(Tensor qkv, Tensor k_cache, Tensor v_cache, Tensor rows, Tensor lens, int q_len, int nq, "
    "int nkv, int head_dim, float scale, int max_len, int window, int splits) -> Tensor",
    # the same two on an FP8 cache (the kernels' e4m3 cache format): k_cache / v_cache float8_e4m3fn (OCP)
    # [rows_max, nkv, S_max, D], k_scale / v_scale f32 [rows_max, nkv, S_max], one scale per key vector: the power
    # of two that puts the vector's amax into (224, 448] (ops.quantize_fp8_rows(pow2=True) of the D-vector, bit for
    # bit; for k, of the roped k).  The append also writes the dequantised k / v (code * scale, exact in bf16) back
    # into qkv.  decode_attn_fp8 is decode_attn at q_len = 1 and decode_attn_multi at q_len > 1, and returns bit
    # for bit what they return on the dequantised bf16 caches
    "kv_cache_append_fp8_(Tensor(a!) qkv, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor(d!) k_scale, "
    "Tensor(e!) v_scale, Tensor cos, Tensor sin, Tensor pos, Tensor rows, int nq, int nkv, int head_dim) -> ()",
    "decode_attn_fp8(Tensor qkv, Tensor k_cache, Tensor v_cache, Tensor k_scale, Tensor v_scale, Tensor rows, "
    "Tensor lens, int q_len, int nq, int nkv, int head_dim, float scale, int max_len, int window, int splits) -> Tensor",
    # fused top-k / top-p / min-p sampling (csrc/kernels/sample.hip): logits [n, V] bf16 / f32 with unit
    # inner stride; params f32 [n, 3] = temperature, top_p, min_p; top_k int32 [n]; rng int64 [n, 3] =
    # seed, stream, step of the row's Philox draw; u f32 [n] in [0, 1) replaces that draw.  Returns
    # (ids int64 [n], kept int32 [n] = size of the set the row was drawn from); nothing is read on the host
    "sample_logits(Tensor logits, Tensor params, Tensor top_k, Tensor rng, Tensor? u=None) -> (Tensor, Tensor)",
    # decode-step projection (csrc/kernels/skinny_gemm.hip): y = x @ w^T (+ bias) for x bf16 [M, K], 1 <= M <= 16
    # (unit inner stride, 16-B aligned rows), w bf16 [N, K] contiguous, K % 8 == 0, f32 accumulation, one
    # rounding; act = 1: w = gate rows then up rows, returns swiglu_fwd of that product, [M, N / 2]
    "skinny_linear(Tensor x, Tensor w, Tensor? bias, int act=0) -> Tensor",
    # the same with weight-only FP8 (the same kernel, its e4m3 weight format): wq float8_e4m3fn (OCP) [N, K]
    # contiguous, K % 16 == 0, scale f32 [N] (one per weight row): y = (x @ float(wq)^T) * scale (+ bias)
    "skinny_linear_fp8(Tensor x, Tensor wq, Tensor scale, Tensor? bias, int act=0) -> Tensor",
    "swiglu_fwd(Tensor gu) -> Tensor",
    "swiglu_bwd(Tensor dh, Tensor gu) -> Tensor",
    "swiglu_bwd_t(Tensor dh, Tensor gu) -> (Tensor, Tensor, Tensor)",
    "ce_fwd_bwd_(Tensor(a!) logits, Tensor labels, int ignore_index, float grad_scale, bool compute_grad) -> Tensor",
    "ce_stats(Tensor logits, Tensor labels, int vocab_start) -> (Tensor, Tensor, Tensor)",
    "ce_grad_(Tensor(a!) logits, Tensor labels, Tensor lse, int vocab_start, int ignore_index, float grad_scale) -> ()",
    "adamw_(Tensor(a!) p, Tensor(b!)? master, Tensor g, Tensor(c!) m, Tensor(d!) v, float lr, float beta1, "
    "float beta2, float eps, float wd, int step, float grad_scale, Tensor? hyper=None, Tensor? gscale=None) -> ()",
    # AdamW over the matrices `mats` (int64 [n, 5]: offset, rows, cols, transposed offset or -1,
    # first tile, counted in 64 x tile_cols tiles) of the flat buffers, also writing each matrix's
    # transpose into `pt`
    "adamw_t_(Tensor(a!) p, Tensor(b!)? master, Tensor g, Tensor(c!) m, Tensor(d!) v, Tensor(e!) pt, Tensor mats, "
    "int ntiles, float lr, float beta1, float beta2, float eps, float wd, int step, float grad_scale, "
    "Tensor? hyper=None, int tile_cols=64, Tensor? gscale=None) -> ()",
    # acc[slot] += sum of squares of the contiguous 1-D gradient buffer g (bf16 / f32), accumulated
    # in f32, bitwise reproducible; `gscale` of adamw_ / adamw_t_ above is the device f32 [1] clip
    # coefficient derived from it, multiplied into grad_scale by the kernel
    "grad_sumsq_(Tensor g, Tensor(a!) acc, int slot) -> ()",
    "adamw_cpu_(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, float lr, float beta1, float beta2, "
    "float eps, float wd, int step, float grad_scale) -> ()",
    # window > 0 (causal only): sliding window, query i sees keys (i - window, i]
    "flash_attn_fwd(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, int max_seqlen, float scale, bool causal, "
    "int window=0) -> (Tensor, Tensor)",
    "flash_attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor cu_seqlens, "
    "int max_seqlen, float scale, bool causal, int window=0) -> (Tensor, Tensor, Tensor)",
    "flash_attn_bwd_qkv(Tensor dout, Tensor qkv, int nq, int nkv, int head_dim, Tensor o, Tensor lse, "
    "Tensor cu_seqlens, int max_seqlen, float scale, bool causal, int window=0) -> Tensor",
    # the same with the RoPE backward of the q / k heads fused into the dQ / dK epilogues
    "flash_attn_bwd_qkv_rope(Tensor dout, Tensor qkv, int nq, int nkv, int head_dim, Tensor o, Tensor lse, "
    "Tensor cu_seqlens, int max_seqlen, float scale, bool causal, Tensor cos, Tensor sin, Tensor pos, "
    "int window=0) -> Tensor",
    # attention-probability dropout regenerated from Philox(seed, offset) in the backward; `rng` is
    # the int64 [2] tensor {seed, offset} of the call (philox_rng: torch's generator, graph-safe)
    "flash_attn_fwd_drop(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, int max_seqlen, float scale, bool causal, "
    "float p, Tensor rng) -> (Tensor, Tensor)",
    "flash_attn_bwd_drop(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor cu_seqlens, "
    "int max_seqlen, float scale, bool causal, float p, Tensor rng) -> (Tensor, Tensor, Tensor)",
    "flash_attn_bwd_qkv_drop(Tensor dout, Tensor qkv, int nq, int nkv, int head_dim, Tensor o, Tensor lse, "
    "Tensor cu_seqlens, int max_seqlen, float scale, bool causal, float p, Tensor rng) -> Tensor",
    "philox_rng(Tensor like, int increment) -> Tensor",
    "transpose2d(Tensor x) -> Tensor",
    # many matrices of a flat buffer transposed in one launch: rows of `mats` (int64 [n, 5]:
    # source offset, rows, cols, destination offset, first 64 x 64 tile); `mats_host` = its CPU copy
    "transpose_mats_(Tensor x, Tensor(a!) out, Tensor mats, Tensor mats_host, int ntiles) -> ()",
    "embedding_bwd_(Tensor(a!) out, Tensor ids, Tensor dy) -> ()",
    # FlashAttention-2-style varlen with explicit per-sequence key ranges (disjoint), causal mask
    # bottom-right aligned: context parallelism's local query chunks over gathered key prefixes
    "flash_attn_varlen_fwd(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor k_start, Tensor k_len, "
    "int max_seqlen_q, int max_seqlen_k, float scale, bool causal) -> (Tensor, Tensor)",
    "flash_attn_varlen_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor cu_seqlens_q, "
    "Tensor k_start, Tensor k_len, int max_seqlen_q, int max_seqlen_k, float scale, bool causal) "
    "-> (Tensor, Tensor, Tensor)",
    "flash_attn_fwd_stamped(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, int max_seqlen, float scale, "
    "bool causal) -> (Tensor, Tensor, Tensor)",
    # backward launch tuning (read once from DTG_FA_* at load): set (kv_split, kv_qb), a negative
    # value keeps a knob; returns the previous pair.  `like` picks the device's implementation.
    "flash_attn_tuning(Tensor like, int kv_split, int kv_qb) -> int[]",
]

for _d in _DEFS:
    LIB.define(_d)
