"""Autograd functions for the decoder hot path.

Each function is a thin torch.autograd.Function over `torch.ops.dtg.*` (HIP on GPU, f32
reference on CPU) or hipBLASLt GEMMs (`torch.mm`).  Activations stay 2-D token-major
[T, features] end to end, so no transposes/copies appear between kernels.
"""
import math
import os

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import grad_routing as _gr
from ._cpu import SKINNY_MAX_M
from .grad_routing import route_embedding_grad, route_param_grad, route_weight_grad_mm

ops = torch.ops.dtg


# --------------------------------------------------------------------------------------------
# Linear (hipBLASLt) with direct weight-gradient routing
# --------------------------------------------------------------------------------------------
# Operand layouts of the backward GEMMs.  hipBLASLt's MFMA kernels are fastest when both
# operands are K-contiguous ("TN"); dX = dY W reads W along its strided dim ("NN") and
# dW = dY^T X reduces over the strided token dim of both activations ("NT").  With
# DTG_LINEAR_BWD=tn the backward hands hipBLASLt explicit transposed copies (one streaming
# pass each through csrc/kernels/transpose.hip); "native" keeps the strided forms; "auto"
# transposes W for every dX and dY, X only for dW of layers whose output is at least as wide as
# their input.  Measured on MI355X (Llama-3-8B, b16 x s1024, profiles/r1/s15_*): native 24.0k,
# auto 25.4k, tn 25.4k tok/s; round 2 with every layout's shapes tuned (profiles/r2/s32/bench_*.log):
# native 24.3k, auto 27.0k, tn 27.0-27.1k -- "tn" is the default.
_LINEAR_BWD = os.environ.get("DTG_LINEAR_BWD", "tn")
_TN_MIN_TOKENS = 4096


def _tn_ok(*ts):
    return all(t.is_cuda and t.dtype == torch.bfloat16 and t.shape[0] % 8 == 0 and t.shape[1] % 8 == 0
               and t.stride(1) == 1 for t in ts)


def _wt(w):
    """K-contiguous W^T for dX = dY W: the engine's persistent copy (refreshed by the optimizer
    kernel, parallel/data_parallel.py) when it is current, else a transpose now."""
    ref = getattr(w, "_dtg_wt", None)
    if ref is not None:
        t = ref[0].weight_t(ref[1])
        if t is not None:
            return t
    return ops.transpose2d(w)


def _bwd_layout(x, w):
    """(dx_tn, dw_tn) for this Linear's backward."""
    mode = _LINEAR_BWD
    if mode == "native" or x.shape[0] < _TN_MIN_TOKENS or not _tn_ok(x, w):
        return False, False
    if mode == "tn":
        return True, True
    return True, w.shape[0] >= w.shape[1]


def _bias_grad(b, dy):
    """b's gradient: the f32 column sum of dy, rounded once."""
    return route_param_grad(b, dy.sum(0, dtype=torch.float32).to(dy.dtype))


def _dx_mm(dy, w, tn):
    """dX = dy @ w, from the K-contiguous W^T when `tn`."""
    return torch.mm(dy, _wt(w).t()) if tn else torch.mm(dy, w)


def _dw_mm(w, dy, x, tn, dy_t=None, x_t=None):
    """w's gradient dy^T @ x; when `tn`, from token-contiguous operands (dy_t / x_t where the
    caller has them, else transposed here)."""
    if not (tn and _tn_ok(dy)):
        return route_weight_grad_mm(w, dy, x)
    return route_weight_grad_mm(w, dy, x, a_t=ops.transpose2d(dy) if dy_t is None else dy_t,
                                b_t=ops.transpose2d(x) if x_t is None else x_t)


def _linear_backward(ctx, dy, x, w):
    dx_tn, dw_tn = _bwd_layout(x, w)
    dx = _dx_mm(dy, w, dx_tn) if ctx.needs_input_grad[0] else None
    dw = _dw_mm(w, dy, x, dw_tn) if ctx.needs_input_grad[1] else None
    return dx, dw


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, out=None):
        ctx.save_for_backward(x, w)
        if out is not None:  # (buffer,): hidden from autograd, e.g. an xGMI workspace slot
            return torch.mm(x, w.t(), out=out[0])
        return torch.mm(x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return (*_linear_backward(ctx, dy, x, w), None)


def linear(x, w, b=None, out=None):
    """y = x @ w^T (+ b); x is [T, in].  `out`: preallocated [T, out_features] result buffer
    (no bias) -- the zero-copy reduce-scatter input of a tensor-parallel region."""
    if b is None:
        return _Linear.apply(x, w, None if out is None else (out,))
    assert out is None, "linear: out= is for the bias-free projections"
    return _LinearBias.apply(x, w, b)


class _LinearBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dx, dw = _linear_backward(ctx, dy, x, w)
        return dx, dw, _bias_grad(b, dy) if ctx.needs_input_grad[2] else None


# --------------------------------------------------------------------------------------------
# RMSNorm and fused residual-add + RMSNorm
# --------------------------------------------------------------------------------------------
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        y, rstd = ops.rmsnorm_fwd(x, w, eps)
        ctx.save_for_backward(x, w, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dx, dw = ops.rmsnorm_bwd(dy, x, w, rstd, None)
        return dx, route_param_grad(w, dw), None


class _AddRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, w, eps):
        y, h, rstd = ops.add_rmsnorm_fwd(x, res, w, eps)
        ctx.save_for_backward(h, w, rstd)
        return y, h

    @staticmethod
    def backward(ctx, dy, dh):
        h, w, rstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(h)
        dx, dw = ops.rmsnorm_bwd(dy, h, w, rstd, dh)
        return dx, dx, route_param_grad(w, dw), None


def rms_norm(x, w, eps):
    return _RMSNorm.apply(x, w, eps)


def add_rms_norm(x, res, w, eps):
    """Returns (rmsnorm(x + res), x + res)."""
    return _AddRMSNorm.apply(x, res, w, eps)


# --------------------------------------------------------------------------------------------
# LayerNorm and fused dropout + residual-add + LayerNorm (GPT-2)
# --------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, mean, rstd = ops.layernorm_fwd(x, w, b, eps)
        ctx.save_for_backward(x, w, b, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dx, _, dw, db = ops.layernorm_bwd(dy, x, w, mean, rstd, None, 0.0, None)
        return dx, route_param_grad(w, dw), route_param_grad(b, db), None


class _DropoutAddLayerNorm(torch.autograd.Function):
    """y = layernorm(h), h = res + dropout(x, p), one pass each way.  The keep mask is a Philox
    function of (rng, row, column), regenerated in the backward (no mask stored); `rng` is the
    device tensor of `dropout_rng`, so a captured HIP graph draws a new mask every replay."""

    @staticmethod
    def forward(ctx, x, res, w, b, eps, p, rng):
        y, h, mean, rstd = ops.dropout_add_layernorm_fwd(x, res, w, b, eps, p, rng)
        saved = (h, w, b, mean, rstd) if rng is None else (h, w, b, mean, rstd, rng)
        ctx.save_for_backward(*saved)
        ctx.p = p
        return y, h

    @staticmethod
    def backward(ctx, dy, dh_in):
        h, w, b, mean, rstd, *rng = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(h)
        dh, dx, dw, db = ops.layernorm_bwd(dy, h, w, mean, rstd, dh_in, ctx.p, rng[0] if rng else None)
        return dx, dh, route_param_grad(w, dw), route_param_grad(b, db), None, None, None


def layer_norm(x, w, b, eps):
    return _LayerNorm.apply(x, w, b, eps)


def dropout_add_layer_norm(x, res, w, b, eps, p=0.0):
    """Returns (layernorm(h), h) with h = res + dropout(x, p); draws its own rng when p > 0."""
    p = float(p)
    return _DropoutAddLayerNorm.apply(x, res, w, b, eps, p, dropout_rng(x) if p > 0.0 else None)


# --------------------------------------------------------------------------------------------
# Rotary tables
# --------------------------------------------------------------------------------------------
def _llama3_inv_freq(inv_freq, scaling):
    factor = scaling["factor"]
    low = scaling.get("low_freq_factor", 1.0)
    high = scaling.get("high_freq_factor", 4.0)
    old_ctx = scaling["original_max_position_embeddings"]
    low_wl = old_ctx / low
    high_wl = old_ctx / high
    wavelen = 2 * math.pi / inv_freq
    out = torch.where(wavelen > low_wl, inv_freq / factor, inv_freq)
    smooth = (old_ctx / wavelen - low) / (high - low)
    smoothed = (1 - smooth) * out / factor + smooth * out
    is_medium = (wavelen >= high_wl) & (wavelen <= low_wl)
    return torch.where(is_medium, smoothed, out)


def rope_tables(head_dim, theta, max_pos, scaling=None, device=None):
    """cos/sin [max_pos, head_dim/2] f32 (HF LlamaRotaryEmbedding semantics, incl. llama3 scaling)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    attn_factor = 1.0
    if scaling is not None:
        kind = scaling.get("rope_type", scaling.get("type"))
        if kind == "llama3":
            inv_freq = _llama3_inv_freq(inv_freq, scaling)
        elif kind in (None, "default"):
            pass
        else:
            raise NotImplementedError(f"rope scaling {kind}")
    t = torch.arange(max_pos, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)
    cos = (freqs.cos() * attn_factor).contiguous()
    sin = (freqs.sin() * attn_factor).contiguous()
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return cos, sin


# --------------------------------------------------------------------------------------------
# Attention (RoPE fused into the same autograd node; fused QKV in, fused dQKV out)
# --------------------------------------------------------------------------------------------
# The RoPE backward of the q / k heads runs inside the attention backward's dQ / dK epilogues
# (csrc/kernels/flash_attn.hip, one bf16 rounding) instead of a separate in-place pass:
# -1.64 ms of RoPE kernels, +0.78 ms of epilogue per 8B step (profiles/r4/s45).
# DTG_FA_ROPE_FUSED=0 restores the separate pass.
_FA_ROPE_FUSED = os.environ.get("DTG_FA_ROPE_FUSED", "1") == "1"


def _qkv_head_views(qkv, nq, nkv, d):
    """q [T, nq, d], k and v [T, nkv, d]: strided head views of a fused [T, (nq + 2 nkv) * d]."""
    T = qkv.shape[0]

    def view(h0, nh):
        return qkv.as_strided((T, nh, d), (qkv.stride(0), d, 1), qkv.storage_offset() + h0 * d)

    return view(0, nq), view(nq, nkv), view(nq + nkv, nkv)


class _AttentionQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, pos, cu_seqlens, max_seqlen, nq, nkv, head_dim, scale, causal, rope, window):
        T = qkv.shape[0]
        d = head_dim
        if rope:
            ops.rope_(qkv, cos, sin, pos, nq + nkv, d, False)
        q, k, v = _qkv_head_views(qkv, nq, nkv, d)
        o, lse = ops.flash_attn_fwd(q, k, v, cu_seqlens, max_seqlen, scale, causal, window)
        ctx.save_for_backward(qkv, o, lse, cu_seqlens, cos, sin, pos)
        ctx.meta = (max_seqlen, nq, nkv, d, scale, causal, rope, window)
        return o.view(T, nq * d)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cu, cos, sin, pos = ctx.saved_tensors
        max_seqlen, nq, nkv, d, scale, causal, rope, window = ctx.meta
        T = qkv.shape[0]
        if rope and _FA_ROPE_FUSED:  # RoPE backward inside the dQ / dK epilogues
            dqkv = ops.flash_attn_bwd_qkv_rope(do.contiguous().view(T, nq, d), qkv, nq, nkv, d, o, lse, cu, max_seqlen,
                                               scale, causal, cos, sin, pos, window)
        else:
            dqkv = ops.flash_attn_bwd_qkv(do.contiguous().view(T, nq, d), qkv, nq, nkv, d, o, lse, cu, max_seqlen,
                                          scale, causal, window)
            if rope:
                ops.rope_(dqkv, cos, sin, pos, nq + nkv, d, True)
        return dqkv, None, None, None, None, None, None, None, None, None, None, None, None


class _AttentionQKVDrop(torch.autograd.Function):
    """Attention with dropout on the probabilities, inside the flash kernels: the keep mask is a
    counter-based (Philox) function of (seed, offset, head, query, key), drawn in the forward and
    regenerated in the backward -- nothing [S, S] is stored.  {seed, offset} is a device tensor
    drawn from torch's CUDA generator (ops.philox_rng), so a captured HIP graph draws a new mask
    every replay (a Python int would be baked into the graph)."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, nq, nkv, head_dim, scale, causal, p, rng):
        T = qkv.shape[0]
        d = head_dim
        q, k, v = _qkv_head_views(qkv, nq, nkv, d)
        o, lse = ops.flash_attn_fwd_drop(q, k, v, cu_seqlens, max_seqlen, scale, causal, p, rng)
        ctx.save_for_backward(qkv, o, lse, cu_seqlens, rng)
        ctx.meta = (max_seqlen, nq, nkv, d, scale, causal, p)
        return o.view(T, nq * d)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cu, rng = ctx.saved_tensors
        max_seqlen, nq, nkv, d, scale, causal, p = ctx.meta
        T = qkv.shape[0]
        dqkv = ops.flash_attn_bwd_qkv_drop(do.contiguous().view(T, nq, d), qkv, nq, nkv, d, o, lse, cu, max_seqlen,
                                           scale, causal, p, rng)
        return dqkv, None, None, None, None, None, None, None, None, None


def dropout_rng(like):
    """{seed, offset} (int64 [2] on `like`'s device) of one attention-dropout call: torch's CUDA
    generator on a GPU (graph-safe), its CPU generator on the CPU reference path."""
    return ops.philox_rng(like, 4)


class _Rope(torch.autograd.Function):
    """Out-of-place RoPE on the q and k heads of a fused QKV activation (v untouched)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, pos, nheads, head_dim):
        y = qkv.contiguous().clone()
        ops.rope_(y, cos, sin, pos, nheads, head_dim, False)
        ctx.save_for_backward(cos, sin, pos)
        ctx.meta = (nheads, head_dim)
        return y

    @staticmethod
    def backward(ctx, dy):
        cos, sin, pos = ctx.saved_tensors
        dx = dy.contiguous().clone()
        ops.rope_(dx, cos, sin, pos, ctx.meta[0], ctx.meta[1], True)
        return dx, None, None, None, None, None


def rope(qkv, cos, sin, pos, nheads, head_dim):
    return _Rope.apply(qkv, cos, sin, pos, int(nheads), int(head_dim))


FA_HEAD_DIMS = (64, 128)  # head dims the flash-attention kernels are instantiated for


# --------------------------------------------------------------------------------------------
# Per-head QK RMSNorm + RoPE (Qwen3), one pass each way (csrc/kernels/qk_norm.hip)
# --------------------------------------------------------------------------------------------
# DTG_QKNORM_FUSED=0 takes the composed path below instead (a copy, the norms in torch, the
# separate RoPE pass): the fused kernel's A/B partner and the yardstick of its accuracy tests.
_QKNORM_FUSED = os.environ.get("DTG_QKNORM_FUSED", "1") == "1"


class _QKNormRope(torch.autograd.Function):
    """y = rope(w * x * rstd) on the q and k heads of a fused QKV activation, in place (v untouched).
    Saves the pre-norm q|k copy the kernel writes and rstd; the backward turns the gradient w.r.t.
    the rotated q / k (what the attention backward without RoPE returns) into dx, in place when
    `grad_inplace` says the incoming gradient belongs to this node alone, else on a copy."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, cos, sin, pos, nq, nkv, head_dim, eps, grad_inplace):
        xqk, rstd = ops.qk_norm_rope_fwd_(qkv, wq, wk, cos, sin, pos, nq, nkv, head_dim, eps)
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(xqk, rstd, wq, wk, cos, sin, pos)
        ctx.meta = (nq, nkv, head_dim, grad_inplace)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        xqk, rstd, wq, wk, cos, sin, pos = ctx.saved_tensors
        nq, nkv, d, grad_inplace = ctx.meta
        dense = dqkv.dim() == 2 and dqkv.stride(1) == 1 and dqkv.stride(0) >= dqkv.shape[1] and dqkv.stride(0) % 8 == 0
        if not (grad_inplace and dense):
            dqkv = dqkv.contiguous().clone() if dense else dqkv.contiguous()
        dwq, dwk = ops.qk_norm_rope_bwd_(dqkv, xqk, rstd, wq, wk, cos, sin, pos, nq, nkv, d)
        return (dqkv, route_param_grad(wq, dwq), route_param_grad(wk, dwk), None, None, None, None, None, None, None,
                None)


class _RoutedParam(torch.autograd.Function):
    """Identity on a parameter whose gradient goes through route_param_grad (for torch-composed paths)."""

    @staticmethod
    def forward(ctx, w):
        ctx.w = w
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        return route_param_grad(ctx.w, g.to(ctx.w.dtype))


def _qk_norm_rope_composed(qkv, wq, wk, eps, nq, nkv, d, cos, sin, pos):
    """The same function from torch ops, out of place: the q|k heads copied out and widened, RMSNorm
    over head_dim and rope_'s rotation in f32, one rounding back to the activation dtype (the fused
    kernel's numerics, so the two agree to the rounding of one store); autograd differentiates it."""
    T, nh = qkv.shape[0], nq + nkv
    xf = qkv[:, : nh * d].reshape(T, nh, d).float()
    n = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    wq, wk = _RoutedParam.apply(wq).float(), _RoutedParam.apply(wk).float()
    y = torch.cat([wq * n[:, :nq], wk * n[:, nq:]], 1)
    if cos is not None:
        h = d // 2
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        y1, y2 = y[..., :h], y[..., h:]
        y = torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], -1)
    return torch.cat([y.reshape(T, nh * d).to(qkv.dtype), qkv[:, nh * d:]], 1)


def qk_norm_rope(qkv, wq, wk, eps, nq, nkv, head_dim, cos=None, sin=None, pos=None, grad_inplace=False):
    """Qwen3's per-head RMSNorm of the q and k heads of a fused [T, (nq + 2 nkv) * d] activation
    (weights wq / wk [d], shared by all heads), followed by RoPE when cos / sin / pos are given
    (norm only otherwise).  One fused pass, in place on `qkv`; follow it with `attention(...)`
    WITHOUT cos / sin / pos.  `grad_inplace`: the backward may overwrite the incoming gradient
    (true when the only consumer is `attention`, whose backward returns a fresh fused dQKV).
    GPU head dims without a kernel instantiation, and DTG_QKNORM_FUSED=0, take the composed path."""
    nq, nkv, d = int(nq), int(nkv), int(head_dim)
    if not _QKNORM_FUSED or (qkv.is_cuda and d not in FA_HEAD_DIMS):
        return _qk_norm_rope_composed(qkv, wq, wk, float(eps), nq, nkv, d, cos, sin, pos)
    if cos is None:
        cos = sin = torch.empty(0, device=qkv.device)
        pos = torch.empty(0, dtype=torch.long, device=qkv.device)
    if qkv.is_leaf and qkv.requires_grad:  # a leaf cannot be written in place
        qkv = qkv.clone()
    return _QKNormRope.apply(qkv, wq, wk, cos, sin, pos, nq, nkv, d, float(eps), bool(grad_inplace))


def _attention_padded(qkv, nq, nkv, d, cu_seqlens, max_seqlen, cos, sin, pos, causal, scale, window):
    """Head dims without a kernel instantiation (e.g. 80, 96, 48): zero-pad every head to the next
    instantiated width.  Zero columns add nothing to q.k (the scale keeps 1/sqrt(d) of the true
    width) and give zero output columns, which are sliced off; autograd drops their gradients.
    Costs the padded width's FLOPs, not a second code path."""
    dp = next((x for x in FA_HEAD_DIMS if x >= d), None)
    if dp is None or d % 2:
        raise ValueError(f"attention: head_dim {d} unsupported (kernels: {FA_HEAD_DIMS}; smaller even dims are padded)")
    T = qkv.shape[0]
    x = qkv.reshape(T, nq + 2 * nkv, d)
    if cos is not None:  # RoPE out of place in torch (the rope kernel is instantiated for 64/128 too)
        h = d // 2
        qk = x[:, : nq + nkv].float()
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        x1, x2 = qk[..., :h], qk[..., h:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)
        x = torch.cat([rot, x[:, nq + nkv:]], 1)
    xp = F.pad(x, (0, dp - d)).reshape(T, (nq + 2 * nkv) * dp)
    e = torch.empty(0, device=qkv.device)
    o = _AttentionQKV.apply(xp, e, e, torch.empty(0, dtype=torch.long, device=qkv.device), cu_seqlens, int(max_seqlen),
                            nq, nkv, dp, float(scale), causal, False, int(window or 0))
    return o.view(T, nq, dp)[..., :d].reshape(T, nq * d)


def attention(qkv, nq, nkv, head_dim, cu_seqlens, max_seqlen, cos=None, sin=None, pos=None, causal=True, scale=None,
              window=0, dropout_p=0.0):
    """Causal (varlen) GQA attention on a fused [T, (nq+2nkv)*d] QKV activation -> [T, nq*d].

    If cos/sin/pos are given, RoPE is applied to q and k first (in place on qkv).  window > 0:
    sliding-window attention (query i sees keys i - window < j <= i; Mistral).  dropout_p > 0:
    dropout on the attention probabilities inside the flash kernels (GPT-2 training)."""
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if dropout_p > 0.0:
        if cos is not None or window:
            raise ValueError("attention dropout is supported without RoPE / sliding windows (GPT-2)")
        if qkv.is_cuda and head_dim not in FA_HEAD_DIMS:
            raise ValueError(f"attention dropout: head_dim {head_dim} needs a kernel instantiation {FA_HEAD_DIMS}")
        return _AttentionQKVDrop.apply(qkv, cu_seqlens, int(max_seqlen), nq, nkv, head_dim, float(scale), causal,
                                       float(dropout_p), dropout_rng(qkv))
    if qkv.is_cuda and head_dim not in FA_HEAD_DIMS:  # the CPU reference takes any width
        return _attention_padded(qkv, nq, nkv, head_dim, cu_seqlens, max_seqlen, cos, sin, pos, causal, scale, window)
    rope = cos is not None
    if not rope:
        cos = sin = torch.empty(0, device=qkv.device)
        pos = torch.empty(0, dtype=torch.long, device=qkv.device)
    return _AttentionQKV.apply(qkv, cos, sin, pos, cu_seqlens, int(max_seqlen), nq, nkv, head_dim, float(scale), causal, rope,
                               int(window or 0))


# --------------------------------------------------------------------------------------------
# KV-cache generation: cache append and split-KV decode attention (csrc/kernels/decode_attn.hip)
# --------------------------------------------------------------------------------------------
# Inference only (no autograd).  DTG_DECODE_FUSED=0 composes both ops from torch ops instead (the
# kernels' A/B partner and the yardstick of their accuracy tests); so do, on a GPU, dtypes other than
# bf16 and head dims and group sizes the kernels are not instantiated for.
#
# FP8 cache: the three ops take `k_scale` / `v_scale` (None = the bf16 cache, today's path byte for byte).
# With scales the caches are float8_e4m3fn [rows_max, nkv, S_max, D] and the scales f32 [rows_max, nkv, S_max],
# one per key vector, by the rule of `quantize_fp8_rows(pow2=True)` on the D-vector; the append also writes
# the dequantised k / v back into qkv.  The compositions dequantise (`cache.float() * scale[..., None]` into
# qkv's dtype) and run as for bf16; the composed append quantises with `quantize_fp8_rows`.
_DECODE_FUSED = os.environ.get("DTG_DECODE_FUSED", "1") == "1"
DECODE_GROUPS = (1, 2, 3, 4, 7, 8, 16)  # query heads per kv head the decode kernel is instantiated for


def _decode_kernels(qkv, nq, nkv, d):
    if not _DECODE_FUSED:
        return False
    return not qkv.is_cuda or (qkv.dtype == torch.bfloat16 and d in FA_HEAD_DIMS and nq // nkv in DECODE_GROUPS)


def _check_cache_args(name, qkv, k_cache, v_cache, nq, nkv, d, index, k_scale=None, v_scale=None):
    if nq < 1 or nkv < 1 or nq % nkv:
        raise ValueError(f"{name}: nq ({nq}) must be a positive multiple of nkv ({nkv})")
    if qkv.dim() != 2 or qkv.shape[1] != (nq + 2 * nkv) * d:
        raise ValueError(f"{name}: qkv must be [T, (nq + 2 nkv) * head_dim], got {tuple(qkv.shape)}")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[1] != nkv or k_cache.shape[3] != d:
        raise ValueError(f"{name}: caches must be [rows_max, {nkv}, S_max, {d}], got {tuple(k_cache.shape)} / "
                         f"{tuple(v_cache.shape)}")
    if (k_scale is None) != (v_scale is None):
        raise ValueError(f"{name}: pass both k_scale and v_scale (an FP8 cache), or neither")
    fp8 = torch.float8_e4m3fn
    if k_scale is None:
        if k_cache.dtype == fp8 or v_cache.dtype == fp8:
            raise ValueError(f"{name}: float8_e4m3fn caches need k_scale and v_scale")
        if k_cache.dtype != qkv.dtype or v_cache.dtype != qkv.dtype or not (k_cache.is_contiguous() and v_cache.is_contiguous()):
            raise ValueError(f"{name}: caches must be contiguous and of qkv's dtype")
    else:
        if k_cache.dtype != fp8 or v_cache.dtype != fp8 or not (k_cache.is_contiguous() and v_cache.is_contiguous()):
            raise ValueError(f"{name}: k_scale / v_scale were given, so k_cache and v_cache must be contiguous "
                             f"float8_e4m3fn tensors, got {k_cache.dtype} / {v_cache.dtype}")
        for what, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if t.dtype != torch.float32 or t.shape != k_cache.shape[:3] or not t.is_contiguous():
                raise ValueError(f"{name}: {what} must be a contiguous f32 tensor {tuple(k_cache.shape[:3])}, got "
                                 f"{t.dtype} {tuple(t.shape)}")
    for what, t in index.items():
        if t.dim() != 1 or t.numel() != qkv.shape[0] or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: {what} must be an integer tensor [{qkv.shape[0]}], got {t.dtype} {tuple(t.shape)}")


def _dequantized(cache, scale, dtype):
    """The cache an FP8 cache stands for, in `dtype` (exact in bf16); slots never written may hold anything."""
    return (cache.float() * scale[..., None]).to(dtype)


@torch.no_grad()
def kv_cache_append(qkv, k_cache, v_cache, pos, rows, nq, nkv, head_dim, cos=None, sin=None, pos_max=None,
                    row_max=None, k_scale=None, v_scale=None):
    """Rotate the q and k heads of the fused `qkv` [T, (nq + 2 nkv) * d] in place at `pos` (cos / sin
    given; None = already roped, as after `qk_norm_rope`) and write every token's k and v to
    cache[rows[t], :, pos[t], :].  Serves the packed prefill and a decode step alike.  Returns qkv.
    `pos` / `rows` are device tensors and are not read on the host.  A caller that knows them on the
    host passes `pos_max` / `row_max`, the largest position / row of the call: they are checked here
    against S_max, the tables and rows_max (models/generation.py does).  Without them a token outside
    the cache silently writes nothing.

    `k_scale` / `v_scale` (f32 [rows_max, nkv, S_max]; the caches are then float8_e4m3fn): every k (after
    RoPE) and v vector is quantised with its own power-of-two scale, `quantize_fp8_rows(pow2=True)` of the
    D-vector, and the dequantised vectors replace k and v in `qkv`, so attention over `qkv` (the prefill)
    sees exactly what the cache holds."""
    nq, nkv, d = int(nq), int(nkv), int(head_dim)
    _check_cache_args("kv_cache_append", qkv, k_cache, v_cache, nq, nkv, d, {"pos": pos, "rows": rows}, k_scale, v_scale)
    if (cos is None) != (sin is None):
        raise ValueError("kv_cache_append: pass both cos and sin, or neither")
    if cos is not None and (cos.dim() != 2 or cos.shape[1] != d // 2 or cos.shape != sin.shape):
        raise ValueError(f"kv_cache_append: tables must be [max_pos, {d // 2}]")
    if pos_max is not None and not 0 <= int(pos_max) < min(k_cache.shape[2], cos.shape[0] if cos is not None else 1 << 62):
        raise ValueError(f"kv_cache_append: position {int(pos_max)} outside the cache (S_max = {k_cache.shape[2]}) or the "
                         f"RoPE tables")
    if row_max is not None and not 0 <= int(row_max) < k_cache.shape[0]:
        raise ValueError(f"kv_cache_append: cache row {int(row_max)} outside [0, {k_cache.shape[0]})")
    pos, rows = pos.long(), rows.to(torch.int32)
    if _decode_kernels(qkv, nq, nq, d):  # the append has no group-size limit
        e = torch.empty(0, device=qkv.device)
        tail = (e if cos is None else cos, e if sin is None else sin, pos.contiguous(), rows.contiguous(), nq, nkv, d)
        if k_scale is None:
            ops.kv_cache_append_(qkv, k_cache, v_cache, *tail)
        else:
            ops.kv_cache_append_fp8_(qkv, k_cache, v_cache, k_scale, v_scale, *tail)
        return qkv
    T, h = qkv.shape[0], d // 2
    ok = (pos >= 0) & (pos < k_cache.shape[2]) & (rows >= 0) & (rows < k_cache.shape[0])
    if cos is not None:
        ok &= pos < cos.shape[0]
        p = pos.clamp(0, cos.shape[0] - 1)
        x = qkv[:, : (nq + nkv) * d].reshape(T, nq + nkv, d).float()
        c, s = cos[p][:, None, :], sin[p][:, None, :]
        x1, x2 = x[..., :h], x[..., h:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(T, (nq + nkv) * d).to(qkv.dtype)
        qkv[:, : (nq + nkv) * d] = torch.where(ok[:, None], rot, qkv[:, : (nq + nkv) * d])
    # boolean selection of the in-range tokens: one host sync, which this fallback path accepts
    r, p = rows.long()[ok], pos[ok]
    if k_scale is not None:
        for cache, scales, c0 in ((k_cache, k_scale, nq * d), (v_cache, v_scale, (nq + nkv) * d)):
            x = qkv[:, c0:c0 + nkv * d].reshape(T, nkv, d)[ok]
            codes, s = quantize_fp8_rows(x.reshape(-1, d).float())
            codes, s = codes.reshape(x.shape), s.reshape(x.shape[:2])
            cache.view(torch.uint8)[r, :, p] = codes.view(torch.uint8)
            scales[r, :, p] = s
            qkv[:, c0:c0 + nkv * d][ok] = _dequantized(codes, s, qkv.dtype).reshape(-1, nkv * d)
        return qkv
    k_cache[r, :, p] = qkv[:, nq * d:(nq + nkv) * d].reshape(T, nkv, d)[ok]
    v_cache[r, :, p] = qkv[:, (nq + nkv) * d:].reshape(T, nkv, d)[ok]
    return qkv


@torch.no_grad()
def decode_attention(qkv, k_cache, v_cache, rows, lens, nq, nkv, head_dim, max_len, scale=None, window=0, splits=0,
                     k_scale=None, v_scale=None):
    """Attention of one query token per sequence against its KV-cache row -> [B, nq * d].

    Row b's query heads are read out of the fused `qkv` row b and attend to keys
    [max(0, lens[b] - window), lens[b]) of cache row rows[b] (window 0 = all).  `lens` / `rows` stay on
    the device; `max_len` is a host upper bound of lens, used for the launch plan only.  `splits` > 0
    overrides the planned split-KV count.  `k_scale` / `v_scale`: the caches are float8_e4m3fn with one f32
    scale per key vector (see `kv_cache_append`); the kernel then returns, bit for bit, what it returns on the
    bf16 cache those stand for."""
    nq, nkv, d = int(nq), int(nkv), int(head_dim)
    _check_cache_args("decode_attention", qkv, k_cache, v_cache, nq, nkv, d, {"rows": rows, "lens": lens}, k_scale, v_scale)
    max_len, window, splits = int(max_len), int(window or 0), int(splits)
    if not 0 <= max_len <= k_cache.shape[2]:
        raise ValueError(f"decode_attention: max_len {max_len} outside [0, S_max = {k_cache.shape[2]}]")
    if window < 0 or splits < 0:
        raise ValueError("decode_attention: window and splits must not be negative")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if _decode_kernels(qkv, nq, nkv, d):
        rows, lens = rows.to(torch.int32).contiguous(), lens.to(torch.int32).contiguous()
        if k_scale is not None:
            return ops.decode_attn_fp8(qkv, k_cache, v_cache, k_scale, v_scale, rows, lens, 1, nq, nkv, d, float(scale),
                                       max_len, window, splits)
        return ops.decode_attn(qkv, k_cache, v_cache, rows, lens, nq, nkv, d, float(scale), max_len, window, splits)
    if k_scale is not None:
        k_cache, v_cache = _dequantized(k_cache, k_scale, qkv.dtype), _dequantized(v_cache, v_scale, qkv.dtype)
    B, g = qkv.shape[0], nq // nkv
    n = lens.long().clamp(0, max_len)
    r = rows.long()
    n = torch.where((r >= 0) & (r < k_cache.shape[0]), n, torch.zeros_like(n))
    r = r.clamp(0, k_cache.shape[0] - 1)
    j = torch.arange(max_len, device=qkv.device)
    keep = j[None] < n[:, None]
    if window > 0:
        keep &= j[None] >= (n - window)[:, None]
    q = qkv[:, : nq * d].reshape(B, nkv, g, d).float()
    # masked slots may hold anything (NaN included): zero them rather than multiply them by 0
    k = torch.where(keep[:, None, :, None], k_cache[r, :, :max_len].float(), torch.zeros((), device=qkv.device))
    v = torch.where(keep[:, None, :, None], v_cache[r, :, :max_len].float(), torch.zeros((), device=qkv.device))
    s = torch.einsum("bhgd,bhsd->bhgs", q, k) * float(scale)
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1).masked_fill(~keep[:, None, None, :], 0.0)  # a row without keys: 0, not NaN
    return torch.einsum("bhgs,bhsd->bhgd", p, v).reshape(B, nq * d).to(qkv.dtype)


@torch.no_grad()
def decode_attention_multi(qkv, k_cache, v_cache, rows, lens, q_len, nq, nkv, head_dim, max_len, scale=None, window=0,
                           splits=0, k_scale=None, v_scale=None):
    """Attention of `q_len` new tokens per sequence against its KV-cache row -> [B * q_len, nq * d]: the verify
    pass of speculative decoding.

    `qkv` is [B * q_len, ...] sequence-major (token t of sequence b is row b * q_len + t), `rows` [B] the cache
    rows, `lens` [B * q_len] one attended length per token: token (b, t) attends keys
    [max(0, len - window), len) of cache row rows[b]; len <= 0 or a row outside the cache gives a row of zeros.
    Causality among the new tokens is the caller's: it appends them first and passes pos + 1.  `max_len` and
    `splits` as in `decode_attention`.  At window 0 the kernel's output row of a token equals, bit for bit,
    `decode_attention` of that token alone with the same `max_len` and `splits`.  `k_scale` / `v_scale`: an FP8
    cache, as in `decode_attention`."""
    q_len, nq, nkv, d = int(q_len), int(nq), int(nkv), int(head_dim)
    if q_len < 1 or qkv.dim() != 2 or qkv.shape[0] % q_len:
        raise ValueError(f"decode_attention_multi: q_len ({q_len}) must be >= 1 and divide the rows of qkv "
                         f"{tuple(qkv.shape)}")
    _check_cache_args("decode_attention_multi", qkv, k_cache, v_cache, nq, nkv, d, {"lens": lens}, k_scale, v_scale)
    B = qkv.shape[0] // q_len
    if rows.dim() != 1 or rows.numel() != B or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"decode_attention_multi: rows must be an integer tensor [{B}] (one cache row per sequence), "
                         f"got {rows.dtype} {tuple(rows.shape)}")
    max_len, window, splits = int(max_len), int(window or 0), int(splits)
    if not 0 <= max_len <= k_cache.shape[2]:
        raise ValueError(f"decode_attention_multi: max_len {max_len} outside [0, S_max = {k_cache.shape[2]}]")
    if window < 0 or splits < 0:
        raise ValueError("decode_attention_multi: window and splits must not be negative")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if _decode_kernels(qkv, nq, nkv, d):
        rows, lens = rows.to(torch.int32).contiguous(), lens.to(torch.int32).contiguous()
        if k_scale is not None:
            return ops.decode_attn_fp8(qkv, k_cache, v_cache, k_scale, v_scale, rows, lens, q_len, nq, nkv, d,
                                       float(scale), max_len, window, splits)
        return ops.decode_attn_multi(qkv, k_cache, v_cache, rows, lens, q_len, nq, nkv, d, float(scale), max_len, window,
                                     splits)
    # decode_attention's composition (the same rule sends it there), one query row per token: masked slots zeroed
    return decode_attention(qkv, k_cache, v_cache, rows.repeat_interleave(q_len), lens, nq, nkv, d, max_len, scale, window,
                            splits, k_scale, v_scale)


# --------------------------------------------------------------------------------------------
# Sampling: fused top-k / top-p / min-p with a per-sequence Philox draw (csrc/kernels/sample.hip)
# --------------------------------------------------------------------------------------------
# DTG_SAMPLE_FUSED=0 composes the same definition from torch ops in f64 on the GPU (the CPU
# implementation's code run on the device: the kernel's A/B partner; it reads `rng` on the host when no
# `u` is given); so do, on a GPU, logits dtypes other than bf16 and f32.
_SAMPLE_FUSED = os.environ.get("DTG_SAMPLE_FUSED", "1") == "1"

_SAMPLE_RULES = {
    "temperature": (lambda v: v >= 0.0, "temperature >= 0"),
    "top_k": (lambda v: v >= 0, "top_k >= 0"),
    "top_p": (lambda v: 0.0 < v <= 1.0, "0 < top_p <= 1"),
    "min_p": (lambda v: 0.0 <= v <= 1.0, "0 <= min_p <= 1"),
}


def check_sample_scalar(name, v):
    """The host-side rule of one scalar sampling parameter (ValueError); NaN fails every rule."""
    ok, text = _SAMPLE_RULES[name]
    if not ok(v):
        raise ValueError(f"sample_logits: need {text}, got {name} = {v!r}")


def _sample_column(name, v, n, dtype, device):
    if isinstance(v, torch.Tensor):
        if v.dim() != 1 or v.shape[0] != n or v.device != device:
            raise ValueError(f"sample_logits: a tensor {name} must be [{n}] on the logits' device, got "
                             f"{tuple(v.shape)} on {v.device}")
        return v.to(dtype)
    if name in _SAMPLE_RULES:
        check_sample_scalar(name, v)
    if dtype == torch.int64:
        v = (int(v) + 2**63) % 2**64 - 2**63  # the 64 bits of the value, as int64
    return torch.full((n,), v, dtype=dtype, device=device)


@torch.no_grad()
def sample_logits(logits, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, stream=None, step=0, u=None):
    """One id per row of `logits` [n, V] -> (ids int64 [n], kept int32 [n]); `kept` is the size of the
    set the row was drawn from.  One kernel launch; nothing is read on the host.

    Every argument is a Python scalar (validated here, then broadcast) or a device tensor [n] (taken
    as is, never synced), so rows of one batch may mix greedy and sampled decoding, temperatures and
    filters.  `stream` defaults to the row index.  Per row, with x = float(logits) (NaN counts as
    -inf) and M = max x:

      * M = -inf: ids = -1, kept = 0.  M = +inf: the lowest index of a +inf, kept = their number.
      * temperature T <= 0 or NaN: greedy, the lowest index of M, kept = 1.
      * else weights w_i = exp((x_i - M) / T) and three value thresholds, each -inf when off:
          t_k (0 < top_k < V): the top_k-th largest x, with multiplicity; A = {x >= t_k}
          t_p (0 < top_p < 1): the largest value t of A with sum_{A, x >= t} w >= top_p * sum_A w
                               (top_p <= 0 keeps the entries equal to M; >= 1 or NaN is off)
          t_m (min_p > 0):     M + T ln(min_p), i.e. w >= min_p
        The kept set is K = {x >= max(t_k, t_p, t_m)}: ties at a cut are kept, and the argmax always
        is.  ids is the smallest i in K whose running sum of w over K in INDEX order exceeds
        u * sum_K w (the last index of K if rounding leaves none).
      * u = (word 0 of Philox4x32-10({step lo, step hi, stream lo, stream hi}, key {seed lo, seed hi})
        >> 8) * 2^-24, or the given `u` (f32 [n] in [0, 1)).

    A row's result depends on that row's logits and parameters alone -- not on the batch size, the
    row's place in it or the other rows -- and is bitwise the same from run to run."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"sample_logits: logits must be [n, V] with V >= 1, got {tuple(logits.shape)}")
    n, V = logits.shape
    dev = logits.device
    col = lambda name, v, dt: _sample_column(name, v, n, dt, dev)  # noqa: E731
    params = torch.stack([col("temperature", temperature, torch.float32), col("top_p", top_p, torch.float32),
                          col("min_p", min_p, torch.float32)], 1)
    k = col("top_k", top_k, torch.int32)
    if stream is None:
        stream = torch.arange(n, dtype=torch.int64, device=dev)
    rng = torch.stack([col("seed", seed, torch.int64), col("stream", stream, torch.int64),
                       col("step", step, torch.int64)], 1)
    if u is not None:
        u = col("u", u, torch.float32)
    if n and (logits.stride(1) != 1 or (n > 1 and logits.stride(0) < V)):
        logits = logits.contiguous()
    if logits.is_cuda and not (_SAMPLE_FUSED and logits.dtype in (torch.bfloat16, torch.float32)):
        from . import _cpu

        return _cpu.sample_logits(logits, params, k, rng, u)
    return ops.sample_logits(logits, params, k, rng, u)


# --------------------------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------------------------
class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return ops.swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dh):
        (gu,) = ctx.saved_tensors
        return ops.swiglu_bwd(dh.contiguous(), gu)


def swiglu(gu):
    return _SwiGLU.apply(gu)


# --------------------------------------------------------------------------------------------
# Skinny GEMM: the decode step's projections at M <= 16 rows (csrc/kernels/skinny_gemm.hip)
# --------------------------------------------------------------------------------------------
# Inference only (no autograd).  DTG_SKINNY_FUSED=0 composes the same function from torch.mm / addmm
# (hipBLASLt) and ops.swiglu: the kernel's A/B partner; so do, on a GPU, dtypes other than bf16.
_SKINNY_FUSED = os.environ.get("DTG_SKINNY_FUSED", "1") == "1"


def _skinny_args(name, x, w, b, act, wname="w"):
    """What skinny_linear and skinny_linear_fp8 (`name`) share in argument handling; returns act as 0 / 1 and
    the bias as [N] or None."""
    if act not in (None, 0, 1, "swiglu"):
        raise ValueError(f"{name}: act must be None or 'swiglu', got {act!r}")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"{name}: x [M, K] and {wname} [N, K] do not match: {tuple(x.shape)}, {tuple(w.shape)}")
    if x.shape[0] > SKINNY_MAX_M:
        raise ValueError(f"{name}: M = {x.shape[0]} rows exceed the kernel's limit of {SKINNY_MAX_M}")
    act = 1 if act in (1, "swiglu") else 0
    if act and w.shape[0] % 2:
        raise ValueError(f"{name}: the SwiGLU epilogue needs an even N, got {w.shape[0]}")
    return act, None if b is None else b.reshape(-1)


def _skinny_composed_tail(y, act):
    """The composed (DTG_SKINNY_FUSED=0) path after the rounded product y [M, N]: its SwiGLU when act."""
    if not act:
        return y
    inter = y.shape[1] // 2
    if inter % 8 == 0:
        return ops.swiglu_fwd(y)
    g, u = y[:, :inter].float(), y[:, inter:].float()  # widths the swiglu kernel does not take
    return (F.silu(g) * u).to(y.dtype)


@torch.no_grad()
def skinny_linear(x, w, b=None, act=None):
    """y = x @ w^T (+ b) for 1 <= M <= 16 rows of x [M, K]: the weight-streaming kernel of the decode
    step.  `w` is [N, K] (the nn.Linear layout), `b` [N] or None.  act = "swiglu" (or 1): `w` holds the
    gate rows, then the up rows (LlamaMLP.gate_up_proj); the result is swiglu(x @ w^T (+ b)), [M, N / 2],
    bitwise what `swiglu(skinny_linear(x, w, b))` returns, in one launch.  f32 accumulation in a fixed
    order that does not depend on M: a row's result is the same alone and inside a batch."""
    act, b = _skinny_args("skinny_linear", x, w, b, act)
    if x.is_cuda and not (_SKINNY_FUSED and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16):
        return _skinny_composed_tail(torch.mm(x, w.t()) if b is None else torch.addmm(b, x, w.t()), act)
    return ops.skinny_linear(x, w, b, act)


# --------------------------------------------------------------------------------------------
# Weight-only FP8 for the decode step (csrc/kernels/skinny_gemm.hip, the e4m3 weight format)
# --------------------------------------------------------------------------------------------
FP8_MAX = 448.0        # largest finite OCP e4m3fn magnitude
FP8_MIN_SCALE_EXP = -100  # scales are floored at 2^-100


def _pow2(k):
    """2^k as f32 for an integer tensor k in [-126, 127], built from the exponent bits: exact on every device."""
    return ((k.to(torch.int32) + 127) << 23).view(torch.float32)


@torch.no_grad()
def quantize_fp8_rows(w, pow2=True):
    """Per-row weight quantisation to OCP e4m3fn (load time, torch ops): `w` bf16 / f32 [N, K] ->
    (wq float8_e4m3fn [N, K] contiguous, scale f32 [N]) with w ~= float(wq) * scale[:, None].

    pow2=True (default): scale[n] is the power of two that puts the row's largest magnitude into
    (224, 448].  e4m3 is a floating-point format, so a power-of-two scale costs no relative precision, and
    float(wq) * scale is exactly representable in bf16: the quantised matrix is exactly some bf16 matrix.
    pow2=False: scale[n] = amax / 448.  An all-zero row gets scale 1; scales are floored at 2^-100.  torch's
    cast to float8_e4m3fn does not saturate (465 becomes NaN), so the quotient is clamped to +-448 first:
    the NaN codes 0x7f / 0xff are never emitted."""
    if w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"quantize_fp8_rows: w must be a bf16 or f32 [N, K] matrix, got {w.dtype} {tuple(w.shape)}")
    w32 = w.detach().float()
    amax = w32.abs().amax(dim=1) if w32.shape[1] else w32.new_zeros(w32.shape[0])
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_fp8_rows: w holds non-finite values")
    zero = amax == 0
    if pow2:
        # amax = m * 2^e with m in [0.5, 1); 448 = 0.875 * 2^9: m <= 0.875 -> amax / 2^(e - 9) in [256, 448],
        # else amax / 2^(e - 8) in (224, 256).  frexp is exact; the quotient is checked all the same and the
        # exponent moved by one step if it lies outside (224, 448].
        m, e = torch.frexp(amax)
        k = torch.where(m <= 0.875, e - 9, e - 8).to(torch.int32).clamp(FP8_MIN_SCALE_EXP, 127)
        top = amax / _pow2(k)
        k = torch.where(top > FP8_MAX, k + 1, torch.where((top <= FP8_MAX / 2) & ~zero, k - 1, k))
        scale = _pow2(k.clamp(FP8_MIN_SCALE_EXP, 127))
    else:
        scale = (amax / FP8_MAX).clamp_min(2.0 ** FP8_MIN_SCALE_EXP)
    scale = torch.where(zero, torch.ones_like(scale), scale)
    wq = (w32 / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous()
    return wq, scale.contiguous()


@torch.no_grad()
def skinny_linear_fp8(x, wq, scale, b=None, act=None):
    """y = (x @ float(wq)^T) * scale (+ b) for 1 <= M <= 16 bf16 rows of x [M, K]: `ops.skinny_linear` with
    the weights streamed as OCP e4m3fn bytes, `wq` float8_e4m3fn [N, K] and `scale` f32 [N] as
    `quantize_fp8_rows` returns them.  f32 accumulation in a fixed order that does not depend on M, one
    multiply by the scale after the reduction, then the bias, then one rounding.  act = "swiglu" (or 1) as
    in `skinny_linear`: bitwise `swiglu(skinny_linear_fp8(x, wq, scale, b))`, in one launch."""
    act, b = _skinny_args("skinny_linear_fp8", x, wq, b, act, wname="wq")
    if scale.dim() != 1 or scale.shape[0] != wq.shape[0]:
        raise ValueError(f"skinny_linear_fp8: scale must be [N = {wq.shape[0]}], got {tuple(scale.shape)}")
    if x.is_cuda and not _SKINNY_FUSED:
        y = torch.mm(x.float(), wq.float().t()) * scale
        if b is not None:
            y = y + b.float()
        return _skinny_composed_tail(y.to(x.dtype), act)
    return ops.skinny_linear_fp8(x, wq, scale, b, act)


def _mlp_backward(act, x, w1, w2, a, dy, b1=None, b2=None):
    """Backward of y = act(x @ w1^T (+ b1)) @ w2^T (+ b2) from the saved pre-activation a; `act`
    names the operators {act}_fwd / _bwd / _bwd_t.  Returns dx, dw1, dw2, db1, db2.

    h = act(a) is recomputed.  On the TN path the {act}_bwd_t kernel writes da together with da^T
    and h^T, the token-contiguous operands of the two weight-gradient GEMMs, so neither needs a
    separate transpose pass; the dX GEMMs use transposed weight copies (see _bwd_layout).  The
    parameters are routed in the order b2, w2, b1, w1 (the engines count notifications per bucket),
    and dh, h^T and h are dropped as soon as they are spent: they set the peak memory."""
    dy = dy.contiguous()
    dx_tn, dw_tn = _bwd_layout(x, w1)
    fused = dw_tn and _tn_ok(dy, a) and a.stride(0) == a.shape[1]
    db2 = None if b2 is None else _bias_grad(b2, dy)
    dh = _dx_mm(dy, w2, dx_tn)
    if fused:
        da, da_t, h_t = getattr(ops, act + "_bwd_t")(dh, a)
        del dh
        dw2 = _dw_mm(w2, dy, None, True, x_t=h_t)
        del h_t
    else:
        da_t = None
        h = getattr(ops, act + "_fwd")(a)
        da = getattr(ops, act + "_bwd")(dh, a)
        del dh
        dw2 = _dw_mm(w2, dy, h, False)
        del h
    db1 = None if b1 is None else _bias_grad(b1, da)
    dx = _dx_mm(da, w1, dx_tn)
    dw1 = _dw_mm(w1, da, x, fused, dy_t=da_t)
    return dx, dw1, dw2, db1, db2


class _SwiGLUMLP(torch.autograd.Function):
    """down(swiglu(x @ W_gu^T)) as one autograd node.  Saves only x and gu
    ([T, I] less resident per layer than with h); the backward is _mlp_backward."""

    @staticmethod
    def forward(ctx, x, w_gu, w_down, out=None):
        gu = torch.mm(x, w_gu.t())
        h = ops.swiglu_fwd(gu)
        ctx.save_for_backward(x, w_gu, w_down, gu)
        if out is not None:
            return torch.mm(h, w_down.t(), out=out[0])
        return torch.mm(h, w_down.t())

    @staticmethod
    def backward(ctx, dy):
        x, w_gu, w_down, gu = ctx.saved_tensors
        dx, dw_gu, dw_down, _, _ = _mlp_backward("swiglu", x, w_gu, w_down, gu, dy)
        return dx, dw_gu, dw_down, None


def swiglu_mlp(x, w_gu, w_down, out=None):
    """Llama MLP: down_proj(silu(gate(x)) * up(x)) with the fused [gate; up] weight.  `out`: see
    `linear`."""
    return _SwiGLUMLP.apply(x, w_gu, w_down, None if out is None else (out,))


# --------------------------------------------------------------------------------------------
# GELU MLP (GPT-2)
# --------------------------------------------------------------------------------------------
class _GeluMLP(torch.autograd.Function):
    """proj(gelu_tanh(x @ W_fc^T + b_fc)) + b_proj as one autograd node.  Saves x and the
    pre-activation a; the backward is _mlp_backward, so the transposes _LinearBias would spend
    around the GELU never run.  The bias gradients are f32 column sums as in _LinearBias."""

    @staticmethod
    def forward(ctx, x, w_fc, b_fc, w_proj, b_proj):
        a = torch.addmm(b_fc, x, w_fc.t())
        h = ops.gelu_fwd(a)
        ctx.save_for_backward(x, w_fc, b_fc, w_proj, b_proj, a)
        return torch.addmm(b_proj, h, w_proj.t())

    @staticmethod
    def backward(ctx, dy):
        x, w_fc, b_fc, w_proj, b_proj, a = ctx.saved_tensors
        dx, dw_fc, dw_proj, db_fc, db_proj = _mlp_backward("gelu", x, w_fc, w_proj, a, dy, b_fc, b_proj)
        return dx, dw_fc, db_fc, dw_proj, db_proj


def gelu_mlp(x, w_fc, b_fc, w_proj, b_proj):
    """GPT-2 MLP: c_proj(gelu_tanh(c_fc(x))), both projections with bias."""
    return _GeluMLP.apply(x, w_fc, b_fc, w_proj, b_proj)


# --------------------------------------------------------------------------------------------
# Embedding
# --------------------------------------------------------------------------------------------
class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, w):
        ctx.save_for_backward(ids)
        ctx.w = w
        return F.embedding(ids, w)

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        w = ctx.w
        return None, route_embedding_grad(w, ids, dy.contiguous(), w.shape[0])


def embedding(ids, w):
    return _Embedding.apply(ids, w)


# --------------------------------------------------------------------------------------------
# Fused lm_head + causal-LM cross entropy (chunked; logits never materialised whole)
# --------------------------------------------------------------------------------------------
def _default_chunk(vocab, hidden_rows):
    """Rows per chunk: ~1 GiB of bf16 logits (DTG_CE_CHUNK_GIB), split evenly over the rows
    (16,384 rows x 128,256 vocab -> 4 x 4,096), a multiple of 64 rows (transposable, MFMA-tile
    aligned), >= 1024."""
    gib = float(os.environ.get("DTG_CE_CHUNK_GIB", "1"))
    n = max(1, -(-hidden_rows * max(vocab, 1) // max(1, int(gib * (1 << 29)))))
    per = -(-hidden_rows // n)
    return max(1024, min(hidden_rows, -(-per // 64) * 64))


def _ce_tn(h, w):
    """Use K-contiguous (TN) operands for the loss head's dX / dW GEMMs (see _bwd_layout)."""
    return _LINEAR_BWD != "native" and _tn_ok(h, w)


def _ce_dx(logits, w, w_t, out):
    """out = logits @ w, as logits @ (w^T)^T when a contiguous w^T is given."""
    if w_t is not None:
        torch.mm(logits, w_t.t(), out=out)
    else:
        torch.mm(logits, w, out=out)


class _FusedLinearCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, labels, ignore_index, num_valid, chunk):
        T = h.shape[0]
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        scale = 1.0 / max(num_valid, 1)
        loss_sum = torch.zeros((), dtype=torch.float32, device=h.device)
        dh = torch.empty_like(h) if need else None
        want_dw = need and ctx.needs_input_grad[1]
        # direct: dW goes straight into w.main_grad now (engine-owned loss, grad_output == 1)
        direct = want_dw and _gr.direct_loss_grad() and getattr(w, "main_grad", None) is not None
        dw = torch.empty(w.shape, dtype=w.dtype, device=h.device) if (want_dw and not direct) else None
        # A vocabulary that is not a multiple of 8 (GPT-2 50,257, the rime 156,939) leaves every
        # logits row, and the transposed weight, 16-B misaligned: hipBLASLt then drops to slower
        # kernels and the TN layout cannot be used at all.  Pad the weight with zero rows to the
        # next multiple of 8: the padded logits columns are exactly 0, the CE kernel sees only the
        # first V columns (strided view) and leaves the pad at 0, so the GEMMs over the padded K
        # add nothing.  One 1-GB copy per step for the rime head.
        V = w.shape[0]
        pad = (-V) % 8 if (need and h.is_cuda and _LINEAR_BWD != "native" and chunk % 8 == 0
                           and _tn_ok(h)) else 0
        wp = w
        if pad:
            wp = torch.zeros((V + pad, w.shape[1]), dtype=w.dtype, device=w.device)
            wp[:V].copy_(w.detach())
        tn = need and _ce_tn(h, wp) and chunk % 8 == 0
        w_t = (_wt(w) if wp is w else ops.transpose2d(wp)) if (tn and ctx.needs_input_grad[0]) else None
        for s in range(0, T, chunk):
            e = min(T, s + chunk)
            lp = torch.mm(h[s:e], wp.t())
            logits = lp[:, :V] if pad else lp
            rows = ops.ce_fwd_bwd_(logits, labels[s:e], ignore_index, scale, need)
            loss_sum += rows.sum()
            if need:
                _ce_dx(lp, wp, w_t, dh[s:e])
                if direct and tn:
                    _gr.accumulate_mm_into_main_grad(w, logits, h[s:e], a_t=ops.transpose2d(lp)[:V],
                                                     b_t=ops.transpose2d(h[s:e]))
                elif direct:
                    _gr.accumulate_mm_into_main_grad(w, logits, h[s:e])
                elif dw is not None:
                    # f32 accumulate inside the GEMM, one bf16 rounding per chunk
                    if s == 0:
                        torch.mm(logits.t(), h[s:e], out=dw)
                    else:
                        dw.addmm_(logits.t(), h[s:e])
        ctx.save_for_backward(dh, dw)
        ctx.w = w
        ctx.direct = direct
        return loss_sum * scale

    @staticmethod
    def backward(ctx, go):
        dh, dw = ctx.saved_tensors
        w = ctx.w
        if ctx.direct:
            _gr.notify_param(w)
            return dh, None, None, None, None, None
        gdh = (dh * go.to(dh.dtype)) if ctx.needs_input_grad[0] else None
        gdw = route_param_grad(w, dw * go.to(dw.dtype)) if dw is not None else None
        return gdh, gdw, None, None, None, None


def fused_linear_cross_entropy(h, w, labels, ignore_index=-100, num_valid=None, chunk=None):
    """mean CE of softmax(h @ w^T) vs labels over rows with label != ignore_index.

    `labels` are already shifted (label of row i = token i+1).  `num_valid` (host int) avoids a
    device sync; if None it is computed (one sync)."""
    if num_valid is None:
        num_valid = int((labels != ignore_index).sum().item())
    if chunk is None:
        chunk = _default_chunk(w.shape[0], h.shape[0])
    return _FusedLinearCE.apply(h, w, labels, ignore_index, int(num_valid), int(chunk))


class _VocabParallelFusedLinearCE(torch.autograd.Function):
    """lm_head sharded over the vocabulary across `group` (tensor parallel); h is replicated.

    Per chunk: local logits -> per-row (max, sum-exp, target logit) -> ONE all-gather of those
    [3, rows] stats over the TP group -> global log-sum-exp -> local softmax gradient in place
    (SURVEY C12/K13).  The chunk loop is software-pipelined: chunk j's stats all-gather is in
    flight (async, RCCL's stream) while chunk j+1's logits GEMM and stats kernel run, and only
    then does chunk j's gradient pass wait for it -- no collective sits between the GEMMs.  The
    weight gradient uses K-contiguous (TN) operands and, with an engine-owned loss, accumulates
    straight into `main_grad` (no [V/tp, H] temporary).  The returned dh is this rank's
    vocab-shard PARTIAL; the caller's TP-region entry (sequence all-gather, whose backward is a
    reduce-scatter) sums it across ranks."""

    @staticmethod
    def forward(ctx, h, w, labels, ignore_index, num_valid, chunk, vocab_start, group):
        from ..utils import comm as _comm

        T = h.shape[0]
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        scale = 1.0 / max(num_valid, 1)
        loss_sum = torch.zeros((), dtype=torch.float32, device=h.device)
        dh = torch.empty_like(h) if need else None
        want_dw = need and ctx.needs_input_grad[1]
        direct = want_dw and _gr.direct_loss_grad() and getattr(w, "main_grad", None) is not None
        dw = torch.empty(w.shape, dtype=w.dtype, device=h.device) if (want_dw and not direct) else None
        tn = need and _ce_tn(h, w) and chunk % 8 == 0 and w.shape[0] % 8 == 0
        w_t = _wt(w) if (tn and ctx.needs_input_grad[0]) else None

        def issue(s, e):
            logits = torch.mm(h[s:e], w.t())
            m, sx, xl = ops.ce_stats(logits, labels[s:e], vocab_start)
            stats, work = _comm.all_gather_stack_async(torch.stack([m, sx, xl]), group)
            return s, e, logits, stats, work

        def finish(s, e, logits, stats, work):
            nonlocal loss_sum
            work.wait()
            gm = stats[:, 0].amax(0)
            sx = (stats[:, 1] * torch.exp(stats[:, 0] - gm)).sum(0)
            lse = gm + torch.log(sx)
            lab = labels[s:e]
            valid = lab != ignore_index
            loss_sum += torch.where(valid, lse - stats[:, 2].sum(0), torch.zeros_like(lse)).sum()
            if not need:
                return
            ops.ce_grad_(logits, lab, lse.contiguous(), vocab_start, ignore_index, scale)
            _ce_dx(logits, w, w_t, dh[s:e])
            if not want_dw:
                return
            a_t = ops.transpose2d(logits) if tn else None
            b_t = ops.transpose2d(h[s:e]) if tn else None
            if direct:
                _gr.accumulate_mm_into_main_grad(w, logits, h[s:e], a_t=a_t, b_t=b_t)
            else:
                lhs, rhs = (a_t, b_t.t()) if tn else (logits.t(), h[s:e])
                if s == 0:  # f32 accumulate inside the GEMM, one bf16 rounding per chunk
                    torch.mm(lhs, rhs, out=dw)
                else:
                    dw.addmm_(lhs, rhs)

        pend = None
        for s in range(0, T, chunk):
            cur = issue(s, min(T, s + chunk))  # GEMM j+1 overlaps the stats gather of chunk j
            if pend is not None:
                finish(*pend)
            pend = cur
        if pend is not None:
            finish(*pend)
        ctx.save_for_backward(dh, dw)
        ctx.w = w
        ctx.direct = direct
        return loss_sum * scale

    @staticmethod
    def backward(ctx, go):
        dh, dw = ctx.saved_tensors
        if ctx.direct:
            _gr.notify_param(ctx.w)
            return dh, None, None, None, None, None, None, None
        gdh = dh * go.to(dh.dtype) if ctx.needs_input_grad[0] else None
        gdw = route_param_grad(ctx.w, dw * go.to(dw.dtype)) if dw is not None else None
        return gdh, gdw, None, None, None, None, None, None


def vocab_parallel_fused_linear_cross_entropy(h, w_local, labels, vocab_start, group, ignore_index=-100,
                                              num_valid=None, chunk=None):
    if num_valid is None:
        num_valid = int((labels != ignore_index).sum().item())
    if chunk is None:
        chunk = _default_chunk(w_local.shape[0], h.shape[0])
    return _VocabParallelFusedLinearCE.apply(h, w_local, labels, ignore_index, int(num_valid), int(chunk),
                                             int(vocab_start), group)
