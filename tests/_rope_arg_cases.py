"""Argument cases of the four operators that take RoPE tables (rope_, kv_cache_append_, qk_norm_rope_fwd_,
flash_attn_bwd_qkv_rope): their host wrappers share the checks of csrc/kernels/rope_common.h, so one
table of perturbations applies to all of them.  Each perturbation breaks exactly one thing the kernels
rely on (16-byte vector accesses on qkv, 32-byte loads from contiguous f32 tables on the GPU, one int64
position per token); the wrapper must refuse it, naming itself, before anything is launched.
"""
import torch

import dtg.ops  # noqa: F401  (defines torch.ops.dtg)

T, NQ, NKV, MAX_POS = 2, 2, 1, 4
DIMS = (64, 128)
ROWS_MAX, S_MAX = 2, 4
SENTINEL = 0x4B4B  # bf16 bits of the caches


def valid_args(D, dev):
    """Arguments every operator accepts; the operators pick what they need."""
    g = torch.Generator().manual_seed(D)
    bf = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)  # noqa: E731
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    kc = torch.full((ROWS_MAX, NKV, S_MAX, D), SENTINEL, dtype=torch.int16).view(torch.bfloat16).to(dev)
    return dict(
        D=D, qkv=bf(T, (NQ + 2 * NKV) * D), cos=fr.cos().float().to(dev), sin=fr.sin().float().to(dev),
        pos=torch.tensor([1, MAX_POS - 1], device=dev), rows=torch.tensor([0, 1], dtype=torch.int32, device=dev),
        kc=kc, vc=kc.clone(), wq=bf(D), wk=bf(D), dout=bf(T, NQ, D), o=bf(T, NQ, D),
        lse=torch.zeros(NQ, T, device=dev), cu=torch.tensor([0, T], dtype=torch.int32, device=dev))


def _misaligned(qkv):
    buf = torch.zeros(qkv.numel() + 8, dtype=qkv.dtype, device=qkv.device)
    view = buf[1:1 + qkv.numel()].view(qkv.shape)
    view.copy_(qkv)
    assert view.data_ptr() % 16 == 2 and view.stride() == qkv.stride()
    return view


def _inner_stride_2(qkv):
    buf = torch.zeros(qkv.size(0), 2 * qkv.size(1), dtype=qkv.dtype, device=qkv.device)
    view = buf[:, ::2]
    view.copy_(qkv)
    assert view.stride() == (2 * qkv.size(1), 2) and view.shape == qkv.shape
    return view


def _both(f):
    return lambda a: dict(cos=f(a["cos"]), sin=f(a["sin"]))


# name -> the arguments it replaces
PERTURBATIONS = {
    "tables_on_cpu": _both(lambda t: t.cpu()),
    "tables_1d": _both(lambda t: t.reshape(-1)),
    "tables_f64": _both(lambda t: t.double()),
    "table_width": lambda a: dict(cos=a["cos"][:, : a["D"] // 2 - 8].contiguous(),
                                  sin=a["sin"][:, : a["D"] // 2 - 8].contiguous()),
    "sin_one_row_short": lambda a: dict(sin=a["sin"][:-1]),
    "pos_int32": lambda a: dict(pos=a["pos"].int()),
    "pos_too_long": lambda a: dict(pos=torch.zeros(T + 1, dtype=torch.long, device=a["pos"].device)),
    "qkv_misaligned_base": lambda a: dict(qkv=_misaligned(a["qkv"])),
    "qkv_inner_stride_2": lambda a: dict(qkv=_inner_stride_2(a["qkv"])),
}

_ops = torch.ops.dtg
OPERATORS = {
    "rope_": lambda a: _ops.rope_(a["qkv"], a["cos"], a["sin"], a["pos"], NQ + NKV, a["D"], False),
    "kv_cache_append_": lambda a: _ops.kv_cache_append_(a["qkv"], a["kc"], a["vc"], a["cos"], a["sin"], a["pos"],
                                                        a["rows"], NQ, NKV, a["D"]),
    "qk_norm_rope_fwd_": lambda a: _ops.qk_norm_rope_fwd_(a["qkv"], a["wq"], a["wk"], a["cos"], a["sin"], a["pos"],
                                                          NQ, NKV, a["D"], 1e-6),
    "flash_attn_bwd_qkv_rope": lambda a: _ops.flash_attn_bwd_qkv_rope(
        a["dout"], a["qkv"], NQ, NKV, a["D"], a["o"], a["lse"], a["cu"], T, a["D"] ** -0.5, True, a["cos"], a["sin"],
        a["pos"], 0),
}


def storage_bits(t):
    """Every element of the buffer `t` is a view of, as int16 on the CPU."""
    n = t.untyped_storage().nbytes() // t.element_size()
    return torch.as_strided(t, (n,), (1,), 0).cpu().view(torch.int16).clone()
