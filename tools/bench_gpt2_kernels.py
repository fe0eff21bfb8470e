#!/usr/bin/env python3
"""The GPT-2 streaming kernels (layernorm.hip, gelu.hip) at the chapter-01 training shape
(16,384 tokens, n_embd 768, n_inner 3072): achieved HBM bandwidth from timed launches and the
bytes each kernel must move, next to rmsnorm_bwd and swiglu_bwd_t at the same byte counts.

    python tools/bench_gpt2_kernels.py [--tokens 16384]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timeit(torch, fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--inter", type=int, default=3072)
    a = ap.parse_args()
    import torch

    import dtg.ops  # noqa: F401

    ops = torch.ops.dtg
    dev = torch.device("cuda")
    T, H, I = a.tokens, a.hidden, a.inter
    bf = dict(device=dev, dtype=torch.bfloat16)
    x, res, dy = (torch.randn(T, H, **bf) for _ in range(3))
    w, b = torch.ones(H, **bf), torch.zeros(H, **bf)
    rng = torch.tensor([1234, 8], dtype=torch.int64, device=dev)
    _, h, mean, rstd = ops.dropout_add_layernorm_fwd(x, res, w, b, 1e-5, 0.0, None)
    _, hr, rrstd = ops.add_rmsnorm_fwd(x, res, w, 1e-5)
    a_fc, dh = torch.randn(T, I, **bf), torch.randn(T, I, **bf)
    I2 = 5 * I // 8 // 8 * 8  # swiglu_bwd_t moves 8 T I2 elements: the 5 T I of gelu_bwd_t
    gu, dh2 = torch.randn(T, 2 * I2, **bf), torch.randn(T, I2, **bf)
    E = 2
    cases = {
        "layernorm_fwd": (lambda: ops.layernorm_fwd(x, w, b, 1e-5), 2 * T * H * E),
        "dropout_add_layernorm_fwd p=0": (lambda: ops.dropout_add_layernorm_fwd(x, res, w, b, 1e-5, 0.0, None), 4 * T * H * E),
        "dropout_add_layernorm_fwd p=0.1": (lambda: ops.dropout_add_layernorm_fwd(x, res, w, b, 1e-5, 0.1, rng), 4 * T * H * E),
        "add_rmsnorm_fwd": (lambda: ops.add_rmsnorm_fwd(x, res, w, 1e-5), 4 * T * H * E),
        "layernorm_bwd": (lambda: ops.layernorm_bwd(dy, h, w, mean, rstd, None, 0.0, None), 3 * T * H * E),
        "layernorm_bwd(+dres)": (lambda: ops.layernorm_bwd(dy, h, w, mean, rstd, dy, 0.0, None), 4 * T * H * E),
        "layernorm_bwd(+dres) p=0.1": (lambda: ops.layernorm_bwd(dy, h, w, mean, rstd, dy, 0.1, rng), 5 * T * H * E),
        "rmsnorm_bwd(+dres)": (lambda: ops.rmsnorm_bwd(dy, hr, w, rrstd, dy), 4 * T * H * E),
        "gelu_fwd": (lambda: ops.gelu_fwd(a_fc), 2 * T * I * E),
        "gelu_bwd": (lambda: ops.gelu_bwd(dh, a_fc), 3 * T * I * E),
        "gelu_bwd_t (dx, dx^T, h^T)": (lambda: ops.gelu_bwd_t(dh, a_fc), 5 * T * I * E),
        f"swiglu_bwd_t (I = {I2})": (lambda: ops.swiglu_bwd_t(dh2, gu), 8 * T * I2 * E),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        ms = timeit(torch, fn)
        out[name] = {"us": round(ms * 1e3, 1), "MB": round(nbytes / 1e6, 1), "TB/s": round(nbytes / ms / 1e9, 2)}
        print(f"{name:36s} {ms * 1e3:8.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / ms / 1e9:6.2f} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
