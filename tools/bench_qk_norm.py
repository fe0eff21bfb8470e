#!/usr/bin/env python3
"""The fused per-head QK RMSNorm + RoPE kernels (csrc/kernels/qk_norm.hip) against the composed
torch path (DTG_QKNORM_FUSED=0), forward and backward, at the Qwen3-0.6B and Qwen3-8B attention
shapes (T = 16 x 1024 tokens): time per call and the bandwidth reached on the bytes the function must
move -- forward: read q|k, write q|k, write the saved pre-norm copy; backward: read the gradient,
read the saved copy, write dx (3 T (nq + nkv) D bf16 values each way; rstd, the tables and the dw
partials are below 2 % of that).  The composed path is rated on the same byte count, so its figure
says how far its extra passes put it from the function's own traffic.

    python tools/bench_qk_norm.py [--tokens 16384]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = {"qwen3-0.6b": (16, 8, 128), "qwen3-8b": (32, 8, 128)}


def timeit(torch, fn, iters=30):
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
    a = ap.parse_args()
    import torch

    from dtg import ops
    from dtg.ops import functional

    raw = torch.ops.dtg
    dev = torch.device("cuda")
    T = a.tokens
    out = {}
    for name, (nq, nkv, D) in SHAPES.items():
        nh, C = nq + nkv, (nq + 2 * nkv) * D
        bf = dict(device=dev, dtype=torch.bfloat16)
        qkv, dqkv = torch.randn(T, C, **bf), torch.randn(T, C, **bf)
        wq, wk = (torch.rand(D, **bf) + 0.5).requires_grad_(), (torch.rand(D, **bf) + 0.5).requires_grad_()
        cos, sin = ops.rope_tables(D, 1e6, 4096, device=dev)
        pos = torch.arange(1024, device=dev).repeat(T // 1024 + 1)[:T].contiguous()
        nbytes = 3 * T * nh * D * 2
        xqk, rstd = raw.qk_norm_rope_fwd_(qkv.clone(), wq.detach(), wk.detach(), cos, sin, pos, nq, nkv, D, 1e-6)

        def fwd_bwd(x):
            x.grad = wq.grad = wk.grad = None
            y = ops.qk_norm_rope(x, wq, wk, 1e-6, nq, nkv, D, cos, sin, pos, grad_inplace=True)
            y.backward(dqkv)

        def composed_fwd():
            with torch.no_grad():
                ops.qk_norm_rope(qkv, wq, wk, 1e-6, nq, nkv, D, cos, sin, pos)

        res = {}
        # the in-place kernels keep renormalising the same buffers: values stay finite, timing is unaffected
        res["fused fwd"] = timeit(torch, lambda: raw.qk_norm_rope_fwd_(qkv, wq.detach(), wk.detach(), cos, sin, pos, nq,
                                                                       nkv, D, 1e-6))
        res["fused bwd"] = timeit(torch, lambda: raw.qk_norm_rope_bwd_(dqkv, xqk, rstd, wq.detach(), wk.detach(), cos,
                                                                       sin, pos, nq, nkv, D))
        qkv, dqkv = torch.randn(T, C, **bf), torch.randn(T, C, **bf)
        functional._QKNORM_FUSED = False
        try:
            res["composed fwd"] = timeit(torch, composed_fwd)
            x = qkv.clone().requires_grad_()
            res["composed bwd"] = timeit(torch, lambda: fwd_bwd(x)) - res["composed fwd"]
        finally:
            functional._QKNORM_FUSED = True
        res["rope_ alone (q|k, in place)"] = timeit(torch, lambda: raw.rope_(qkv, cos, sin, pos, nh, D, False))
        out[name] = {}
        for k, ms in res.items():
            nb = 2 * T * nh * D * 2 if k.startswith("rope_") else nbytes
            out[name][k] = {"us": round(ms * 1e3, 1), "MB": round(nb / 1e6, 1), "TB/s": round(nb / ms / 1e9, 2)}
            print(f"{name:11s} {k:30s} {ms * 1e3:9.1f} us  {nb / 1e6:8.1f} MB  {nb / ms / 1e9:6.2f} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
