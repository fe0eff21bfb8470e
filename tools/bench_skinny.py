#!/usr/bin/env python3
"""ops.skinny_linear (csrc/kernels/skinny_gemm.hip) and ops.skinny_linear_fp8 (the same kernel, weight-only
e4m3) against hipBLASLt (torch.mm / addmm, + ops.swiglu for the gate_up projection) in the same process, at
the decode-step projection shapes of Llama-3-8B and M = 1, 4, 8, 16 rows: time per call from HIP events and
the rate at which the weight bytes are consumed (the FP8 arm's GB/s counts its one-byte weights).

Every call of a timing takes the next of `copies` distinct weight buffers, enough that the set exceeds
the 256 MB Infinity Cache (--min-set-mb), so a weight is never re-read from a cache and the figure is an
HBM rate (profiles/r7/decode/README.md explains the trap); the FP8 arm has its own, more numerous, buffers
for the same total.  The three paths alternate; each keeps the better median.  Needs a GPU.

    python tools/bench_skinny.py [--md OUT.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# name -> (N, K, SwiGLU epilogue)
SHAPES = {"qkv": (6144, 4096, False), "o": (4096, 4096, False), "gate_up": (28672, 4096, True),
          "down": (4096, 14336, False), "head": (128256, 4096, False)}
MS = (1, 4, 8, 16)


def time_ms(torch, fn, min_ms, rounds=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    iters = max(3, min(2000, int(min_ms / max(s.elapsed_time(e), 1e-3)) + 1))
    ts = []
    for _ in range(rounds):
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / iters)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=100.0)
    ap.add_argument("--min-set-mb", type=float, default=640.0, help="total size of the rotated weight buffers")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny: needs a GPU")
    import dtg  # noqa: F401
    from dtg import ops

    dev = torch.device("cuda:0")
    out = []
    for name, (N, K, act) in SHAPES.items():
        wbytes = N * K * 2
        copies = max(2, int(a.min_set_mb * 1e6 / wbytes) + 1)
        ws = [(torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        copies8 = max(2, int(a.min_set_mb * 1e6 / (N * K)) + 1)
        w8 = [ops.quantize_fp8_rows(ws[j % copies]) for j in range(copies8)]  # distinct buffers, values repeat
        for M in MS:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            i = [0]

            def kernel():
                i[0] = (i[0] + 1) % copies
                return ops.skinny_linear(x, ws[i[0]], None, act="swiglu" if act else None)

            def fp8():
                i[0] = (i[0] + 1) % copies8
                return ops.skinny_linear_fp8(x, w8[i[0]][0], w8[i[0]][1], None, act="swiglu" if act else None)

            def blas():
                i[0] = (i[0] + 1) % copies
                y = torch.mm(x, ws[i[0]].t())
                return ops.swiglu(y) if act else y

            res = {}
            for which, fn in (("kernel", kernel), ("fp8", fp8), ("blas", blas)) * 2:
                t = time_ms(torch, fn, a.min_ms)
                res[which] = min(res.get(which, t), t)
            r = {"proj": name, "N": N, "K": K, "M": M, "copies": copies, "kernel_us": round(res["kernel"] * 1e3, 1),
                 "blas_us": round(res["blas"] * 1e3, 1), "kernel_GBps": round(wbytes / res["kernel"] / 1e6, 1),
                 "blas_GBps": round(wbytes / res["blas"] / 1e6, 1), "blas_over_kernel": round(res["blas"] / res["kernel"], 2),
                 "fp8_copies": copies8, "fp8_us": round(res["fp8"] * 1e3, 1),
                 "fp8_GBps": round(N * K / res["fp8"] / 1e6, 1), "kernel_over_fp8": round(res["kernel"] / res["fp8"], 2)}
            print(json.dumps(r), flush=True)
            out.append(r)
        del ws, w8
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fp:
            fp.write("| projection | N x K | M | bf16 kernel µs | fp8 kernel µs | hipBLASLt µs | bf16 kernel GB/s (weights) | "
                     "fp8 kernel GB/s (fp8 bytes) | hipBLASLt GB/s | hipBLASLt / bf16 kernel | bf16 kernel / fp8 kernel |\n")
            fp.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in out:
                fp.write(f"| {r['proj']} | {r['N']} x {r['K']} | {r['M']} | {r['kernel_us']} | {r['fp8_us']} | {r['blas_us']} | "
                         f"{r['kernel_GBps']} | {r['fp8_GBps']} | {r['blas_GBps']} | {r['blas_over_kernel']} | "
                         f"{r['kernel_over_fp8']} |\n")


if __name__ == "__main__":
    main()
