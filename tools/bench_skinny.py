#!/usr/bin/env python3
"""ops.skinny_linear (csrc/kernels/skinny_gemm.hip), ops.skinny_linear_fp8 (the same kernel, weight-only
e4m3), ops.skinny_linear_mfma (csrc/kernels/skinny_mfma.hip), ops.skinny_linear_mxfp4 (weight-only MXFP4,
csrc/kernels/skinny_mfma.hip) and ops.skinny_linear_mxfp4_a8 (W4A8 on the same MXFP4 buffers: the activation
quantiser plus the GEMM, "a8", and the GEMM alone on rows quantised outside the clock, "a8 gemm") against hipBLASLt (torch.mm / addmm, +
ops.swiglu for the gate_up projection) in the same process, at the decode-step projection shapes of Llama-3-8B
(and the two narrow ones of Llama-3.2-1B and Qwen3-0.6B) and M = 1, 4, 8, 16, 32, 64 rows: time per call from
HIP events and the rate at which the weight bytes are consumed (the FP8 arm's GB/s counts its one-byte
weights, the MXFP4 arm's its 17 bytes per 32 weights).  The fmaf arms (bf16 and fp8) stop at their 16-row limit.

Every call of a timing takes the next of `copies` distinct weight buffers, enough that the set exceeds
the 256 MB Infinity Cache (--min-set-mb), so a weight is never re-read from a cache and the figure is an
HBM rate (profiles/r7/decode/README.md explains the trap); the FP8 and MXFP4 arms have their own, more numerous,
buffers for the same total.  The paths alternate; each keeps the better of its two medians, and the gap between
the two (relative to the better) is reported as the arm's spread for the MXFP4 and FP8 arms: call one faster only
when the gap between them exceeds both spreads.  Needs a GPU.

    python tools/bench_skinny.py [--md OUT.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# name -> (N, K, SwiGLU epilogue)
SHAPES = {"qkv": (6144, 4096, False), "o": (4096, 4096, False), "gate_up": (28672, 4096, True),
          "down": (4096, 14336, False), "head": (128256, 4096, False),
          "o-1b": (2048, 2048, False), "down-0.6b": (1024, 3072, False)}
MS = (1, 4, 8, 16, 32, 64)
FMAF_MAX_M = 16


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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny: needs a GPU")
    import dtg  # noqa: F401
    from dtg import ops

    dev = torch.device("cuda:0")
    out = []
    for name in a.shapes.split(","):
        N, K, act = SHAPES[name]
        wbytes = N * K * 2
        copies = max(2, int(a.min_set_mb * 1e6 / wbytes) + 1)
        ws = [(torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        copies8 = max(2, int(a.min_set_mb * 1e6 / (N * K)) + 1)
        w8 = [ops.quantize_fp8_rows(ws[j % copies]) for j in range(copies8)]  # distinct buffers, values repeat
        mxbytes = N * K * 17 // 32  # codes and block scales
        copies4 = max(2, int(a.min_set_mb * 1e6 / mxbytes) + 1)
        w4 = [ops.quantize_mxfp4_rows(ws[j % copies]) for j in range(copies4)]
        for M in map(int, a.ms.split(",")):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            i = [0]

            def kernel():
                i[0] = (i[0] + 1) % copies
                return ops.skinny_linear(x, ws[i[0]], None, act="swiglu" if act else None)

            def mfma():
                i[0] = (i[0] + 1) % copies
                return ops.skinny_linear_mfma(x, ws[i[0]], None, act="swiglu" if act else None)

            def fp8():
                i[0] = (i[0] + 1) % copies8
                return ops.skinny_linear_fp8(x, w8[i[0]][0], w8[i[0]][1], None, act="swiglu" if act else None)

            def mx4():
                i[0] = (i[0] + 1) % copies4
                return ops.skinny_linear_mxfp4(x, w4[i[0]][0], w4[i[0]][1], None, act="swiglu" if act else None)

            def a8():
                i[0] = (i[0] + 1) % copies4
                return ops.skinny_linear_mxfp4_a8(x, w4[i[0]][0], w4[i[0]][1], None, act="swiglu" if act else None)

            xq, xs = ops.quantize_mxfp8_rows(x)

            def a8_gemm():
                i[0] = (i[0] + 1) % copies4
                return torch.ops.dtg.skinny_linear_mxfp4_a8(xq, xs, w4[i[0]][0], w4[i[0]][1], None, int(act))

            def blas():
                i[0] = (i[0] + 1) % copies
                y = torch.mm(x, ws[i[0]].t())
                return ops.swiglu(y) if act else y

            res, spread = {}, {}
            arms = (("mfma", mfma), ("mx4", mx4), ("a8", a8), ("a8g", a8_gemm), ("blas", blas)) + ((("kernel", kernel), ("fp8", fp8)) if M <= FMAF_MAX_M else ())
            for which, fn in arms * 2:
                t = time_ms(torch, fn, a.min_ms)
                spread[which] = round(100 * abs(res.get(which, t) - t) / min(res.get(which, t), t), 1)
                res[which] = min(res.get(which, t), t)
            r = {"proj": name, "N": N, "K": K, "M": M, "copies": copies, "mfma_us": round(res["mfma"] * 1e3, 1),
                 "mfma_GBps": round(wbytes / res["mfma"] / 1e6, 1), "blas_over_mfma": round(res["blas"] / res["mfma"], 2),
                 "blas_us": round(res["blas"] * 1e3, 1), "blas_GBps": round(wbytes / res["blas"] / 1e6, 1),
                 "mx4_copies": copies4, "mx4_us": round(res["mx4"] * 1e3, 1), "mx4_spread_pct": spread["mx4"],
                 "mx4_GBps": round(mxbytes / res["mx4"] / 1e6, 1), "mfma_over_mx4": round(res["mfma"] / res["mx4"], 2),
                 "a8_us": round(res["a8"] * 1e3, 1), "a8_spread_pct": spread["a8"], "a8_gemm_us": round(res["a8g"] * 1e3, 1),
                 "a8_gemm_spread_pct": spread["a8g"], "a8_gemm_GBps": round(mxbytes / res["a8g"] / 1e6, 1),
                 "mx4_over_a8": round(res["mx4"] / res["a8"], 2), "mx4_over_a8_gemm": round(res["mx4"] / res["a8g"], 2),
                 "mfma_over_a8": round(res["mfma"] / res["a8"], 2)}
            if M <= FMAF_MAX_M:
                r.update({"kernel_us": round(res["kernel"] * 1e3, 1), "kernel_GBps": round(wbytes / res["kernel"] / 1e6, 1),
                          "blas_over_kernel": round(res["blas"] / res["kernel"], 2),
                          "kernel_over_mfma": round(res["kernel"] / res["mfma"], 2),
                          "fp8_copies": copies8, "fp8_us": round(res["fp8"] * 1e3, 1),
                          "fp8_GBps": round(N * K / res["fp8"] / 1e6, 1),
                          "kernel_over_fp8": round(res["kernel"] / res["fp8"], 2), "fp8_spread_pct": spread["fp8"],
                          "fp8_over_mx4": round(res["fp8"] / res["mx4"], 2)})
            print(json.dumps(r), flush=True)
            out.append(r)
        del ws, w8, w4
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fp:
            cols = ["a8_us", "a8_gemm_us", "a8_spread_pct", "a8_gemm_spread_pct", "a8_gemm_GBps", "mx4_over_a8",
                    "mx4_over_a8_gemm", "mfma_over_a8", "mx4_us", "mfma_us", "kernel_us", "fp8_us", "blas_us", "mx4_GBps", "mfma_GBps", "kernel_GBps", "fp8_GBps",
                    "blas_GBps", "mx4_spread_pct", "fp8_spread_pct", "fp8_over_mx4", "mfma_over_mx4", "blas_over_mfma",
                    "kernel_over_mfma", "blas_over_kernel", "kernel_over_fp8"]
            fp.write("| projection | N x K | M | W4A8 quantiser + GEMM µs | W4A8 GEMM µs | W4A8 spread % | W4A8 GEMM spread % | "
                     "W4A8 GEMM GB/s (mxfp4 bytes) | mxfp4 / W4A8 | mxfp4 / W4A8 GEMM | mfma / W4A8 | mxfp4 kernel µs | mfma kernel µs | fmaf kernel µs | fp8 kernel µs | hipBLASLt µs | "
                     "mxfp4 GB/s (mxfp4 bytes) | mfma GB/s (weights) | fmaf GB/s (weights) | fp8 GB/s (fp8 bytes) | "
                     "hipBLASLt GB/s | mxfp4 spread % | fp8 spread % | fp8 / mxfp4 | mfma / mxfp4 | hipBLASLt / mfma | "
                     "fmaf / mfma | hipBLASLt / fmaf | fmaf / fp8 |\n")
            fp.write("|---" * (3 + len(cols)) + "|\n")
            for r in out:
                fp.write(f"| {r['proj']} | {r['N']} x {r['K']} | {r['M']} | " + " | ".join(str(r.get(c, "-")) for c in cols)
                         + " |\n")


if __name__ == "__main__":
    main()
