#!/usr/bin/env python3
"""The split-KV decode attention kernel (csrc/kernels/decode_attn.hip) against the composed torch path
(DTG_DECODE_FUSED=0) in the same process: time per call from HIP events and the rate at which the K
and V bytes the call must read are consumed, at the Llama-3-8B head shape (nq 32, nkv 8, D 128), batch
1 / 8 / 64 and cache lengths 1k / 8k / 32k.

Bytes counted: 2 (K, V) x B x nkv x len x D bf16 values -- every sequence is `len` long, so this is what
any implementation has to read; q, the output and the split partials are below 1 % of it.  Every shape
is warmed up, the two paths alternate, and each timing covers at least `--min-ms` of device time.
Needs a GPU: there is no CPU fallback for a timing.

--kv-cache fp8 adds the kernel's e4m3 cache format as a third arm, alternated with the bf16 kernel in the same
process: the same keys quantised per key vector (ops.quantize_fp8_rows), so its bytes are
2 x B x nkv x len x (D + 4): the codes and one f32 scale per key vector.  --no-composed drops the torch arm.

    python tools/bench_decode.py [--md OUT.md] [--kv-cache fp8] [--no-composed]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NQ, NKV, D = 32, 8, 128
BATCHES = (1, 8, 64)
LENGTHS = (1024, 8192, 32768)


def time_ms(torch, fn, min_ms, rounds=3):
    """Median over `rounds` of the mean device time per call, each round >= min_ms of work."""
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
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--md", default=None, help="also write the table as markdown here")
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes instead of 1,8,64")
    ap.add_argument("--lengths", default=None, help="comma-separated cache lengths instead of 1024,8192,32768")
    ap.add_argument("--true-len", type=int, default=None, help="every sequence is this long while the launch plan is "
                    "made for the cache length (max_len): what planning for a whole length bucket costs")
    ap.add_argument("--kv-cache", choices=("bf16", "fp8"), default="bf16", help="fp8: also time the kernel on an e4m3 cache")
    ap.add_argument("--no-composed", action="store_true", help="skip the composed torch arm")
    a = ap.parse_args()
    batches = BATCHES if a.batches is None else tuple(int(v) for v in a.batches.split(","))
    lengths = LENGTHS if a.lengths is None else tuple(int(v) for v in a.lengths.split(","))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode: needs a GPU (a CPU timing says nothing about the kernel)")
    import dtg  # noqa: F401
    from dtg import ops
    from dtg.ops import functional

    dev = torch.device("cuda:0")
    rows_out = []
    for B in batches:
        for L in lengths:
            g = torch.Generator(device=dev).manual_seed(B * 100003 + L)
            qkv = torch.randn(B, (NQ + 2 * NKV) * D, device=dev, generator=g).to(torch.bfloat16)
            kc = torch.randn(B, NKV, L, D, device=dev, generator=g).to(torch.bfloat16)
            vc = torch.randn(B, NKV, L, D, device=dev, generator=g).to(torch.bfloat16)
            rows = torch.arange(B, dtype=torch.int32, device=dev)
            n_keys = L if a.true_len is None else min(a.true_len, L)
            lens = torch.full((B,), n_keys, dtype=torch.int32, device=dev)

            def call():
                return ops.decode_attention(qkv, kc, vc, rows, lens, NQ, NKV, D, L)

            arms = [True] if a.no_composed else [True, False]
            if a.kv_cache == "fp8":
                q8 = []
                for c in (kc, vc):  # one sequence at a time: the quantiser works in f32
                    codes = torch.empty(c.shape, dtype=torch.float8_e4m3fn, device=dev)
                    scale = torch.empty(c.shape[:3], dtype=torch.float32, device=dev)
                    for b in range(B):
                        cq, sq = ops.quantize_fp8_rows(c[b].reshape(-1, D))
                        codes[b], scale[b] = cq.reshape(NKV, L, D), sq.reshape(NKV, L)
                    q8 += [codes, scale]
                kq, ks, vq, vs = q8

                def call_fp8():
                    return ops.decode_attention(qkv, kq, vq, rows, lens, NQ, NKV, D, L, k_scale=ks, v_scale=vs)

                arms.append("fp8")
            res, outs = {}, {}
            for arm in arms * 2:  # alternate; keep the better median of each path
                functional._DECODE_FUSED = arm is not False
                fn = call_fp8 if arm == "fp8" else call
                outs[arm] = fn()
                t = time_ms(torch, fn, a.min_ms)
                res[arm] = min(res.get(arm, t), t)
            functional._DECODE_FUSED = True
            nbytes = 2 * B * NKV * n_keys * D * 2
            r = {"batch": B, "len": L, "keys": n_keys, "kernel_us": round(res[True] * 1e3, 1),
                 "kernel_GBps": round(nbytes / res[True] / 1e6, 1)}
            if False in res:
                diff = (outs[True].float() - outs[False].float()).abs().max().item()
                r.update({"composed_us": round(res[False] * 1e3, 1), "composed_GBps": round(nbytes / res[False] / 1e6, 1),
                          "speedup": round(res[False] / res[True], 2), "max_abs_diff": round(diff, 5)})
            if "fp8" in res:
                nbytes8 = 2 * B * NKV * n_keys * (D + 4)
                r.update({"fp8_us": round(res["fp8"] * 1e3, 1), "fp8_GBps": round(nbytes8 / res["fp8"] / 1e6, 1),
                          "bf16_over_fp8": round(res[True] / res["fp8"], 2), "bf16_MB": round(nbytes / 2 ** 20, 1),
                          "fp8_MB": round(nbytes8 / 2 ** 20, 1),
                          "fp8_vs_bf16_max_abs_diff": round((outs["fp8"].float() - outs[True].float()).abs().max().item(), 5)})
                del kq, vq, ks, vs, q8
            print(json.dumps(r), flush=True)
            rows_out.append(r)
            del kc, vc
    if a.md:
        with open(a.md, "w") as fp:
            fp.write("| batch | cache len | kernel µs | composed µs | kernel GB/s (K+V) | composed GB/s | composed / kernel | max abs diff |\n")
            fp.write("|---|---|---|---|---|---|---|---|\n")
            for r in rows_out:
                fp.write(f"| {r['batch']} | {r['len']} | {r['kernel_us']} | {r.get('composed_us')} | {r['kernel_GBps']} | "
                         f"{r.get('composed_GBps')} | {r.get('speedup')} | {r.get('max_abs_diff')} |\n")
            if a.kv_cache == "fp8":
                fp.write("\n| batch | cache len | bf16 MB | fp8 MB | bf16 µs | fp8 µs | bf16 GB/s | fp8 GB/s (codes + scales) | bf16 / fp8 |\n")
                fp.write("|---|---|---|---|---|---|---|---|---|\n")
                for r in rows_out:
                    fp.write(f"| {r['batch']} | {r['len']} | {r['bf16_MB']} | {r['fp8_MB']} | {r['kernel_us']} | {r['fp8_us']} | "
                             f"{r['kernel_GBps']} | {r['fp8_GBps']} | {r['bf16_over_fp8']} |\n")


if __name__ == "__main__":
    main()
