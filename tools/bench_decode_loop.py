#!/usr/bin/env python3
"""The decode loop of dtg.generate in its six forms -- projections in hipBLASLt, in the skinny-GEMM kernel
or in the weight-only FP8 skinny-GEMM kernel, the loop eager or captured into HIP graphs -- on random-init
Qwen3-0.6B and Llama-3.2-1B, batch 1 and 8, a 16-token prompt and 256 new tokens, greedy.  The FP8 copies are
quantised once per model, outside every clock; a step reads every matrix once, and both models' matrices
(0.6-2.5 GB in either format) exceed the 256 MB Infinity Cache, so no arm re-reads its weights from a cache.

The arms alternate over `--rounds` rounds.  Tokens / s cover the decode steps after the first bucket's
warm-up and capture.  Eager arms: the clock starts (device synchronised) once the loop has run WARM steps
and stops after the last.  Graph arms: a first short run on a GraphedDecode warms up and captures the
first bucket, then a whole second run on the same object is timed and a separately measured prefill is
subtracted; the capture of the last bucket (lengths 257-272, 16 steps) falls inside that run, so the
graph arms are understated by it.  The capture time of both buckets is reported on its own.  blas +
eager is the loop without either option and is the baseline.  For every arm the spread (max - min over the rounds, relative to the median) is printed next to the median: call an arm
faster only when the gap exceeds both spreads.  Needs a GPU.

    python tools/bench_decode_loop.py [--md OUT.md]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MODELS = ("qwen3-0.6b", "llama-3.2-1b")
BATCHES = (1, 8)
PROMPT, NEW, WARM = 16, 256, 8
ARMS = [("blas", "eager"), ("skinny", "eager"), ("skinny-fp8", "eager"), ("blas", "graph"), ("skinny", "graph"),
        ("skinny-fp8", "graph")]


def run_arm(torch, model, prompts, linear, decode, s_max, fp8=None):
    """One generate()-equivalent run; returns (tokens / s of the timed steps, capture seconds, first row's ids)."""
    from dtg.models.decode_graph import GraphedDecode
    from dtg.models.generation import KVCache, decode_bucket, decode_step, prefill

    n = len(prompts)
    fp8 = fp8 if linear == "skinny-fp8" else None  # quantised once per model, outside every clock
    if decode == "graph":
        # the loop of GraphedDecode.run with a clock in it: two runs on one object, the first captures
        gd = GraphedDecode(model, n, s_max, linear=linear, fp8=fp8)
        gd.run(prompts, WARM + 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gd.run(prompts, NEW)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # the second run replays from its first step; its prefill is measured on its own and subtracted
        t1 = time.perf_counter()
        gd.reset()
        prefill(model, prompts, gd.cache, fp8=fp8)
        torch.cuda.synchronize()
        pre = time.perf_counter() - t1
        return n * (NEW - 1) / max(dt - pre, 1e-9), gd.capture_seconds, out[0]
    dev = model.embed_tokens.weight.device
    cache = KVCache(model.config, n, s_max, device=dev, dtype=model.embed_tokens.weight.dtype)
    nxt = prefill(model, prompts, cache, fp8=fp8).argmax(-1)
    ids = [nxt]
    for step in range(1, NEW):
        if step == WARM:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        nxt = decode_step(model, nxt, cache, linear=linear, plan_len=decode_bucket(cache.max_len + 1, s_max),
                          fp8=fp8).argmax(-1)
        ids.append(nxt)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return n * (NEW - WARM) / dt, 0.0, torch.stack(ids, 1)[0].cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_loop: needs a GPU")
    import dtg  # noqa: F401
    from dtg.models import Fp8DecodeWeights, build_model, resolve_config

    dev = torch.device("cuda:0")
    rows = []
    for name in a.models.split(","):
        cfg = resolve_config(name)
        torch.manual_seed(0)
        model = build_model(cfg, device=dev).eval()
        fp8 = Fp8DecodeWeights(model)
        for n in BATCHES:
            g = torch.Generator().manual_seed(n)
            prompts = [torch.randint(0, cfg.vocab_size, (PROMPT,), generator=g) for _ in range(n)]
            s_max = PROMPT + NEW
            res = {arm: [] for arm in ARMS}
            cap = {arm: 0.0 for arm in ARMS}
            ids = {}
            with torch.no_grad():
                for _ in range(a.rounds):
                    for arm in ARMS:
                        tps, c, first = run_arm(torch, model, prompts, arm[0], arm[1], s_max, fp8)
                        res[arm].append(tps)
                        cap[arm] = max(cap[arm], c)
                        ids[arm] = first
            base = sorted(res[("blas", "eager")])[len(res[("blas", "eager")]) // 2]
            for arm in ARMS:
                v = sorted(res[arm])
                med = v[len(v) // 2]
                r = {"model": name, "batch": n, "linear": arm[0], "decode": arm[1], "tokens_per_s": round(med, 1),
                     "ms_per_step": round(1e3 * n / med, 3), "spread_pct": round(100 * (v[-1] - v[0]) / med, 1),
                     "vs_baseline": round(med / base, 2), "capture_s": round(cap[arm], 3),
                     "ids_equal_skinny_eager": bool(torch.equal(ids[arm], ids[("skinny", "eager")]))}
                print(json.dumps(r), flush=True)
                rows.append(r)
        del model, fp8
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fp:
            fp.write("| model | batch | linear | decode | tokens/s | ms / step | spread % | vs blas+eager | capture s |\n")
            fp.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fp.write(f"| {r['model']} | {r['batch']} | {r['linear']} | {r['decode']} | {r['tokens_per_s']} | "
                         f"{r['ms_per_step']} | {r['spread_pct']} | {r['vs_baseline']} | {r['capture_s']} |\n")


if __name__ == "__main__":
    main()
