#!/usr/bin/env python3
"""Time the sampling step: `sample_next` (the chain of torch ops behind sampler="torch") against
`ops.sample_logits` (the fused HIP kernel behind sampler="fused"), in one process on one GPU.

    python tools/bench_sampler.py [--warmup 10] [--iters 50] [--out FILE.jsonl]

bf16 logits at (n, V) = (1, 151936), (8, 151936), (64, 128256), with temperature 0.8 / top_k 50 /
top_p 0.95 and with no filter (temperature 1).  Every call is timed with a pair of HIP events after
`--warmup` untimed calls; the figure is the median of `--iters` calls, the two paths alternating call by
call.  The fused op takes its parameters as prebuilt device tensors, as a decode loop holds them; the
torch path takes Python scalars, its only form.  Prints one JSON line per point.  Needs a GPU: there is
no CPU fallback for a timing."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

POINTS = [(1, 151936), (8, 151936), (64, 128256)]
FILTERS = {"T0.8_k50_p0.95": (0.8, 50, 0.95), "no_filter": (1.0, 0, 1.0)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch

    import dtg  # noqa: F401
    from dtg import ops
    from dtg.models.generation import sample_next

    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler: needs a GPU")
    dev = torch.device("cuda:0")
    lines = []
    for n, V in POINTS:
        logits = (torch.randn(n, V, generator=torch.Generator().manual_seed(n)) * 4).bfloat16().to(dev)
        for label, (T, k, p) in FILTERS.items():
            gen = torch.Generator(device=dev)
            gen.manual_seed(0)
            col = lambda v, dt: torch.full((n,), v, dtype=dt, device=dev)  # noqa: E731
            kw = dict(temperature=col(T, torch.float32), top_k=col(k, torch.int32), top_p=col(p, torch.float32),
                      min_p=col(0.0, torch.float32), seed=col(0, torch.int64),
                      stream=torch.arange(n, dtype=torch.int64, device=dev), step=col(0, torch.int64))
            paths = {"torch": lambda: sample_next(logits, T, k, p, gen), "fused": lambda: ops.sample_logits(logits, **kw)}
            times = {name: [] for name in paths}
            for it in range(a.warmup + a.iters):
                for name, fn in paths.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if it >= a.warmup:
                        times[name].append(e0.elapsed_time(e1) * 1e3)
            med = {name: statistics.median(t) for name, t in times.items()}
            lines.append(json.dumps({"n": n, "V": V, "filter": label, "torch_us": round(med["torch"], 1),
                                     "fused_us": round(med["fused"], 1), "min_torch_us": round(min(times["torch"]), 1),
                                     "min_fused_us": round(min(times["fused"]), 1),
                                     "speedup": round(med["torch"] / med["fused"], 2), "iters": a.iters}))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
