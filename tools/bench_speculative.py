#!/usr/bin/env python3
"""Speculative decoding (generate(..., speculate=...)) against the plain eager loop, and the verify attention
kernel (ops.decode_attention_multi) against Q launches of ops.decode_attention, in one process.

Loop: tokens / s of `generate` at batch 1 and 4 on Qwen3-0.6B and a Llama-3.2-1B-shaped model (random init),
linear = blas / skinny / skinny-fp8, greedy, for the plain loop and for the speculative loop under three drafters:
  oracle  proposes the plain run's own ids: everything is accepted, the ceiling of the mode;
  wrong   proposes ids that are never right: one id per verify pass, the floor (the cost of a wasted verify);
  ngram   the built-in prompt-lookup drafter on a prompt that repeats itself (a random-init model does not
          repeat its prompt, so this mostly shows the drafter's host cost).
Every run is timed between HIP events around the whole call (device synchronised), after one warm-up call of
the same kind; the best of `--rounds` is kept.  The ids of every speculative run are compared with the plain
run's (linear = skinny / skinny-fp8: they must be equal).

Kernel: Llama-3-8B head shape (nq 32, nkv 8, D 128), time per call from HIP events as tools/bench_decode.py
takes it (warm-up, >= --min-ms per round, median of 3).  Needs a GPU.

    python tools/bench_speculative.py [--md OUT.md]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from bench_decode import time_ms  # noqa: E402

MODELS = {
    "qwen3-0.6b": ("qwen3-0.6b", {}),
    "llama-3.2-1b": ("llama-3.2-3b", dict(hidden_size=2048, num_hidden_layers=16, num_attention_heads=32,
                                         num_key_value_heads=8, intermediate_size=8192, head_dim=64)),
}


class Oracle:
    def __init__(self, ids, base, wrong, vocab):
        self.ids, self.base, self.wrong, self.vocab = ids, base, wrong, vocab

    def propose(self, history, want):
        out = []
        for row, h, w, b in zip(self.ids, history, want, self.base):
            d = row[len(h) - b: len(h) - b + w]
            out.append([(t + 1) % self.vocab for t in d] if self.wrong else d)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=100.0)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--md", default=None, help="also write the tables as markdown here")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_speculative: needs a GPU")
    import dtg  # noqa: F401
    from dtg import ops
    from dtg.models import Fp8DecodeWeights, Speculative, build_model, generate, resolve_config

    dev = torch.device("cuda:0")

    def timed(fn):
        fn()  # warm-up: allocations, hipBLASLt heuristics, the rope tables
        best, out = None, None
        for _ in range(a.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            out = fn()
            e.record()
            torch.cuda.synchronize()
            t = s.elapsed_time(e) * 1e-3
            best = t if best is None else min(best, t)
        return best, out

    loop_rows = []
    for name in a.models.split(","):
        base_name, over = MODELS[name]
        cfg = resolve_config(base_name, **over)
        torch.manual_seed(0)
        model = build_model(cfg, device=dev).eval()
        fp8_w = Fp8DecodeWeights(model)
        for batch in (1, 4):
            g = torch.Generator().manual_seed(batch)
            piece = torch.randint(0, cfg.vocab_size, (a.prompt_len // 4,), generator=g)
            prompts = {"random": [torch.randint(0, cfg.vocab_size, (a.prompt_len,), generator=g) for _ in range(batch)],
                       "repeat": [piece.roll(i).repeat(4) for i in range(batch)]}
            s_max = a.prompt_len + a.new
            for linear in ("blas", "skinny", "skinny-fp8"):
                kw = dict(s_max=s_max, linear=linear, fp8=fp8_w if linear == "skinny-fp8" else None)
                plain = {}
                for which, pr in prompts.items():
                    t, ids = timed(lambda pr=pr: generate(model, pr, a.new, **kw))
                    plain[which] = (t, ids)
                for mode in ("oracle", "wrong", "ngram"):
                    which = "repeat" if mode == "ngram" else "random"
                    t0, ref = plain[which]
                    pr = prompts[which]
                    if mode == "ngram":
                        spec = Speculative("ngram", k=a.k)
                    else:
                        spec = Speculative(Oracle([r.tolist() for r in ref], [len(p) for p in pr], mode == "wrong",
                                                  cfg.vocab_size), k=a.k)
                    t1, ids = timed(lambda pr=pr, spec=spec: generate(model, pr, a.new, speculate=spec, **kw))
                    st = spec.stats
                    r = {"model": name, "batch": batch, "linear": linear, "drafter": mode, "k": a.k,
                         "plain_tok_s": round(batch * a.new / t0, 1), "spec_tok_s": round(st["tokens"] / t1, 1),
                         "speedup": round(t0 / t1, 2), "steps": st["steps"], "proposed": st["proposed"],
                         "accepted": st["accepted"], "ids_equal": all(torch.equal(x, y) for x, y in zip(ids, ref))}
                    print(json.dumps(r), flush=True)
                    loop_rows.append(r)
        del model, fp8_w
        torch.cuda.empty_cache()

    NQ, NKV, D = 32, 8, 128
    kernel_rows = []
    for B in (1, 4):
        for L in (1024, 8192):
            for Q in (4, 8):
                g = torch.Generator(device=dev).manual_seed(B * 1000 + L + Q)
                qkv = torch.randn(B * Q, (NQ + 2 * NKV) * D, device=dev, generator=g).to(torch.bfloat16)
                kc = torch.randn(B, NKV, L, D, device=dev, generator=g).to(torch.bfloat16)
                vc = torch.randn(B, NKV, L, D, device=dev, generator=g).to(torch.bfloat16)
                rows = torch.arange(B, dtype=torch.int32, device=dev)
                lens = (L - Q + 1 + torch.arange(Q, device=dev)).repeat(B).to(torch.int32)
                per_tok = [(qkv[t::Q].contiguous(), lens[t::Q].contiguous()) for t in range(Q)]

                def multi():
                    return ops.decode_attention_multi(qkv, kc, vc, rows, lens, Q, NQ, NKV, D, L)

                def singles():
                    return [ops.decode_attention(x, kc, vc, rows, n, NQ, NKV, D, L) for x, n in per_tok]

                same = all(torch.equal(multi()[t::Q], o) for t, o in enumerate(singles()))
                tm = min(time_ms(torch, multi, a.min_ms), time_ms(torch, multi, a.min_ms))
                ts = min(time_ms(torch, singles, a.min_ms), time_ms(torch, singles, a.min_ms))
                r = {"batch": B, "len": L, "Q": Q, "multi_us": round(tm * 1e3, 1), "q_launches_us": round(ts * 1e3, 1),
                     "ratio": round(ts / tm, 2), "bitwise_equal": same}
                print(json.dumps(r), flush=True)
                kernel_rows.append(r)
    if a.md:
        with open(a.md, "w") as fp:
            fp.write("| model | batch | linear | drafter | plain tok/s | speculative tok/s | speculative / plain | passes | "
                     "proposed | accepted | ids equal |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in loop_rows:
                fp.write(f"| {r['model']} | {r['batch']} | {r['linear']} | {r['drafter']} | {r['plain_tok_s']} | "
                         f"{r['spec_tok_s']} | {r['speedup']} | {r['steps']} | {r['proposed']} | {r['accepted']} | "
                         f"{r['ids_equal']} |\n")
            fp.write("\n| batch | cache len | Q | decode_attn_multi µs | Q x decode_attn µs | Q launches / multi | bitwise equal |\n"
                     "|---|---|---|---|---|---|---|\n")
            for r in kernel_rows:
                fp.write(f"| {r['batch']} | {r['len']} | {r['Q']} | {r['multi_us']} | {r['q_launches_us']} | {r['ratio']} | "
                         f"{r['bitwise_equal']} |\n")


if __name__ == "__main__":
    main()
