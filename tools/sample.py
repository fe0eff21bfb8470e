#!/usr/bin/env python3
"""Generate from a model of this framework with the KV-cache path (dtg.models.generation).

    python tools/sample.py --model-name qwen3-0.6b --num-layers 2 --prompt-ids "1,2,3;4,5"
    python tools/sample.py --model-name llama-3.2-3b --init-from /data/llama-3.2-3b --tokenizer /data/llama-3.2-3b \
        --prompt "The capital of France is" --max-new-tokens 32 --temperature 0.7 --top-p 0.9
    python tools/sample.py --model-name qwen3-0.6b --prompt-ids "1,2,3;4,5" --temperature 0.8 --top-k 50 --min-p 0.05 \
        --sampler fused
    python tools/sample.py --model-name qwen3-0.6b --prompt-ids "1,2,3;4,5" --max-new-tokens 256 --linear skinny \
        --decode graph

Weights: `--init-from DIR` (HF safetensors) or `--ckpt DIR` (a sharded checkpoint directory written by
this trainer); random init otherwise.  Prompts: `--prompt-ids` (sequences separated by ';', ids by
','), or `--tokenizer DIR --prompt TEXT` with a tokenizer loaded from a LOCAL directory only -- nothing
is ever fetched.  Prints the new ids of every sequence (and their text with a tokenizer), then one
JSON line with the token count and tokens / s (wall time of the whole generate call, device synchronised).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def parse_prompt_ids(text):
    seqs = [[int(t) for t in s.split(",") if t.strip()] for s in text.split(";") if s.strip()]
    if not seqs or any(not s for s in seqs):
        raise SystemExit(f"--prompt-ids: no ids in {text!r}")
    return seqs


def load_tokenizer(path):
    if not os.path.isdir(path):
        raise SystemExit(f"--tokenizer: {path!r} is not a local directory (tokenizers are never downloaded)")
    os.environ.setdefault("HF_HUB_OFFLINE", "1")
    os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")
    try:
        from transformers import AutoTokenizer
    except ImportError as e:
        raise SystemExit(f"--tokenizer needs the `transformers` package: {e}")
    return AutoTokenizer.from_pretrained(path, local_files_only=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-name", required=True)
    ap.add_argument("--num-layers", type=int, default=None, help="truncate the config to this many layers")
    ap.add_argument("--init-from", default=None, help="HF safetensors directory")
    ap.add_argument("--ckpt", default=None, help="sharded checkpoint directory of this trainer")
    ap.add_argument("--prompt-ids", default=None, help='e.g. "1,2,3;4,5": two prompts')
    ap.add_argument("--tokenizer", default=None, help="local tokenizer directory")
    ap.add_argument("--prompt", action="append", default=None, help="text prompt (repeatable; needs --tokenizer)")
    ap.add_argument("--max-new-tokens", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--min-p", type=float, default=0.0, help="keep ids at least this likely relative to the favourite "
                    "(needs --sampler fused)")
    ap.add_argument("--sampler", choices=("torch", "fused"), default="torch",
                    help="torch: the chain of torch ops, one generator for the batch; fused: one HIP launch per step "
                    "with a counter-based draw per sequence (different ids for the same seed)")
    ap.add_argument("--linear", choices=("blas", "skinny", "skinny-fp8"), default="blas",
                    help="decode-step projections: hipBLASLt, the skinny-GEMM HIP kernel, or that kernel on weight-only "
                    "FP8 (e4m3, per-row scales) copies of the matrices, quantised at start (at most 16 prompts)")
    ap.add_argument("--kv-cache", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: an e4m3 KV cache with one power-of-two scale per key vector, about half the bytes")
    ap.add_argument("--decode", choices=("eager", "graph"), default="eager",
                    help="graph: capture the decode step into one HIP graph per length bucket and replay it (GPU; "
                    "sampling then needs --sampler fused)")
    ap.add_argument("--speculate", choices=("ngram",), default=None,
                    help="speculative decoding with exact-match verification: the prompt-lookup drafter (eager decode; "
                    "sampling needs --sampler fused); prints the acceptance stats")
    ap.add_argument("--draft-tokens", type=int, default=4, metavar="K",
                    help="tokens per verify pass and prompt: the last accepted id plus K - 1 drafted ids")
    ap.add_argument("--eos-token-id", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default=None, help="default: cuda if available, else cpu")
    ap.add_argument("--override", action="append", default=[], metavar="KEY=INT", help="config override, e.g. vocab_size=512")
    a = ap.parse_args(argv)
    if a.init_from and a.ckpt:
        raise SystemExit("pass --init-from or --ckpt, not both")
    if (a.prompt_ids is None) == (a.prompt is None):
        raise SystemExit("pass --prompt-ids, or --tokenizer DIR --prompt TEXT")
    if a.prompt is not None and a.tokenizer is None:
        raise SystemExit("--prompt needs --tokenizer DIR")

    import torch

    import dtg  # noqa: F401
    from dtg.models import build_model, resolve_config

    dev = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    over = {k: int(v) for k, v in (o.split("=", 1) for o in a.override)}
    if a.num_layers is not None:
        over["num_hidden_layers"] = a.num_layers
    cfg = resolve_config(a.model_name, **over)
    torch.manual_seed(a.seed)
    model = build_model(cfg, device=dev)
    if a.init_from or a.ckpt:
        from dtg.parallel.data_parallel import DataParallel

        eng = DataParallel(model, mode="single")
        if a.init_from:
            from dtg.models.loading import load_pretrained

            load_pretrained(eng, a.init_from, cfg)
        else:
            from dtg.train.checkpoint import load_sharded

            load_sharded(a.ckpt, eng, load_optimizer=False)
    tok = load_tokenizer(a.tokenizer) if a.tokenizer else None
    if a.prompt is not None:
        seqs = [tok(p)["input_ids"] for p in a.prompt]
    else:
        seqs = parse_prompt_ids(a.prompt_ids)
    bad = [i for s in seqs for i in s if not 0 <= i < cfg.vocab_size]
    if bad:
        raise SystemExit(f"prompt ids {bad[:5]} outside the vocabulary [0, {cfg.vocab_size})")
    eos = a.eos_token_id if a.eos_token_id is not None else (getattr(tok, "eos_token_id", None) if tok else None)
    prompts = [torch.tensor(s, dtype=torch.long) for s in seqs]

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    spec = None
    if a.speculate is not None:
        try:
            spec = dtg.Speculative(a.speculate, k=a.draft_tokens)
        except ValueError as e:
            raise SystemExit(f"--draft-tokens: {e}")
    sync()
    t0 = time.perf_counter()
    out = dtg.generate(model, prompts, a.max_new_tokens, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                       eos_token_id=eos, seed=a.seed, min_p=a.min_p, sampler=a.sampler, linear=a.linear, decode=a.decode,
                       speculate=spec, kv_cache=a.kv_cache)
    sync()
    dt = time.perf_counter() - t0
    if spec is not None:
        print(json.dumps({"speculate": a.speculate, "draft_tokens": spec.k, **spec.stats}))
    for i, ids in enumerate(out):
        print(f"ids[{i}]: {','.join(str(int(t)) for t in ids)}")
        if tok is not None:
            print(f"text[{i}]: {tok.decode(ids.tolist())}")
    n = sum(int(o.numel()) for o in out)
    print(json.dumps({"sequences": len(out), "new_tokens": n, "seconds": round(dt, 4),
                      "tokens_per_s": round(n / dt, 2) if dt > 0 else None, "device": str(dev), "sampler": a.sampler,
                      "linear": a.linear, "decode": a.decode}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
