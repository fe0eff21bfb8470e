"""Global-norm gradient clipping through the engines on CPU ranks (gloo): every engine and
layout reports the one-process norm, counts TP-replicated weights once, and agrees with
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.

Tolerances are the ones the existing equivalence tests use:
  * parameters after a step: atol=3e-4, rtol=1e-3 (tests/test_engines_cpu.py, test_fsdp_cpu.py and
    test_tp_cpu.py `TOL`);
  * the gradient norm: rtol=1e-4, the relative tolerance test_tp_cpu.py puts on gradients
    (test_vocab_parallel_ce_pipelined_chunks_match_single: atol=1e-5, rtol=1e-4);
  * against torch's AdamW: atol=1e-6, rtol=1e-5 (tests/test_ops_cpu.py
    test_adamw_cpu_matches_torch_adamw).
"""
import math

import pytest
import torch

import dtg  # noqa: F401

from _dist import run_distributed

TOL = dict(atol=3e-4, rtol=1e-3)
NORM_RTOL = 1e-4
TORCH_TOL = dict(atol=1e-6, rtol=1e-5)
SIZES = [0, 1, 7, 8, 9, 1001, 2048, 2049, 256 * 8 * 3 + 5, 2 ** 20 + 3]


def _batch(vocab, B=4, S=32, seed=0):
    return torch.randint(0, vocab, (B, S), generator=torch.Generator().manual_seed(seed))


def _is_norm(name):
    return "norm" in name


def _full_model(model_name, norm_scale):
    """The unsharded f32 model every layout starts from.  norm_scale < 1 shrinks the RMSNorm
    weights: the gradients of everything downstream of a norm shrink with them while the norm
    weights' own gradients do not, which gives those (TP-replicated) weights a large share of
    the squared gradient norm."""
    from dtg.models import build_model, resolve_config

    cfg = resolve_config(model_name)
    torch.manual_seed(0)
    full = build_model(cfg, device="cpu", dtype=torch.float32)
    if norm_scale != 1.0:
        with torch.no_grad():
            for n, p in full.named_parameters():
                if _is_norm(n):
                    p.mul_(norm_scale)
    return cfg, full


def _step(rank, world, kind, tp, model_name, ids, max_norm, accum=1, norm_scale=1.0):
    """One optimizer step of `kind` (single | ddp | zero | fsdp) on dp = world / tp data-parallel
    ranks x tp tensor-parallel ranks.  Returns the full (or this TP rank's) parameters, the
    norm, the clip coefficient of every rank, the TP rank and the norm weights' share."""
    import torch.distributed as dist

    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    cfg, model = _full_model(model_name, norm_scale)
    dp_group = tp_group = None
    dp, dp_rank, tp_rank = world, rank, 0
    if tp > 1:
        from dtg.parallel.tensor_parallel import make_mesh, shard_full_state_dict

        dp_group, tp_group, dp_rank, tp_rank, dp = make_mesh(tp)
        sharded = build_model(cfg, device="cpu", dtype=torch.float32, tp_group=tp_group, init=False)
        sharded.load_state_dict(shard_full_state_dict(model.state_dict(), cfg, tp_rank, tp))
        model = sharded
    if kind == "fsdp":
        from dtg.parallel.fsdp import FullyShard

        eng = FullyShard(model, group=dp_group, tp_group=tp_group, device="cpu", max_grad_norm=max_norm)
    else:
        eng = DataParallel(model, mode=kind if dp > 1 else "single", group=dp_group, tp_group=tp_group,
                           bucket_mb=1, broadcast_from_rank0=tp_group is None, max_grad_norm=max_norm)
    opt = FlatAdamW(eng, lr=1e-2, eps=1e-3)
    per = ids.shape[0] // dp
    mine = ids[dp_rank * per:(dp_rank + 1) * per]
    opt.zero_grad()
    micro = mine.chunk(accum)
    for i, mb in enumerate(micro):
        if i < accum - 1:
            with eng.no_sync():
                eng.backward(model(input_ids=mb, labels=mb).loss)
        else:
            eng.backward(model(input_ids=mb, labels=mb).loss)
    share = None
    if kind == "single" and tp == 1:  # main_grad holds the whole summed gradient
        tot = sum(p.main_grad.double().pow(2).sum().item() for p in model.parameters())
        nrm = sum(p.main_grad.double().pow(2).sum().item() for n, p in model.named_parameters() if _is_norm(n))
        share = (nrm / tot, math.sqrt(tot) / accum)
    opt.step()
    coef = eng.last_clip_coef.reshape(1).clone()
    coefs = [coef]
    if world > 1:
        coefs = [torch.zeros(1) for _ in range(world)]
        dist.all_gather(coefs, coef)
    if kind == "fsdp":
        sd = eng.full_state_dict(rank0_only=False)
    else:
        if hasattr(eng, "wait_param_gather"):
            eng.wait_param_gather()
        sd = {n: p.detach().clone() for n, p in model.named_parameters()}
    return dict(params=sd, norm=float(eng.last_grad_norm), coefs=coefs, tp_rank=tp_rank, share=share)


_REF = {}


def _reference(model_name, max_norm, norm_scale=1.0):
    """The one-process step on the whole batch; computed once per configuration and shared."""
    from dtg.models import resolve_config

    key = (model_name, max_norm, norm_scale)
    if key not in _REF:
        ids = _batch(resolve_config(model_name).vocab_size)
        _REF[key] = (ids, _step(0, 1, "single", 1, model_name, ids, max_norm, norm_scale=norm_scale))
    return _REF[key]


def _check_against(ref, res, tp, cfg):
    for r in res:
        assert r["norm"] == pytest.approx(ref["norm"], rel=NORM_RTOL), (r["norm"], ref["norm"])
        for c in r["coefs"]:  # every rank applied bit-identical coefficients
            assert torch.equal(c, res[0]["coefs"][0]), r["coefs"]
    if tp > 1:
        from dtg.parallel.tensor_parallel import unshard_state_dicts

        shards = [r["params"] for r in sorted(res[:tp], key=lambda r: r["tp_rank"])]
        full = unshard_state_dicts(shards, cfg)
    else:
        full = res[-1]["params"]
    for n, v in ref["params"].items():
        torch.testing.assert_close(full[n], v, **TOL, msg=n)


# ---------------------------------------------------------------------------------------- B1
@pytest.mark.parametrize("kind", ["ddp", "zero", "fsdp"])
def test_engines_agree_with_one_process(kind):
    from dtg.models import resolve_config

    ids, ref = _reference("llama-tiny", 1.0)
    assert ref["share"][1] > 2.0 and ref["coefs"][0].item() < 0.5  # the clip is active
    assert ref["norm"] == pytest.approx(ref["share"][1], rel=NORM_RTOL)
    res = run_distributed(_step, 2, kind, 1, "llama-tiny", ids, 1.0)
    _check_against(ref, res, 1, resolve_config("llama-tiny"))


# ---------------------------------------------------------------------------------------- B2
@pytest.mark.parametrize("world,kind", [(2, "ddp"), (4, "zero"), (4, "fsdp")])
def test_tp_counts_replicated_weights_once(world, kind):
    """tp 2 (x dp 2): the norm weights are replicated over TP and must enter the norm once.  They
    carry well over 10 % of the squared norm here (asserted), so counting them once per TP rank
    would move the norm by more than 4 %, far outside the tolerance."""
    from dtg.models import resolve_config

    name, scale, clip = "llama-tiny-d128", 0.02, 0.02
    ids, ref = _reference(name, clip, scale)
    assert ref["share"][0] >= 0.10, ref["share"]
    assert ref["coefs"][0].item() < 1.0  # the clip is active
    res = run_distributed(_step, world, kind, 2, name, ids, clip, 1, scale)
    _check_against(ref, res, 2, resolve_config(name))


# ---------------------------------------------------------------------------------------- B3
def test_clip_semantics_match_torch():
    """clip_grad_norm_ + torch.optim.AdamW on a copy of the model with the engine's gradients."""
    from dtg.models import build_model, resolve_config
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    cfg = resolve_config("llama-tiny")
    torch.manual_seed(0)
    model = build_model(cfg, device="cpu", dtype=torch.float32)
    twin = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.named_parameters()}
    eng = DataParallel(model, mode="single", max_grad_norm=1.0)
    opt = FlatAdamW(eng, lr=1e-2, eps=1e-3, weight_decay=0.01)
    ids = _batch(cfg.vocab_size)
    opt.zero_grad()
    eng.backward(model(input_ids=ids, labels=ids).loss)
    for n, p in model.named_parameters():
        twin[n].grad = p.main_grad.detach().clone()
    opt.step()
    total = torch.nn.utils.clip_grad_norm_(list(twin.values()), 1.0)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-2, eps=1e-3, weight_decay=0.01)
    ref_opt.step()
    assert float(total) > 1.0  # the clip is active
    assert float(eng.last_grad_norm) == pytest.approx(float(total), rel=NORM_RTOL)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.detach(), twin[n].detach(), **TORCH_TOL, msg=n)


# ---------------------------------------------------------------------------------------- B4
@pytest.mark.parametrize("kind", ["single", "fsdp"])
def test_accumulated_norm_is_of_the_averaged_gradient(kind):
    from dtg.models import resolve_config

    ids, ref = _reference("llama-tiny", 1.0)
    one = _step(0, 1, kind, 1, "llama-tiny", ids, 1.0, accum=1)
    two = _step(0, 1, kind, 1, "llama-tiny", ids, 1.0, accum=2)
    for r in (one, two):
        _check_against(ref, [r], 1, resolve_config("llama-tiny"))


def test_measure_only_leaves_the_step_unchanged():
    from dtg.models import resolve_config

    ids = _batch(resolve_config("llama-tiny").vocab_size)
    for kind in ("single", "fsdp"):
        off = _step_plain(kind, ids)
        on = _step(0, 1, kind, 1, "llama-tiny", ids, float("inf"))
        assert on["coefs"][0].item() == 1.0 and on["norm"] > 0
        for n, v in off.items():
            assert torch.equal(on["params"][n], v), n


def _step_plain(kind, ids):
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    _, model = _full_model("llama-tiny", 1.0)
    if kind == "fsdp":
        from dtg.parallel.fsdp import FullyShard

        eng = FullyShard(model, device="cpu")
    else:
        eng = DataParallel(model, mode="single", bucket_mb=1)
    opt = FlatAdamW(eng, lr=1e-2, eps=1e-3)
    opt.zero_grad()
    eng.backward(model(input_ids=ids, labels=ids).loss)
    opt.step()
    assert eng.last_grad_norm is None and eng.last_clip_coef is None
    if kind == "fsdp":
        return eng.full_state_dict(rank0_only=False)
    return {n: p.detach().clone() for n, p in model.named_parameters()}


# ---------------------------------------------------------------------------------------- B5
def test_rejections():
    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel
    from dtg.parallel.fsdp import FullyShard
    from dtg.train import trainer

    model = build_model("llama-tiny", device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="overlap_optimizer"):
        DataParallel(model, mode="single", overlap_optimizer=True, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="cpu_offload"):
        FullyShard(model, device="cpu", cpu_offload=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        DataParallel(model, mode="single", max_grad_norm=0.0)
    base = ["-e", "x", "-d", "synthetic", "-m", "llama-tiny"]
    with pytest.raises(SystemExit, match="--pp"):
        trainer.run("02", base + ["--pp", "2", "--max-grad-norm", "1.0"])
    with pytest.raises(SystemExit, match="--pp"):
        trainer.run("02", base + ["--pp", "2", "--log-grad-norm", "on"])
    with pytest.raises(SystemExit, match="--cpu-offload"):
        trainer.run("04", base + ["--cpu-offload", "on", "--max-grad-norm", "1.0"])
    with pytest.raises(SystemExit, match="--cpu-offload"):
        trainer.run("05", base + ["--max-grad-norm", "1.0"])  # chapter 05 offloads by default


def test_cli_flags_and_deepspeed_mapping(tmp_path):
    import json

    from dtg.train import trainer
    from dtg.train.cli import get_parser

    base = ["-e", "x", "-d", "synthetic", "-m", "llama-tiny"]
    for ch in ("rime", "01", "02", "04", "05", "06", "07", "deepspeed"):
        a = get_parser(ch).parse_args(base)
        assert a.max_grad_norm == 0.0 and a.log_grad_norm == "off"
        assert trainer._max_grad_norm(a, "01") is None
    a = get_parser("01").parse_args(base + ["--max-grad-norm", "0.5"])
    assert trainer._max_grad_norm(a, "01") == 0.5
    a = get_parser("01").parse_args(base + ["--log-grad-norm", "on"])
    assert trainer._max_grad_norm(a, "01") == float("inf")
    cfg = tmp_path / "ds.json"
    cfg.write_text(json.dumps({"gradient_clipping": 0.7, "zero_optimization": {"stage": 2}}))
    a = trainer._deepspeed_overrides(get_parser("deepspeed").parse_args(base + ["--deepspeed_config", str(cfg)]))
    assert a.max_grad_norm == 0.7
    cfg.write_text(json.dumps({"zero_optimization": {"stage": 2}}))
    a = trainer._deepspeed_overrides(get_parser("deepspeed").parse_args(base + ["--deepspeed_config", str(cfg)]))
    assert a.max_grad_norm == 0.0


# ---------------------------------------------------------------------------------------- B6
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_sumsq_cpu_op_is_exact_on_integers(dtype):
    """Gradients from {-2, ..., 2}: every partial sum is an integer <= 4 n < 2^24, so any f32
    summation order is exact."""
    from dtg.ops.grad_norm import grad_sumsq_

    gen = torch.Generator().manual_seed(0)
    for n in SIZES:
        buf = torch.randint(-2, 3, (n + 1,), generator=gen).to(dtype)
        for g in (buf[:n], buf[1:]):
            keep = g.clone()
            acc = torch.tensor([5.0, 7.0])
            grad_sumsq_(g, acc, 0)
            assert torch.equal(acc, torch.tensor([5.0 + float(g.double().pow(2).sum()), 7.0])), n
            assert torch.equal(g, keep)  # the input is only read


def test_clip_coef_semantics():
    from dtg.ops.grad_norm import clip_coef_

    def coef(sumsq, max_norm, pre=1.0):
        return clip_coef_(torch.zeros(2), torch.tensor(sumsq), max_norm, pre)

    s = coef(16.0, 1.0, 0.5)  # norm of the averaged gradient = 4 * 0.5
    assert s[0].item() == 2.0 and s[1].item() == pytest.approx(1.0 / (2.0 + 1e-6))
    assert coef(0.25, 1.0)[1].item() == 1.0  # below the bound: untouched
    assert coef(float("inf"), 1.0)[1].item() == 0.0 and math.isnan(coef(float("nan"), 1.0)[1].item())
    for x in (4.0, float("inf"), float("nan")):  # measure only: exactly 1
        assert coef(x, float("inf"))[1].item() == 1.0
