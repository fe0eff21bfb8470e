"""Global gradient norm on the GPU: the grad_sumsq_ reduction (csrc/kernels/grad_norm.hip), the
device-side gradient scale of the AdamW kernels, the single-device engine, the HIP-graph step
and the chapter 01 command line."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import dtg.ops  # noqa: F401  (declares the torch.ops.dtg schemas, loads the native kernels)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 7, 8, 9, 1001, 2048, 2049, 256 * 8 * 3 + 5, 2 ** 20 + 3]
U = 2.0 ** -24  # unit roundoff of f32


def _sumsq(g, slots=2, slot=0, init=0.0):
    acc = torch.full((slots,), init, dtype=torch.float32, device=g.device)
    torch.ops.dtg.grad_sumsq_(g, acc, slot)
    return acc


# ---------------------------------------------------------------------------------------- A1
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sumsq_exact_coverage(cuda, dtype):
    """Gradients from {-2, ..., 2}: every partial sum is an integer <= 4 n < 2^24, so any f32
    summation order is exact and a dropped or doubled element (tails, grid-stride seams, the
    misaligned head) changes the result.  The view from element 1 starts 2 / 4 bytes off a
    16-byte boundary."""
    gen = torch.Generator().manual_seed(0)
    for n in SIZES:
        buf = torch.randint(-2, 3, (n + 1,), generator=gen).to(dtype).to(cuda)
        for g in (buf[:n], buf[1:]):
            acc = torch.tensor([5.0, 7.0], device=cuda)
            torch.ops.dtg.grad_sumsq_(g, acc, 0)
            want = torch.tensor([5.0 + float(g.double().pow(2).sum()), 7.0], device=cuda)
            assert torch.equal(acc, want), (n, g.data_ptr() % 16, acc, want)
    acc = torch.tensor([5.0, 7.0], device=cuda)
    torch.ops.dtg.grad_sumsq_(buf[1:], acc, 1)  # the other slot
    assert torch.equal(acc, torch.tensor([5.0, 7.0 + float(buf[1:].double().pow(2).sum())], device=cuda))


def test_sumsq_past_2_31_elements(cuda):
    """Indices past 2^31 (a 32-bit element index would wrap and drop or re-read elements)."""
    n = 2 ** 31 + 11
    g = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    for i in (0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 8, n - 1):
        g[i] = 2.0
    assert torch.equal(_sumsq(g), torch.tensor([20.0, 0.0], device=cuda))
    assert torch.equal(_sumsq(g[1:]), torch.tensor([16.0, 0.0], device=cuda))


# ---------------------------------------------------------------------------------------- A2
def test_sumsq_is_bitwise_reproducible(cuda):
    g = torch.randn(2 ** 20 + 3, generator=torch.Generator().manual_seed(1)).bfloat16().to(cuda)
    a, b = _sumsq(g), _sumsq(g)
    assert torch.equal(a, b) and a[0].item() > 0


# ---------------------------------------------------------------------------------------- A3
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sumsq_propagates_non_finite(cuda, dtype):
    g = torch.ones(4099, dtype=dtype, device=cuda)
    g[4097] = float("inf")
    assert math.isinf(_sumsq(g)[0].item())
    g[17] = float("nan")
    assert math.isnan(_sumsq(g)[0].item())


# ---------------------------------------------------------------------------------------- A4
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sumsq_random_against_float64(cuda, dtype):
    """All terms are non-negative, so the relative error is at most u x the longest chain of
    roundings a term passes through.  n = 2^18 launches 128 workgroups of 256 lanes, one
    8-element vector per lane: 8 roundings in the lane's sum (one per fused multiply-add; one
    more for the square where the compiler does not fuse), 6 wave butterfly adds, 4 adds over
    the waves' sums; the second launch gives each of 128 lanes one partial (added to 0: exact),
    then 6 + 4 adds again, and one add into the accumulator: 8 + 1 + 6 + 4 + 6 + 4 + 1 = 30.
    32 u = 1.9e-6 is asserted, inside the 1e-5 of a 146-add serial sum over the partials."""
    n = 2 ** 18
    g = torch.randn(n, generator=torch.Generator().manual_seed(2)).to(dtype).to(cuda)
    got = _sumsq(g)[0].double().item()
    ref = g.double().pow(2).sum().item()
    rel = abs(got - ref) / ref
    print(f"sumsq {dtype}: relative error {rel:.3e}")
    assert rel <= 32 * U <= 1e-5, rel


# ---------------------------------------------------------------------------------------- A5
def _adam_state(n, cuda, f32_states):
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen).bfloat16().to(cuda)
    g = torch.randn(n, generator=gen).bfloat16().to(cuda)
    sd = torch.float32 if f32_states else torch.bfloat16
    m = (0.1 * torch.randn(n, generator=gen)).to(sd).to(cuda)
    v = (0.01 * torch.rand(n, generator=gen)).to(sd).to(cuda)
    master = p.float() if f32_states else None
    return p, g, m, v, master


@pytest.mark.parametrize("f32_states", [False, True])
@pytest.mark.parametrize("n", [1001, 2 ** 16])
def test_adamw_device_scale(cuda, f32_states, n):
    """gscale = [0.5] with grad_scale 0.25 == grad_scale 0.125 (power-of-two products are exact)."""
    p, g, m, v, master = _adam_state(n, cuda, f32_states)
    a = [t.clone() for t in (p, m, v)] + [None if master is None else master.clone()]
    b = [t.clone() for t in (p, m, v)] + [None if master is None else master.clone()]
    half = torch.tensor([0.5], device=cuda)
    torch.ops.dtg.adamw_(a[0], a[3], g, a[1], a[2], 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.25, None, half)
    torch.ops.dtg.adamw_(b[0], b[3], g, b[1], b[2], 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.125, None, None)
    for x, y in zip(a, b):
        assert x is None or torch.equal(x, y)
    assert not torch.equal(a[0], p)


# ---------------------------------------------------------------------------------------- A6
@pytest.mark.parametrize("f32_states", [False, True])
def test_adamw_t_device_scale(cuda, f32_states):
    rows, cols, tc = 128, 192, 64
    n = rows * cols + 48  # one matrix with a transposed copy, one W^T-less row
    p, g, m, v, master = _adam_state(n, cuda, f32_states)
    mats = torch.tensor([[0, rows, cols, 0, 0], [rows * cols, 1, 48, -1, (rows // 64) * (cols // tc)]],
                        dtype=torch.long, device=cuda)
    ntiles = (rows // 64) * (cols // tc) + 1
    half = torch.tensor([0.5], device=cuda)
    outs = []
    for gs, dev in ((0.25, half), (0.125, None)):
        st = [t.clone() for t in (p, m, v)] + [None if master is None else master.clone()]
        pt = torch.zeros(rows * cols, dtype=torch.bfloat16, device=cuda)
        torch.ops.dtg.adamw_t_(st[0], st[3], g, st[1], st[2], pt, mats, ntiles, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3,
                               gs, None, tc, dev)
        outs.append(st + [pt])
    for x, y in zip(*outs):
        assert x is None or torch.equal(x, y)
    w = outs[0][0][:rows * cols].view(rows, cols)
    assert torch.equal(outs[0][4].view(cols, rows), w.t()) and not torch.equal(outs[0][0], p)


# ---------------------------------------------------------------------------------------- A7
def _engine(cuda, max_grad_norm, weight_t=None):
    from dtg.models import build_model
    from dtg.parallel.data_parallel import DataParallel, FlatAdamW

    torch.manual_seed(0)
    model = build_model("llama-tiny", device=cuda)
    eng = DataParallel(model, mode="single", max_grad_norm=max_grad_norm, weight_t=weight_t)
    return model, eng, FlatAdamW(eng, lr=1e-3)


def _fwd_bwd(model, eng, opt, ids):
    opt.zero_grad()
    eng.backward(model(input_ids=ids, labels=ids).loss)


@pytest.mark.parametrize("weight_t", [True, False])
def test_engine_clips_to_the_global_norm(cuda, weight_t):
    """The reported norm against float64 over the parameters' main_grads, to 1e-5: llama-tiny has
    1.44 M gradients = 705 workgroups, still one vector per lane, and each lane of the second
    launch chains 3 partials, so the sum of squares is within 33 u and the norm (a square root
    halves the relative error, plus its own rounding) within 18 u = 1.1e-6.  The update: a twin
    engine without clipping stepped with grad_scale = the coefficient is bitwise equal (single
    mode has pre_scale = 1, so the kernel's product 1 * coef is exact)."""
    ids = torch.randint(0, 512, (4, 64), generator=torch.Generator().manual_seed(4)).to(cuda)
    model, eng, opt = _engine(cuda, 0.5, weight_t)
    _fwd_bwd(model, eng, opt, ids)
    ref = math.sqrt(sum(p.main_grad.double().pow(2).sum().item() for p in model.parameters()))
    opt.step()
    norm, coef = float(eng.last_grad_norm), float(eng.last_clip_coef)
    print(f"engine norm {norm!r} vs f64 {ref!r}: relative error {abs(norm - ref) / ref:.3e}; coef {coef!r}")
    assert ref > 0.5 and coef < 1.0  # the clip is active
    assert abs(norm - ref) / ref <= 1e-5
    assert coef == pytest.approx(0.5 / (norm + 1e-6), rel=1e-6)

    twin_model, twin, twin_opt = _engine(cuda, None, weight_t)
    _fwd_bwd(twin_model, twin, twin_opt, ids)
    g = twin_opt.param_groups[0]
    twin.step(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale=coef)
    assert twin.last_grad_norm is None
    assert torch.equal(twin.space.grad_buf, eng.space.grad_buf)
    assert torch.equal(twin.space.param_buf, eng.space.param_buf)
    assert torch.equal(twin.exp_avg, eng.exp_avg) and torch.equal(twin.exp_avg_sq, eng.exp_avg_sq)
    if weight_t:
        assert eng._wt_buf is not None and torch.equal(twin._wt_buf, eng._wt_buf)


# ---------------------------------------------------------------------------------------- A8
def test_measure_only_leaves_the_step_unchanged(cuda):
    gen = torch.Generator().manual_seed(5)
    batches = [torch.randint(0, 512, (4, 64), generator=gen).to(cuda) for _ in range(2)]
    bufs = []
    for mgn in (float("inf"), None):
        model, eng, opt = _engine(cuda, mgn)
        for ids in batches:
            _fwd_bwd(model, eng, opt, ids)
            opt.step()
        bufs.append(eng.space.param_buf.clone())
        if mgn is None:
            assert eng.last_grad_norm is None and eng.last_clip_coef is None
        else:
            assert float(eng.last_grad_norm) > 0 and float(eng.last_clip_coef) == 1.0
    assert torch.equal(bufs[0], bufs[1])


# ---------------------------------------------------------------------------------- A9, A10
def _chapter01(tmp_path, name, steps, *flags):
    cmd = [sys.executable, os.path.join(ROOT, "01-single-gpu", "train_llm.py"), "-e", name, "-d", "synthetic",
           "-m", "llama-tiny-d128", "-s", "256", "-b", "2", "--num-samples", "64", "--save-dir", str(tmp_path),
           "--log-freq", "1", "--ckpt-freq", "1000", "--num-workers", "0", "--max-steps", str(steps), *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=os.path.join(ROOT, "01-single-gpu"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    recs = [json.loads(x) for x in (tmp_path / name / "metrics-rank0.jsonl").read_text().splitlines()]
    assert len(recs) == steps
    return recs, out


def test_hip_graph_step_with_clipping_matches_eager(cuda, tmp_path):
    """Past the 3 eager warm-up steps the captured step holds the reduction, the coefficient and
    the scaled update.  The criterion is the one of test_graph_gpu.py's eager-vs-graph test:
    every loss within 2e-3 relative (hipBLASLt may pick other GEMM algorithms inside a capture)."""
    eager, _ = _chapter01(tmp_path, "eager", 8, "--max-grad-norm", "0.5")
    graph, out = _chapter01(tmp_path, "graph", 8, "--max-grad-norm", "0.5", "--hip-graph", "on")
    assert "HIP graph" in out
    assert graph[-1]["time/backward"] == 0.0  # the replayed steps
    for a, b in zip(graph, eager):
        assert abs(a["running_loss"] - b["running_loss"]) <= 2e-3 * abs(b["running_loss"]), (graph, eager)
        assert math.isfinite(a["grad_norm"]) and a["grad_norm"] > 0
        assert 0 < a["grad_clip_coef"] <= 1


def test_cli_end_to_end(cuda, tmp_path):
    recs, _ = _chapter01(tmp_path, "clip", 3, "--max-grad-norm", "1.0")
    for r in recs:
        assert math.isfinite(r["grad_norm"]) and 0 < r["grad_clip_coef"] <= 1, r
    recs, _ = _chapter01(tmp_path, "plain", 3)
    assert all("grad_norm" not in r and "grad_clip_coef" not in r for r in recs)
    recs, _ = _chapter01(tmp_path, "measure", 3, "--log-grad-norm", "on")
    assert all(math.isfinite(r["grad_norm"]) and "grad_clip_coef" not in r for r in recs)
