"""Cases, the f64 yardstick and the checks of `ops.sample_logits`, shared by test_sampler_cpu.py (the CPU
operator) and test_sampler_gpu.py (the HIP kernel).

Yardstick: `ref_row`, a plain numpy f64 evaluation of the definition, one row at a time (np.unique tie
groups, np.cumsum in index order).  It shares no code with dtg.ops._cpu.sample_logits.

Bound: EPS = 2e-5 relative to Z_K.  The kernel's mass error: the f32 product (x - M) * (1 / T) is off by
at most about |arg| * 2.4e-7, the fast exponential adds about |arg| * 6e-8 plus 2 ulp; for every weight
above 4e-8 (|arg| <= 17) that is about 5e-6, and the fixed-point step adds 2^-40: EPS is a 4x margin.

Logits are randn * spread rounded to bf16 (many exact ties, which the cuts must keep); the odd rows of
the f32 case keep their full f32 mantissa so that the third radix level of the f32 kernel decides.
top_p and min_p of the kept-set checks are built from the yardstick so that the cut is unambiguous
(midpoint of the cut tie group's mass interval / geometric midpoint of two adjacent distinct weights);
every check asserts that precondition (half the group's mass, half the relative gap >= 4 EPS) first."""
import functools
import math

import numpy as np
import torch

from dtg import ops
from dtg.ops import _cpu

EPS = 2e-5
MAX_UNCLEAR = 0.02
DRAWS = 4096
NINF = float("-inf")

# name -> (V, spread, rows, dtype, width of the parent tensor (strided view) or None)
CASES = {
    "v1": (1, 4.0, 3, torch.bfloat16, None),
    "v7": (7, 4.0, 4, torch.bfloat16, None),
    "v255": (255, 4.0, 4, torch.bfloat16, None),
    "v256": (256, 4.0, 4, torch.bfloat16, None),
    "v257": (257, 4.0, 4, torch.bfloat16, None),
    "v1025": (1025, 4.0, 3, torch.bfloat16, None),
    "v4099_bf16": (4099, 6.0, 5, torch.bfloat16, None),
    "v4099_f32": (4099, 6.0, 5, torch.float32, None),
    "rime": (156939, 4.0, 2, torch.bfloat16, None),
    "qwen": (151936, 4.0, 2, torch.bfloat16, None),
    "strided": (4000, 6.0, 4, torch.bfloat16, 4096),
}
LARGE = ("rime", "qwen")
SETS = ("none", "k1", "k50", "kV-1", "kV", "p", "m", "all", "mix")


@functools.lru_cache(maxsize=None)
def logits_cpu(name):
    """The case's logits on the CPU (a [n, V] view of a [n, width] tensor for the strided case)."""
    V, spread, n, dtype, width = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    full = torch.randn(n, width or V, generator=g) * spread
    x = full.bfloat16().to(dtype)
    if dtype == torch.float32:
        x[1::2] = full[1::2]
    return x[:, :V]


@functools.lru_cache(maxsize=None)
def logits_on(name, dev):
    V = CASES[name][0]
    return logits_cpu(name)._base.to(dev)[:, :V] if CASES[name][4] else logits_cpu(name).to(dev)


def rows64(name):
    return logits_cpu(name).double().numpy()


def ref_row(x, T, k, top_p, min_p):
    """The definition for one sampled row (finite max, T > 0): dict of the kept mask, the weights, the
    index-order CDF of the kept weights and the thresholds."""
    x = np.where(np.isnan(x), NINF, np.asarray(x, dtype=np.float64))
    V, M = x.size, x.max()
    w = np.exp((x - M) / T)
    t_k = np.sort(x)[::-1][k - 1] if 0 < k < V else NINF
    A = x >= t_k
    t_p = NINF
    if 0 < top_p < 1:
        vals, inv = np.unique(x[A], return_inverse=True)
        mass = np.cumsum(np.bincount(inv, weights=w[A])[::-1])  # mass of {A, x >= value}, values descending
        t_p = vals[::-1][np.argmax(mass >= top_p * w[A].sum())]
    elif top_p <= 0:
        t_p = M
    t_m = M + T * math.log(min_p) if min_p > 0 else NINF
    thr = min(max(t_k, t_p, t_m), M)
    K = x >= thr
    return {"K": K, "w": w, "cdf": np.cumsum(np.where(K, w, 0.0)), "A": A, "M": M}


def clear_top_p(x, T, k, want=0.9):
    """(top_p, half mass): the midpoint of the mass interval of the tie group at which the descending
    mass of A crosses `want`, and half that group's share of Z_A."""
    r = ref_row(x, T, k, 1.0, 0.0)
    xa, wa = np.where(np.isnan(x), NINF, x)[r["A"]], r["w"][r["A"]]
    vals, inv = np.unique(xa, return_inverse=True)
    gm = np.bincount(inv, weights=wa)[::-1] / wa.sum()
    cum = np.cumsum(gm)
    j = int(np.argmax(cum >= want))
    if j == 0:  # the favourite alone reaches `want`: cut after the first group (top_p must be > 0)
        return float(gm[0] / 2), float(gm[0] / 2)
    return float(cum[j] - gm[j] / 2), float(gm[j] / 2)


def clear_min_p(x, T, want=0.05):
    """(min_p, half relative gap): the geometric midpoint of the two adjacent distinct weights around
    `want` (the two smallest when none is below it); a row with one distinct weight keeps `want`."""
    w = np.unique(ref_row(x, T, 0, 1.0, 0.0)["w"])
    if w.size < 2:
        return want, math.inf
    j = min(max(int(np.searchsorted(w, want)), 1), w.size - 1)  # w[j - 1] < want <= w[j] where possible
    lo, hi = w[j - 1], w[j]
    return float(math.sqrt(lo * hi)), float((hi - lo) / hi / 2)


def param_set(name, which):
    """Per-row lists (T, top_k, top_p, min_p), and the smallest precondition figure of the set."""
    V, _, n, _, _ = CASES[name]
    x = rows64(name)
    T, K, P, Mn = [1.0] * n, [0] * n, [1.0] * n, [0.0] * n
    room = math.inf
    kinds = [which] * n
    if which == "mix":
        kinds = ["greedy", "k50", "p", "all", "m", "none", "k1", "all"][:n]
        T = [0.0, 0.7, 1.3, 0.9, 1.0, 1.0, 1.0, 1.0][:n]
    for i, kind in enumerate(kinds):
        if kind in ("k1", "k50", "kV-1", "kV", "all"):
            K[i] = {"k1": 1, "k50": 50, "kV-1": V - 1, "kV": V, "all": 50}[kind]
        if kind in ("p", "all"):
            P[i], half = clear_top_p(x[i], T[i], K[i])
            room = min(room, half)
        if kind in ("m", "all"):
            Mn[i], half = clear_min_p(x[i], T[i])
            room = min(room, half)
    return T, K, P, Mn, room


def run(dev, logits, T, K, P, Mn, u=None, **rng):
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
    ids, kept = ops.sample_logits(logits, t(T, torch.float32), t(K, torch.int32), t(P, torch.float32), t(Mn, torch.float32),
                                  u=None if u is None else t(u, torch.float32), **rng)
    assert ids.dtype == torch.int64 and kept.dtype == torch.int32 and ids.device == logits.device
    return ids.cpu().numpy(), kept.cpu().numpy()


# ---- check 1: the kept set, exact
def check_kept(name, which, dev):
    T, K, P, Mn, room = param_set(name, which)
    print(f"[sampler] {name}/{which}: smallest half mass / half gap {room:.3g} (needs >= {4 * EPS:.1g})")
    assert room >= 4 * EPS, f"{name}/{which}: the cut is not clear ({room})"
    x = rows64(name)
    n = x.shape[0]
    u = np.random.default_rng(7).random(n).astype(np.float32)
    ids, kept = run(dev, logits_on(name, dev), T, K, P, Mn, u=u.tolist())
    for i in range(n):
        if T[i] <= 0:
            assert (ids[i], kept[i]) == (int(np.argmax(x[i])), 1), f"greedy row {i}"
            continue
        r = ref_row(x[i], T[i], K[i], np.float32(P[i]), np.float32(Mn[i]))
        assert kept[i] == int(r["K"].sum()), f"{name}/{which} row {i}: kept {kept[i]} != {int(r['K'].sum())}"
        assert 0 <= ids[i] < x.shape[1] and r["K"][ids[i]], f"{name}/{which} row {i}: id {ids[i]} outside K"


# ---- check 2: the draw, with explicit u
def judge_draws(r, u, ids):
    """Number of non-clear draws; asserts the rule of every draw.  `r` = ref_row of the row."""
    cdf, K = r["cdf"], r["K"]
    Z = cdf[-1]
    kept_idx = np.flatnonzero(K)
    kc = cdf[kept_idx]                                   # CDF at the kept ids, increasing
    target = u.astype(np.float64) * Z
    j = np.minimum(np.searchsorted(kc, target, side="right"), kept_idx.size - 1)
    lower = np.where(j > 0, kc[np.maximum(j - 1, 0)], -np.inf)  # nothing lies below the first interval
    upper = np.where(j < kept_idx.size - 1, kc[j], np.inf)      # nor above the last
    near_lo, near_hi = target - lower <= EPS * Z, upper - target <= EPS * Z
    ref_id = kept_idx[j]
    lo_id, hi_id = kept_idx[np.maximum(j - 1, 0)], kept_idx[np.minimum(j + 1, kept_idx.size - 1)]
    ok = (ids == ref_id) | (near_lo & (ids == lo_id)) | (near_hi & (ids == hi_id))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{bad.size} draws off: u {u[bad][:4]}, got {ids[bad][:4]}, want {ref_id[bad][:4]} "
                           f"(clear: {(~(near_lo | near_hi))[bad][:4]})")
    return int((near_lo | near_hi).sum())


def draw_setup(name, draws):
    """Rows of the case repeated to `draws` rows, one parameter set per source row, none greedy."""
    V, _, n, _, _ = CASES[name]
    kinds = (["k50", "all"] if name in LARGE else ["none", "k50", "p", "all", "m"])[:n]
    x = rows64(name)
    src = np.arange(draws) % len(kinds)
    per = {}
    for i, kind in enumerate(kinds):
        k = 50 if kind in ("k50", "all") else 0
        p = clear_top_p(x[i], 1.0, k)[0] if kind in ("p", "all") else 1.0
        m = clear_min_p(x[i], 1.0)[0] if kind in ("m", "all") else 0.0
        per[i] = (1.0, k, float(np.float32(p)), float(np.float32(m)))
    return src, per


def check_draws(name, dev, draws=DRAWS, chunk=None, fallback=False):
    src, per = draw_setup(name, draws)
    u = np.random.default_rng(11).random(draws).astype(np.float32)
    T, K, P, Mn = ([per[i][c] for i in src] for c in range(4))
    lg = logits_on(name, dev)
    ids = np.empty(draws, dtype=np.int64)
    chunk = chunk or draws
    for a in range(0, draws, chunk):
        b = min(draws, a + chunk)
        rows = lg[torch.as_tensor(src[a:b], device=dev)]
        ids[a:b], _ = run(dev, rows, T[a:b], K[a:b], P[a:b], Mn[a:b], u=u[a:b].tolist())
    x = rows64(name)
    unclear = 0
    for i, (t, k, p, m) in per.items():
        sel = src == i
        unclear += judge_draws(ref_row(x[i], t, k, np.float32(p), np.float32(m)), u[sel], ids[sel])
    print(f"[sampler] {name}{' (torch path)' if fallback else ''}: {unclear} of {draws} draws not clear "
          f"({100.0 * unclear / draws:.2f} %)")
    assert unclear <= MAX_UNCLEAR * draws, f"{name}: {unclear} of {draws} draws are not clear"


# ---- check 3: the Philox draw
def check_philox(dev):
    name = "v257"
    n = CASES[name][2]
    seed, streams, steps = (1 << 40) + 12345, [3, (1 << 33) + 1, 7, (1 << 62) + 5], [(1 << 32) + 9, 0, (1 << 35), 1]
    w0 = _cpu.philox4x32_10(*[np.array([v & 0xFFFFFFFF for v in a], dtype=np.uint64) if lo else
                              np.array([v >> 32 for v in a], dtype=np.uint64)
                              for a, lo in ((steps, 1), (steps, 0), (streams, 1), (streams, 0))],
                            seed & 0xFFFFFFFF, seed >> 32)[0]
    u = ((w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))
    assert np.array_equal(u, _cpu.sample_u(torch.tensor([[seed, a, b] for a, b in zip(streams, steps)])).numpy())
    assert len(set(u.tolist())) == n and ((0 <= u) & (u < 1)).all()
    args = ([1.0] * n, [0] * n, [1.0] * n, [0.0] * n)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    a = run(dev, logits_on(name, dev), *args, seed=seed, stream=t64(streams), step=t64(steps))
    b = run(dev, logits_on(name, dev), *args, u=u.tolist())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = run(dev, logits_on(name, dev), *args, seed=seed + (1 << 32), stream=t64(streams), step=t64(steps))
    assert not np.array_equal(a[0], c[0]), "the seed's high word does not reach the draw"


# ---- check 4: a row's result depends on that row alone, bitwise
def check_row_independence(dev):
    for name in ("v4099_bf16", "v4099_f32", "v257"):
        lg = logits_on(name, dev)
        V = lg.shape[1]
        T, K, P, Mn, _ = param_set(name, "all")
        g = torch.Generator().manual_seed(3)
        others = (torch.randn(8, V, generator=g) * 5).to(lg.dtype).to(dev)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
        alone = ops.sample_logits(lg[2:3], T[2], K[2], P[2], Mn[2], seed=9, stream=t([17], torch.int64), step=4)
        batch = others.clone()
        batch[5] = lg[2]
        col = lambda v, other, dt: t([other] * 5 + [v] + [other] * 2, dt)  # noqa: E731
        kw = dict(temperature=col(T[2], 0.5, torch.float32), top_k=col(K[2], 3, torch.int32),
                  top_p=col(P[2], 0.5, torch.float32), min_p=col(Mn[2], 0.2, torch.float32), seed=9,
                  stream=col(17, 1, torch.int64), step=4)
        mid = ops.sample_logits(batch, **kw)
        rev = ops.sample_logits(batch.flip(0), **{k: v.flip(0) if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
        again = ops.sample_logits(batch, **kw)
        for j in range(2):
            assert torch.equal(alone[j], mid[j][5:6]), f"{name}: row alone != row 5 of 8"
            assert torch.equal(mid[j], rev[j].flip(0)), f"{name}: reversed batch differs"
            assert torch.equal(mid[j], again[j]), f"{name}: two identical calls differ"


# ---- check 5: the distribution of the Philox draws
CHI2_15_Q = 56.4934  # chi-square quantile 1 - 1e-6 at 15 degrees of freedom


def check_distribution(dev):
    """8,192 (stream, step) pairs of seed 2024 on one 16-id row; the statistic is 17.13 with the CPU
    operator (the median of chi-square(15) is 14.3), far below the quantile."""
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(16, generator=g) * 1.5).bfloat16()
    n = 8192
    i = torch.arange(n, dtype=torch.int64, device=dev)
    ids, kept = ops.sample_logits(row.to(dev)[None].expand(n, 16), 1.0, seed=2024, stream=i % 128, step=i // 128)
    assert bool((kept == 16).all())
    counts = np.bincount(ids.cpu().numpy(), minlength=16)
    p = ref_row(row.double().numpy(), 1.0, 0, 1.0, 0.0)["w"]
    p = p / p.sum()
    stat = float(((counts - n * p) ** 2 / (n * p)).sum())
    print(f"[sampler] chi-square over 16 ids, {n} draws: {stat:.2f} (bound {CHI2_15_Q})")
    assert stat < CHI2_15_Q, stat


# ---- check 6: edges
def check_edges(dev):
    inf, nan = float("inf"), float("nan")
    V = 300
    g = torch.Generator().manual_seed(8)
    base = (torch.randn(V, generator=g) * 2).bfloat16().float()
    base[123] = 30.0  # a clear leader
    t = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731

    def one(row, dtype=torch.bfloat16, **kw):
        ids, kept = ops.sample_logits(row.to(dtype).to(dev)[None], **kw)
        return int(ids[0]), int(kept[0])

    for dtype in (torch.bfloat16, torch.float32):
        assert one(torch.full((V,), -inf), dtype, temperature=1.0) == (-1, 0)
        assert one(torch.full((V,), nan), dtype, temperature=1.0) == (-1, 0)
        assert one(torch.full((V,), -inf), dtype, temperature=0.0) == (-1, 0)
        row = base.clone()
        row[[7, 200]] = inf
        assert one(row, dtype, temperature=1.0, top_k=5, top_p=0.5) == (7, 2)
        assert one(row, dtype) == (7, 2)
        row = base.clone()
        row[5], row[123] = nan, nan  # the leader is NaN: it is never picked
        for u in (0.0, 0.5, 0.999999):
            i, k = one(row, dtype, temperature=t([5.0]), u=t([u]))
            assert i not in (5, 123) and 0 <= i < V and k == V
        i, k = one(row, dtype, temperature=0.0)
        assert (i, k) == (int(torch.where(torch.isnan(row), torch.full_like(row, -inf), row).argmax()), 1)
        assert one(base, dtype, temperature=0.0) == (123, 1)
        assert one(base, dtype, temperature=t([1e-6]), u=t([0.7]))[0] == 123
        assert one(base, dtype, temperature=t([nan])) == (123, 1)
        assert one(base, dtype, temperature=t([-1.0])) == (123, 1)
        # top_k beyond V and negative top_k: no top-k filter
        for k in (V + 5, 1 << 30, -3):
            assert one(base, dtype, temperature=t([3.0]), top_k=t([k], torch.int32), u=t([0.3]))[1] == V
        # top_p 0: only the entries equal to the max; 1 and NaN: off
        assert one(base, dtype, temperature=t([3.0]), top_p=t([0.0]), u=t([0.9])) == (123, 1)
        assert one(base, dtype, temperature=t([3.0]), top_p=t([-1.0]), u=t([0.9])) == (123, 1)
        assert one(base, dtype, temperature=t([3.0]), top_p=t([1.0]), u=t([0.3]))[1] == V
        assert one(base, dtype, temperature=t([3.0]), top_p=t([nan]), u=t([0.3]))[1] == V
        # min_p 1 (and beyond): only the entries equal to the max, the argmax always stays
        assert one(base, dtype, temperature=t([3.0]), min_p=1.0, u=t([0.9])) == (123, 1)
        assert one(base, dtype, temperature=t([3.0]), min_p=t([7.0]), u=t([0.9])) == (123, 1)
        assert one(base, dtype, temperature=t([3.0]), min_p=t([nan]), u=t([0.3]))[1] == V
        tie = base.clone()
        tie[250] = 30.0
        assert one(tie, dtype, temperature=t([3.0]), top_p=t([0.0]), u=t([0.9])) == (250, 2)
        assert one(tie, dtype, temperature=t([3.0]), top_k=1, u=t([0.1])) == (123, 2)  # ties at the cut are kept
        assert one(tie, dtype, temperature=0.0) == (123, 1)
        # u at and beyond its range: the first / last kept id
        i, k = one(base, dtype, temperature=t([3.0]), top_k=4, u=t([1.0]))
        assert k >= 4 and 0 <= i < V and i == int(torch.topk(base, k).indices.max())  # the last id of K
        ids, kept = ops.sample_logits(torch.empty(0, V, dtype=dtype, device=dev), 1.0)
        assert ids.shape == (0,) and kept.shape == (0,) and ids.dtype == torch.int64 and kept.dtype == torch.int32
    # mixed rows in one call, all parameter edges at once: nothing faults, every id is in range
    rows = torch.stack([base, torch.full((V,), -inf), tie, base.neg(), base * 1e30, base]).to(dev)
    ids, kept = ops.sample_logits(rows, t([0.0, 1.0, inf, 1e-30, 1.0, 1e30]), t([0, 5, -1, 1 << 31 - 1, 2, V], torch.int32),
                                  t([0.5, nan, 0.0, 1.0, 1e-30, 0.999999]), t([0.0, inf, nan, 1.0, 1e-30, 0.0]), seed=-1,
                                  step=-1)
    assert ids.tolist()[:2] == [123, -1] and kept.tolist()[:2] == [1, 0]
    assert all(0 <= i < V for i in ids.tolist()[2:]) and all(1 <= k <= V for k in kept.tolist()[2:])
    for bad in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(min_p=-0.1),
                dict(min_p=1.5), dict(temperature=nan)):
        try:
            ops.sample_logits(rows, **bad)
        except ValueError:
            continue
        raise AssertionError(f"{bad} was accepted")
