"""The gfx950 kernels of csrc/kernels/flash_attn.hip against the float64 references and bounds of
tests/_flash_cases.py (the cases test_flash_attn_cpu.py runs through the CPU operators).  Every test
prints [numerics] lines: the largest error in bf16 ulps and the largest error / bound per sequence."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the env-knob child process: no conftest has set the path up
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import _flash_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

OK_LINE = "flash env knobs ok"


@pytest.mark.parametrize("layout,max_seqlen", [("pad8", None), ("fused", 300)], ids=["pad8-tight", "fused-ms300"])
@pytest.mark.parametrize("name", C.EDGE)
def test_edge_length_pack(cuda, name, layout, max_seqlen):
    C.check_case(name, cuda, "edge", layout, max_seqlen)


@pytest.mark.parametrize("name", C.HEADS)
def test_head_maps(cuda, name):
    C.check_case(name, cuda, "heads")


@pytest.mark.parametrize("name", ["edge_A_c_d128", "edge_B_c_d64", "edge_A_nc_d64", "edge_B_nc_d128"])
def test_backward_tuning(cuda, name):
    knobs = [(s, qb) for s in (0, 1, 2, 3, 8) for qb in (32, 64)]
    c = C.make_case(name)
    assert C.planned_nsplit(c, 0, max(c["lens"])) > 1  # kv_split = 0: the plan itself splits this case
    C.check_tuning(name, cuda, knobs)


def test_env_only_kernels(cuda):
    """DTG_FA_OCC=2 and DTG_FA_KV_PF=2 are read when the extension loads: one fresh child process runs the
    checker on the edge-length packs and the key-range cases with both set."""
    env = dict(os.environ, DTG_FA_OCC="2", DTG_FA_KV_PF="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and OK_LINE in r.stdout.splitlines(), (r.stdout + r.stderr)[-3000:]
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("[summary]")))


@pytest.mark.parametrize("name", C.WINDOW)
def test_sliding_window(cuda, name):
    C.check_case(name, cuda, "window")


def test_window_identities(cuda):
    C.check_window_identities(cuda)


@pytest.mark.parametrize("name", C.LOGIT)
def test_logit_range(cuda, name):
    C.check_case(name, cuda, "logit")


@pytest.mark.parametrize("name", C.KR)
def test_key_ranges(cuda, name):
    C.check_case(name, cuda, "key_ranges")


@pytest.mark.parametrize("name", C.DROP)
def test_dropout(cuda, name):
    C.check_drop(name, cuda)


def test_dropout_p0_meets_the_plain_bound(cuda):
    C.check_p0_is_plain(cuda)


@pytest.mark.parametrize("D", [64, 128])
def test_exact_mask_probes(cuda, D):
    C.check_mask_probes(cuda, D)


@pytest.mark.parametrize("name", C.ROPE)
def test_fused_rope_backward(cuda, name):
    from dtg import ops

    c = C.make_case(name)
    for split in (0, 1):
        with ops.fa_tuning(cuda, kv_split=split):
            C.check_bwd(c, cuda, f"rope split{split}", "fused", None, kv_split=split)


def test_fused_dropout_backward(cuda):
    C.check_bwd(C.make_case("drop_0.1_c_d128"), cuda, "dropout fused", "fused")


def test_public_attention(cuda):
    C.check_public_attention("edge_A_c_d128", cuda)
    C.check_public_attention("edge_B_nc_d64", cuda)


def test_refusals_and_empties(cuda):
    C.check_refusals_and_empties(cuda)


def _print_summary():
    for (fam, out), (ulps, ratio) in sorted(C.report().items()):
        print(f"[summary] {fam} {out}: max {ulps:.3f} bf16 ulp, max err/bound {ratio:.3f}")


@pytest.fixture(scope="module", autouse=True)
def _numerics_summary():
    """After the module's tests: what those that ran measured, per case family and output."""
    yield
    _print_summary()


def _child():
    assert os.environ.get("DTG_FA_OCC") == "2" and os.environ.get("DTG_FA_KV_PF") == "2"
    dev = torch.device("cuda:0")
    C.check_edge_pack(dev, "env")
    # Key ranges under DTG_FA_KV_PF=2: a range with keys and no queries gives its key blocks zero items,
    # which the two-ahead dK/dV prologue cannot take (it loads items 0 and 1 unconditionally); the launch
    # plan gives key-range calls the single-set loop instead (tests/native/fa_plan_check.cpp pins it).
    for name in C.KR:
        C.check_case(name, dev, "env key_ranges")
    torch.cuda.synchronize()
    _print_summary()
    print(OK_LINE)


if __name__ == "__main__":
    _child()
