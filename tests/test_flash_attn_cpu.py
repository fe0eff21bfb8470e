"""What tests/_flash_cases.py can show without a GPU: the package's CPU attention operators against the
float64 references and bounds (references and operators check each other), a float64 emulation of the
kernels' bf16 operand rounding inside the bounds (the bounds admit the design), deliberately wrong
references outside them (the bounds are not vacuous), and Philox4x32-10 -- the cases' and the
package's -- against the Random123 known answers."""
import numpy as np
import pytest
import torch

import _flash_cases as C
from _refs import round_bf16

CPU = torch.device("cpu")
ALL = C.EDGE + C.HEADS + C.WINDOW + C.LOGIT + C.KR + C.DROP + C.ROPE + ["window_64_noncausal"]


def test_philox_known_answers():
    from dtg.ops import _cpu

    for ctr, key, want in C.PHILOX_KAT:
        mine = [int(x[0]) for x in C.philox([np.array([x]) for x in ctr], key)]
        theirs = [int(np.asarray(x).reshape(-1)[0]) for x in _cpu.philox4x32_10(*[np.array([x]) for x in ctr], *key)]
        assert tuple(mine) == want, [hex(x) for x in mine]
        assert tuple(theirs) == want, [hex(x) for x in theirs]


def test_keep_mask_layout_matches_the_package():
    from dtg.ops import _cpu

    for p, s0, off in ((0.1, 0, 7), (0.5, 5, 9 + (1 << 33)), (0.999, 34, 77), (0.0, 3, 1)):
        for head in (0, 2):
            assert torch.equal(C.keep_mask(0x123456789AB, off, head, s0, 13, 22, p),
                               _cpu.dropout_keep(0x123456789AB, off, head, s0, 13, 22, p))
    assert C.drop_thr(0.0) == 256 and C.drop_thr(0.999) == 1 and C.drop_thr(0.5) == 128


@pytest.mark.parametrize("name", ALL)
def test_cpu_operators_within_bounds(name):
    layout = "fused" if name in C.ROPE or name.endswith("d128") else "pad8"
    C.check_case(name, CPU, "cpu", layout, 300 if layout == "fused" else None)


def test_cpu_window_identities_p0_probes_and_refusals():
    C.check_window_identities(CPU)
    C.check_p0_is_plain(CPU)
    C.check_mask_probes(CPU, splits=(1,))
    C.check_refusals_and_empties(CPU)
    C.check_public_attention("edge_A_c_d64", CPU)


def _as_outputs(r):
    out = {n: round_bf16(r[n]).to(torch.bfloat16) for n in ("o", "dq", "dk", "dv")}
    out["lse"] = r["lse"].float()
    return out


@pytest.mark.parametrize("name", ALL)
def test_bf16_emulation_within_bounds(name):
    """The reference with P and dS rounded to bf16 where the kernels pack them."""
    c = C.make_case(name)
    r = C.reference(c, emulate=True, given=(c["ref"]["o_in"], c["ref"]["lse_in"]))
    C.compare(c, c["ref"], _as_outputs(r), "emulation")


MUTANTS = [("causal_off1", "edge_A_c_d64"), ("win_lo", "window_64"), ("win_hi", "window_64"), ("win_lo", "window_2"),
           ("win_hi", "window_129"), ("last_key", "edge_A_nc_d64"), ("last_key", "edge_B_c_d128"),
           ("kv_item_row", "edge_B_c_d64"), ("gqa_head", "heads_4_2"), ("gqa_head", "heads_8_1"),
           ("delta_neighbour", "heads_4_4"), ("dk_scale2", "edge_A_c_d128"), ("head_order", "heads_6_2"),
           ("kstart_off1", "kr_off"), ("kstart_off1", "kr_diag"), ("drop_shift", "drop_0.5_c_d64"),
           ("drop_s0", "drop_0.5_c_d64"), ("drop_s0", "drop_0.1_nc_d128"), ("dv_rescale", "drop_0.1_c_d64"),
           ("rope_sign", "rope_B_d64")]


ALL4 = ("o", "dq", "dk", "dv")
# the outputs each mistake reaches: every one of them, on its own, must leave the bound
TARGETS = {"causal_off1": ALL4 + ("lse",), "win_lo": ALL4, "win_hi": ALL4, "last_key": ALL4, "kv_item_row": ("dk", "dv"),
           "gqa_head": ("dk", "dv"), "delta_neighbour": ("dq", "dk"), "dk_scale2": ("dk",), "head_order": ALL4,
           "kstart_off1": ALL4, "drop_shift": ALL4, "drop_s0": ALL4, "dv_rescale": ("dv",), "rope_sign": ("dq", "dk")}


@pytest.mark.parametrize("mut,name", MUTANTS, ids=[f"{m}-{n}" for m, n in MUTANTS])
def test_bounds_reject_mutant(mut, name):
    """A reference with one deliberate mistake, rounded like a kernel output, must fall outside the bound in
    every output the mistake reaches."""
    c = C.make_case(name)
    outs = _as_outputs(C.reference(c, mut=mut, given=(c["ref"]["o_in"], c["ref"]["lse_in"])))
    for n in TARGETS[mut]:
        with pytest.raises(AssertionError, match=rf"\|{n}\|"):
            C.compare(c, c["ref"], {n: outs[n]}, f"mutant {mut}")
