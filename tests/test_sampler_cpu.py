"""ops.sample_logits on the CPU (dtg.ops._cpu.sample_logits, the f64 form of the definition) against the
independent yardstick of _sampler_cases.py.  The two full-vocabulary cases draw 256 values here instead
of 4,096: the f64 operator sorts every repeated row again, and 4,096 rows of 150k ids take minutes."""
import pytest
import torch

import _sampler_cases as sc

DEV = torch.device("cpu")


@pytest.mark.parametrize("which", sc.SETS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_kept_set(name, which):
    sc.check_kept(name, which, DEV)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_draws(name):
    if name in sc.LARGE:
        sc.check_draws(name, DEV, draws=256, chunk=32)
    else:
        sc.check_draws(name, DEV, chunk=512)


def test_philox_draw():
    sc.check_philox(DEV)


def test_row_independence():
    sc.check_row_independence(DEV)


def test_distribution():
    sc.check_distribution(DEV)


def test_edges():
    sc.check_edges(DEV)
