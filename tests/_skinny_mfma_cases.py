"""Shapes, refusals and prompts shared by test_skinny_mfma_cpu.py and test_skinny_mfma_gpu.py."""
import torch

import _generate_cases as gc
import _skinny_cases as sc

# (M, N, K) with the kernel's W = 8 waves and U = 8 slabs per pass: one slab (seven waves add zero); one slab
# per wave and a second M tile of one row; N one past a tile with one full pass plus one slab (32 W U + 32);
# three M tiles, partial both ways; four M tiles, several workgroups; a long K.
SHAPES = [(1, 1, 32), (17, 16, 256), (16, 17, 2080), (33, 67, 4128), (64, 130, 4096), (48, 2, 14336)]


def raw_refusals(dev):
    """name -> call of the raw operator that must raise RuntimeError("dtg: ...")."""
    x, w, b = sc.inputs(4, 10, 64, dev)
    op, z = torch.ops.dtg.skinny_linear_mfma, lambda *s: torch.zeros(*s, dtype=x.dtype, device=dev)
    return {
        "M = 0": lambda: op(x[:0], w, b, 0),
        "M = 65": lambda: op(z(65, 64), w, b, 0),
        "K % 32": lambda: op(x[:, :48].contiguous(), w[:, :48].contiguous(), b, 0),
        "f32 x": lambda: op(x.float(), w, b, 0),
        "f32 w": lambda: op(x, w.float(), b, 0),
        "non-contiguous w": lambda: op(x, z(64, 10).t(), b, 0),
        "misaligned x": lambda: op(z(4, 72)[:, 1:65], w, b, 0),
        "odd N with act": lambda: op(x, w[:9].contiguous(), None, 1),
        "bias length": lambda: op(x, w, b[:9].contiguous(), 0),
        "act = 2": lambda: op(x, w, b, 2),
    }


def prompts(n):
    g = torch.Generator().manual_seed(n)
    return [torch.randint(0, gc.VOCAB, (5 + i % 9,), generator=g) for i in range(n)]
