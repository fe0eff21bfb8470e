"""Global-norm gradient clipping shared by the engines (DataParallel, FullyShard).

An engine hands over the pieces of its final (reduced, not yet averaged) flat gradient it owns,
each tagged with a slot:
  slot 0  gradients of parameters sharded over tensor parallel (and everything without TP):
          every TP rank holds a different part, so the sums are added over the TP group;
  slot 1  gradients of TP-replicated (sequence-parallel) parameters: identical on every TP rank
          once reduced, so they are counted once and never summed over TP.
Both slots are summed over the data-parallel group when the ranks own disjoint shards (ZeRO,
FSDP).  The scalar collectives are plain `torch.distributed.all_reduce` on the process groups
(never the direct-peer xGMI path, whose summation order depends on the rank), so every rank
ends up with a bit-identical coefficient.  Nothing is read back to the host: the coefficient
reaches AdamW as a device scalar (`gscale`), the norm is read only when the trainer logs it.
"""
from __future__ import annotations

import math
from typing import Iterable, Tuple

import torch
import torch.distributed as dist

from ..ops.grad_norm import clip_coef_, grad_sumsq_


class GradClip:
    def __init__(self, max_norm: float, device, shard_group=None, sharded: bool = False, tp_group=None):
        """max_norm: clip to this global L2 norm; inf = measure only.  `sharded`: the ranks of
        `shard_group` own disjoint gradient shards (their sums are added)."""
        max_norm = float(max_norm)
        if not max_norm > 0:
            raise ValueError(f"max_grad_norm must be > 0 (inf measures only, None turns it off), got {max_norm}")
        self.max_norm = max_norm
        self.measure_only = math.isinf(max_norm)
        self.shard_group = shard_group
        self.sharded = bool(sharded) and dist.is_initialized() and dist.get_world_size(shard_group) > 1
        tp_on = tp_group is not None and dist.is_initialized() and dist.get_world_size(tp_group) > 1
        self.tp_group = tp_group if tp_on else None
        self.acc = torch.zeros(2, dtype=torch.float32, device=device)  # [sharded over TP, TP-replicated]
        self.stats = torch.tensor([0.0, 1.0], dtype=torch.float32, device=device)  # [norm, coef]

    @property
    def norm(self) -> torch.Tensor:
        return self.stats[0]

    @property
    def coef(self) -> torch.Tensor:
        return self.stats[1]

    @property
    def gscale(self):
        """AdamW's device gradient scale: None when only measuring (the update stays bit-identical)."""
        return None if self.measure_only else self.stats[1:2]

    @torch.no_grad()
    def update(self, pieces: Iterable[Tuple[torch.Tensor, int]], pre_scale: float):
        """Norm of the averaged gradient (pieces * pre_scale) and the clip coefficient."""
        self.acc.zero_()
        for g, slot in pieces:
            if g.numel():
                grad_sumsq_(g, self.acc, slot)
        if self.sharded:
            dist.all_reduce(self.acc, group=self.shard_group)
        if self.tp_group is not None:
            dist.all_reduce(self.acc[0:1], group=self.tp_group)
        clip_coef_(self.stats, self.acc[0] + self.acc[1], self.max_norm, pre_scale)
        return self.gscale
