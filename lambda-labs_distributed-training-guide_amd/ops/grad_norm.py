"""Global gradient norm and clip coefficient on the device (HIP reduction on GPU, reference on CPU).

Nothing here reads a device value on the host, so a step that clips stays free of host syncs and
can be captured in a HIP graph (the only host values baked in are `max_norm` and `pre_scale`)."""
import math

import torch


def grad_sumsq_(g, acc, slot=0):
    """acc[slot] += sum(g^2): g a contiguous 1-D bf16 / f32 buffer, acc f32 on the same device.
    Accumulated in f32, bitwise reproducible run to run; NaN / inf in g propagate."""
    torch.ops.dtg.grad_sumsq_(g, acc, int(slot))


def clip_coef_(stats, sumsq, max_norm, pre_scale=1.0):
    """stats[0] = norm = sqrt(sumsq) * pre_scale; stats[1] = coef = min(1, max_norm / (norm + 1e-6)).

    `sumsq` is a device f32 scalar, `stats` a persistent device f32 [2] (written in place, so a
    captured graph and the AdamW kernels keep reading the same addresses).  `pre_scale` is the
    engine's averaging factor: the norm is that of the averaged gradient g * pre_scale.  As in
    torch.nn.utils.clip_grad_norm_, a NaN norm gives a NaN coefficient and an inf norm gives 0.
    max_norm = inf measures only: coef is exactly 1 whatever the norm."""
    norm = sumsq.sqrt() * float(pre_scale)
    stats[0:1].copy_(norm.reshape(1))
    if math.isinf(max_norm):
        stats[1:2].fill_(1.0)
    else:
        stats[1:2].copy_((float(max_norm) / (norm + 1e-6)).clamp(max=1.0).reshape(1))
    return stats
