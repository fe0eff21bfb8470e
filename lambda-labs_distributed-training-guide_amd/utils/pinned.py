"""Exact-size page-locked host buffers for CPU offload (chapter 05).

`torch.zeros(..., pin_memory=True)` goes through PyTorch's caching host allocator, which rounds
every block up to the next power of two.  For the 405B offload shards that is ruinous: one
rank of an 8-GPU job holds a 101 GB bf16 parameter shard and a 101 GB gradient shard, and each
would be rounded up to 137 GB -- 72 GB of host RAM per rank lost to padding, on a host whose
eight ranks already need ~406 GB each for the offloaded training state.

`pinned_zeros` instead allocates page-locked host memory of the exact size with hipHostMalloc
(csrc/comm/host_mem.hip), so the copy engines DMA straight from / into it (`non_blocking=True`
copies stay asynchronous).  The memory is born pinned: nothing is registered after the fact
(hipHostRegister of pages the process already owns is not supported on every host, a virtual
machine for one, and its failure stays behind as the next launch's error).  The memory is freed
when the storage is (after the device drains), however many views of it are still around until
then.  Without a GPU the buffer is returned pageable; with one, a failed allocation raises.
"""
from __future__ import annotations

import atexit

import torch

_EXIT_HOOK = False


def pinned_zeros(n: int, dtype: torch.dtype) -> torch.Tensor:
    global _EXIT_HOOK
    n = int(n)
    if n == 0 or not torch.cuda.is_available():
        return torch.zeros(n, dtype=dtype)
    from ..ops import _native

    _native.require()
    torch.cuda.init()  # until PyTorch has initialised the device, `is_pinned()` answers False for any memory
    if not _EXIT_HOOK:
        # never free at interpreter exit (the device drain then can hang); process exit frees it
        atexit.register(torch.ops.dtg_host.keep_at_exit)
        _EXIT_HOOK = True
    esz = torch.empty((), dtype=dtype).element_size()
    return torch.ops.dtg_host.pinned_zeros(n * esz).view(dtype)
