"""KV block copy for the fork of a prompt's KV (csrc/kernels/kv_copy.hip): one launch copies whole
blocks inside every K and V cache of every layer.  Bytes, so bf16 and FP8 caches are one kernel."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import native, reference

MAX_PAIRS = 32  # (src, dst) pairs of one launch: they travel by value in the launch arguments


def _tensors(kv_caches) -> List[torch.Tensor]:
    return [t for kv in kv_caches for t in kv]


def block_bytes(kv_caches) -> int:
    """Bytes of one block in every cache tensor (K and V blocks are equally long contiguous runs)."""
    t = kv_caches[0][0]
    return t[0].numel() * t.element_size()


def pointer_table(kv_caches) -> Optional[torch.Tensor]:
    """Device table of the ``2 x layers`` cache base pointers, built once when the caches are
    allocated (None for CPU caches: the reference copy takes the tensors)."""
    ts = _tensors(kv_caches)
    if not ts or not ts[0].is_cuda:
        return None
    bb, nb = block_bytes(kv_caches), ts[0].shape[0]
    for t in ts:
        if not t.is_contiguous() or t.shape[0] != nb or t[0].numel() * t.element_size() != bb:
            raise ValueError("kv_copy_blocks: every cache must be contiguous with equal block bytes")
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=ts[0].device)


def try_copy_blocks(kv_caches, pairs: Sequence[Tuple[int, int]], table: Optional[torch.Tensor] = None) -> int:
    """The launcher's return code: 0, or -1 for a refused call (nothing launched)."""
    ts = _tensors(kv_caches)
    if not ts[0].is_cuda:
        try:
            reference.kv_copy_blocks(kv_caches, pairs)
        except ValueError:
            return -1
        return 0
    if table is None:
        table = pointer_table(kv_caches)
    flat = [int(x) for p in pairs for x in p]
    arr = (ctypes.c_int * max(1, len(flat)))(*flat)
    return native.lib().pk_kv_copy_blocks(table.data_ptr(), len(ts), block_bytes(kv_caches), ts[0].shape[0], arr,
                                          len(pairs), native.stream_ptr(ts[0].device))


def copy_blocks(kv_caches, pairs: Sequence[Tuple[int, int]], table: Optional[torch.Tensor] = None) -> None:
    """Block ``dst`` becomes a copy of block ``src`` in every K and V cache, for every pair; eager, on
    the current stream, without a host wait."""
    native.check(try_copy_blocks(kv_caches, pairs, table), "pk_kv_copy_blocks")
