"""Multi-LoRA shrink / expand (``csrc/kernels/lora.hip``): per-row adapters on a shared projection.

    t      = bf16(rinv * x @ A[slot]^T)                     :func:`shrink`
    out   += s[slot] * t[seg(n)] @ B[slot]^T                :func:`expand`  (fp32 slab or bf16 rows)

``slot`` is ``idx[row]`` (int32, one per token row; -1 = no adapter: the row is neither read nor
written).  The grids depend on shapes only, so both launches can sit in a captured graph whose
index buffer is rewritten between replays.  CPU tensors take the fp32 references
(:func:`..reference.lora_shrink` / :func:`..reference.lora_expand`).
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import native, reference
from .gemm import Partial, RowScale

MAX_SEG_RANK = 64  # ranks per sub-projection the expand kernel keeps in registers


@dataclasses.dataclass
class Segments:
    """Which rank block of ``t`` a column of a fused projection reads: ``il`` > 0 = gate / up rows
    interleaved by ``il``; else the q | k | v boundaries ``b0`` <= ``b1`` (both N: one block)."""
    b0: int
    b1: int
    il: int = 0

    @classmethod
    def single(cls, N: int) -> "Segments":
        return cls(N, N, 0)

    def count(self, N: int) -> int:
        return 2 if self.il > 0 else 1 + (self.b0 < N) + (self.b1 < N)


def shrink(x: torch.Tensor, A: torch.Tensor, idx: torch.Tensor, t: torch.Tensor, seg_r: int,
           ranks: Optional[torch.Tensor] = None, rowscale: Optional[RowScale] = None) -> torch.Tensor:
    """``t[:M * R]`` viewed [M, R] <- bf16(rinv * x @ A[idx]^T); ``A`` [slots, R, K] bf16 with
    R = segments * ``seg_r``; ``x`` [M, K] bf16 with a row stride; ``t`` a flat bf16 scratch (never
    the split-K workspace).  ``ranks`` int32 [slots]: rank columns at or above it are zeros."""
    M, K = x.shape
    S, R, KA = A.shape
    assert KA == K and R % seg_r == 0 and t.numel() >= M * R and idx.numel() >= M
    assert idx.dtype == torch.int32 and A.is_contiguous() and x.stride(1) == 1
    tv = t.view(-1)[: M * R].view(M, R)
    if not x.is_cuda:
        return reference.lora_shrink(x, A, idx, None if rowscale is None else rowscale.parts,
                                     0.0 if rowscale is None else rowscale.eps, out=tv)
    assert x.dtype == torch.bfloat16 and A.dtype == torch.bfloat16 and t.dtype == torch.bfloat16
    parts = rowscale.parts if rowscale is not None else None
    if parts is not None:
        assert parts.dtype == torch.float32 and parts.is_contiguous() and parts.shape[1] == M
    native.call("pk_lora_shrink", tv.data_ptr(), x.data_ptr(), x.stride(0), A.data_ptr(), idx.data_ptr(),
                native.ptr(ranks), M, K, R, seg_r, S, native.ptr(parts), 0 if parts is None else parts.shape[0],
                0.0 if rowscale is None else float(rowscale.eps), native.stream_ptr())
    return tv


def expand(out: torch.Tensor, t: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, idx: torch.Tensor,
           seg: Segments, ranks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out`` [M, N] += scale[idx] * t @ B[idx]^T, in place: fp32 ``out`` is a split-K slab (the
    slab form), bf16 ``out`` becomes bf16(float(out) + delta) (the bf16 form; row stride allowed).
    ``B`` [slots, N, seg_r] bf16 in the fused / interleaved row order of the weight it accompanies."""
    M, N = out.shape
    S, NB, seg_r = B.shape
    R = t.shape[1]
    assert NB == N and t.shape[0] == M and R == seg.count(N) * seg_r and idx.numel() >= M and scale.numel() == S
    assert out.stride(1) == 1 and out.dtype in (torch.float32, torch.bfloat16)
    if not out.is_cuda:
        return reference.lora_expand(out, t, B, scale, idx, seg.b0, seg.b1, seg.il)
    assert seg_r <= MAX_SEG_RANK and t.is_contiguous() and B.is_contiguous() and scale.dtype == torch.float32
    native.call("pk_lora_expand", out.data_ptr(), out.stride(0), int(out.dtype == torch.float32), t.data_ptr(),
                B.data_ptr(), scale.data_ptr(), idx.data_ptr(), native.ptr(ranks), M, N, R, seg_r, seg.b0, seg.b1,
                seg.il, S, native.stream_ptr())
    return out


def slab0(p: Partial) -> torch.Tensor:
    """The first split-K slab of ``p`` as fp32 [M, N]: where the slab form adds its delta."""
    return p.buf[: p.M * p.N].view(p.M, p.N)
