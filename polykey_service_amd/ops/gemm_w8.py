"""Weight-only FP8 projections: ``y = (x @ widen(byte)^T) * scale`` with OCP e4m3 weight bytes and
one fp32 scale per output channel (row of the ``[N, K]`` weight).

Activations, accumulation and outputs are those of the bf16 projections (:mod:`.gemm`); only the
weight stream changes.  Up to :data:`KERNEL_MAX_M` rows the hand-written decode GEMM
(``csrc/kernels/gemm_w8.hip``: the W8 instantiations of the bf16 kernels' tile body,
``skinny_tile.h``) streams the block-packed bytes (:func:`pack_w8`) and widens them to
bf16 in registers; above it the *wide path* widens the projection into a bf16 scratch,
runs the library GEMM on it and scales the output columns.  The ops mirror their bf16 namesakes
and share their tiling rules, so the fp32 slabs feed the same reducers.  CPU tensors take the fp32
reference (:func:`..reference.w8_linear`).
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import torch

from . import gemm, native, reference
from .gemm import (DECODE_MAX_M, FUSED_MAX_M, HALF_BIT, NT_BIT, Partial, RowScale, choose_split, down_kr, gate_up_split,
                   partial_tiling)

# rows the kernel serves; above it the wide path (widen -> library GEMM -> column scale).
# tools/bench_gemm_w8.py measures the crossover (profiles/w8_gemm.md)
KERNEL_MAX_M = DECODE_MAX_M


def pack_w8(b: torch.Tensor) -> torch.Tensor:
    """Row-major bytes ``[N, K]`` (uint8 or e4m3) -> the block-packed layout of the W8 decode GEMM
    (same size, uint8).  For every 128-row n-block (one workgroup) and 128-deep k-step the 16 KiB
    the workgroup consumes are contiguous: 8 row tiles x 2 loads of 1 KiB in lane order; lane
    l = 16 g + r of load jj holds row r and 16 bytes, k = 32 (2 jj + half) + 8 g + e for
    half = 0, 1 and e = 0..7 -- two MFMA fragments per 16-byte load."""
    N, K = b.shape
    assert N % 128 == 0 and K % 256 == 0, f"W8 weights need N % 128 == 0 and K % 256 == 0 (got {N} x {K})"
    b = b.view(torch.uint8)
    # [nb, tile, r, ks, jj, half, g, e] -> [nb, ks, tile, jj, g, r, half, e]
    return b.view(N // 128, 8, 16, K // 128, 2, 2, 4, 8).permute(0, 3, 1, 4, 6, 2, 5, 7).contiguous().view(N, K)


def unpack_w8(p: torch.Tensor) -> torch.Tensor:
    N, K = p.shape
    return p.view(N // 128, K // 128, 8, 2, 4, 16, 2, 8).permute(0, 2, 5, 1, 3, 6, 4, 7).contiguous().view(N, K)


@dataclasses.dataclass
class W8:
    """A quantised projection: block-packed e4m3 bytes ``[N, K]`` (uint8), fp32 scales ``[N]``.
    ``scratch``: a flat bf16 buffer of at least N * K elements the wide path widens into (owned
    by the model, shared by its projections); None: the wide path allocates one per call."""
    packed: torch.Tensor
    scale: torch.Tensor
    shape: Tuple[int, int]
    scratch: Optional[torch.Tensor] = None

    @classmethod
    def from_weight(cls, w: torch.Tensor) -> "W8":
        """Quantise a row-major ``[N, K]`` weight (per-row scale, :func:`..reference.quantize_fp8_rows`)."""
        b, scale = reference.quantize_fp8_rows(w)
        return cls.from_bytes(b, scale)

    @classmethod
    def from_bytes(cls, b: torch.Tensor, scale: torch.Tensor) -> "W8":
        return cls(pack_w8(b), scale.float().contiguous(), (b.shape[0], b.shape[1]))

    def bytes_rowmajor(self) -> torch.Tensor:
        """Row-major e4m3 ``[N, K]``."""
        return unpack_w8(self.packed).view(reference.FP8)

    def dequant(self) -> torch.Tensor:
        """fp32 ``scale * widen(byte)``, row-major."""
        return self.bytes_rowmajor().float() * self.scale[:, None]

    @property
    def nbytes(self) -> int:
        return self.packed.numel() + 4 * self.scale.numel()

    @property
    def device(self) -> torch.device:
        return self.packed.device


# ---------------------------------------------------------------------------------- wide path
def widen(w: W8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major bf16 ``[N, K]`` of the bytes (exact, no scale); ``out``: a flat bf16 buffer."""
    N, K = w.shape
    if not w.packed.is_cuda:
        r = w.bytes_rowmajor().to(torch.bfloat16)
        return r if out is None else out[: N * K].view(N, K).copy_(r)
    if out is None:
        out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    assert out.numel() >= N * K and out.dtype == torch.bfloat16 and out.is_contiguous()
    native.call("pk_w8_widen", out.data_ptr(), w.packed.data_ptr(), N, K, native.stream_ptr())
    return out[: N * K].view(N, K)


def col_scale(out: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """In place: ``out[m, n] = bf16(float(out[m, n]) * scale[n])``."""
    M, N = out.shape
    if not out.is_cuda:
        return out.copy_((out.float() * scale.float()[None, :]).to(out.dtype))
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1 and scale.dtype == torch.float32
    assert out.data_ptr() % 16 == 0 and scale.numel() == N, "unaligned output"
    native.call("pk_col_scale", out.data_ptr(), scale.data_ptr(), M, N, out.stride(0), native.stream_ptr())
    return out


def linear_wide(x: torch.Tensor, w: W8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The prefill path: widen into the handle's scratch (a buffer of this call's own when it has
    none), library GEMM, column scale (two bf16 roundings: the GEMM's output, then the scaled
    value)."""
    N, K = w.shape
    wb = widen(w, w.scratch if w.scratch is not None and w.scratch.numel() >= N * K else None)
    if out is None:
        out = torch.empty((x.shape[0], N), dtype=x.dtype, device=x.device)
    torch.mm(x, wb.t(), out=out)
    return col_scale(out, w.scale)


# ------------------------------------------------------------------------------------ kernel
def kernel_ok(x: torch.Tensor, max_m: int = KERNEL_MAX_M) -> bool:
    """Activations the W8 decode GEMM takes (else: the wide path)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and 0 < x.shape[0] <= max_m and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)


def _nt(w: W8) -> int:
    """Non-temporal weight loads by the byte threshold of the bf16 kernel (gemm.NT_MIN_BYTES)."""
    return NT_BIT if w.packed.numel() >= gemm.NT_MIN_BYTES else 0


def _launch(mode: int, x: torch.Tensor, w: W8, S: int, out: Optional[torch.Tensor] = None,
            ws: Optional[torch.Tensor] = None, rowscale: Optional[RowScale] = None) -> None:
    M, K = x.shape
    N = w.shape[0]
    assert K == w.shape[1], f"x has {K} columns, the weight {w.shape[1]}"
    assert kernel_ok(x), "activations the W8 kernel does not take (see kernel_ok)"
    assert out is None or (out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.stride(0) % 4 == 0
                           and out.data_ptr() % 8 == 0 and out.shape[0] >= M), "unaligned output"
    assert ws is None or (ws.dtype == torch.float32 and ws.data_ptr() % 16 == 0), "unaligned workspace"
    native.call("pk_w8_gemm", native.ptr(out) or 0, native.ptr(ws) or 0, x.data_ptr(), w.packed.data_ptr(),
                w.scale.data_ptr(), M, N, K, x.stride(0), out.stride(0) if out is not None else N, S, mode,
                rowscale.parts.data_ptr() if rowscale is not None else 0,
                rowscale.parts.shape[0] if rowscale is not None else 0,
                float(rowscale.eps) if rowscale is not None else 0.0, native.stream_ptr())


def _ref(x: torch.Tensor, w: W8, rowscale: Optional[RowScale] = None) -> torch.Tensor:
    """fp32 reference value of the projection (CPU tensors)."""
    rinv = None
    if rowscale is not None:
        rinv = torch.rsqrt(rowscale.parts.float().sum(0) / x.shape[1] + rowscale.eps)
    return reference.w8_linear(x, w.bytes_rowmajor(), w.scale, rinv)


def linear(x: torch.Tensor, w: W8, out: Optional[torch.Tensor] = None, max_m: int = KERNEL_MAX_M) -> torch.Tensor:
    """bf16 out [M, N]: the kernel up to ``max_m`` rows, the wide path above."""
    M, N = x.shape[0], w.shape[0]
    if not x.is_cuda:
        y = _ref(x, w).to(x.dtype)
        return y if out is None else out.copy_(y)
    if not kernel_ok(x, max_m):
        return linear_wide(x, w, out)
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _launch(gemm.MODE_BF16 | _nt(w), x, w, 1, out=out)
    return out


def linear_partial(x: torch.Tensor, w: W8, ws: torch.Tensor, S: Optional[int] = None, half: bool = False) -> Partial:
    """Split-K fp32 slabs into ``ws`` (>= S*M*N), tiled as :func:`gemm.linear_partial`."""
    M, K = x.shape
    N = w.shape[0]
    S_auto, half = partial_tiling(N, K, M, w.packed, half)
    S = S_auto if S is None else S
    assert ws.numel() >= S * M * N, "split-K workspace too small"
    if not x.is_cuda:
        ws[: M * N].view(M, N).copy_(_ref(x, w))
        return Partial(ws, 1, M, N)
    _launch(gemm.MODE_PARTIAL | (HALF_BIT if half else 0), x, w, S, ws=ws)
    return Partial(ws, S, M, N)


def linear_partial_rowscale(x: torch.Tensor, w: W8, ws: torch.Tensor, rowscale: RowScale, S: Optional[int] = None,
                            half: bool = False) -> Partial:
    """:func:`linear_partial` of a folded-norm projection: slabs of rinv[m] * scale[n] * acc."""
    M, K = x.shape
    N = w.shape[0]
    S_auto, half = partial_tiling(N, K, M, w.packed, half)
    S = S_auto if S is None else S
    assert ws.numel() >= S * M * N, "split-K workspace too small"
    if not x.is_cuda:
        ws[: M * N].view(M, N).copy_(_ref(x, w, rowscale))
        return Partial(ws, 1, M, N)
    _launch(gemm.MODE_PARTIAL | (HALF_BIT if half else 0), x, w, S, ws=ws, rowscale=rowscale)
    return Partial(ws, S, M, N)


def linear_silu(x: torch.Tensor, w: W8, ws: Optional[torch.Tensor] = None, rowscale: Optional[RowScale] = None,
                max_m: int = KERNEL_MAX_M) -> torch.Tensor:
    """silu(gate) * up of an interleaved gate/up projection -> [M, N / 2], split as
    :func:`gemm.linear_silu` splits it (``rowscale``: the folded norm)."""
    M, K = x.shape
    N = w.shape[0]
    if not x.is_cuda:
        return reference.silu_and_mul_interleaved(_ref(x, w, rowscale).to(x.dtype))
    if not kernel_ok(x, max_m):
        assert rowscale is None, "the folded-norm gate_up runs on the kernel only"
        return gemm.silu_and_mul_interleaved(linear_wide(x, w))
    out = torch.empty((M, N // 2), dtype=x.dtype, device=x.device)
    if rowscale is not None:
        S = gate_up_split(N, K, M) if M <= FUSED_MAX_M else 1
    else:
        S = choose_split(N, K, M)
    if S > 1 and ws is not None and ws.numel() >= S * M * N:
        p = (linear_partial_rowscale(x, w, ws, rowscale, S=S) if rowscale is not None
             else linear_partial(x, w, ws, S))
        return gemm.silu_reduce(p, out)
    _launch(gemm.MODE_SILU | _nt(w), x, w, 1, out=out, rowscale=rowscale)
    return out


def linear_down(h: torch.Tensor, w: W8, ws: torch.Tensor) -> Partial:
    """The decode down projection, tiled as :func:`gemm.linear_down` -> fp32 slabs."""
    M, K = h.shape
    N = w.shape[0]
    S = choose_split(N, K, M)
    if h.is_cuda and down_kr(N, K, M) == 1 and M <= FUSED_MAX_M:
        assert ws.numel() >= S * M * N, "split-K workspace too small"
        _launch(gemm.MODE_PARTIAL | HALF_BIT, h, w, S, ws=ws)
        return Partial(ws, S, M, N)
    return linear_partial(h, w, ws, S)
