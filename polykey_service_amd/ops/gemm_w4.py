"""Weight-only MXFP4 projections: ``y = x @ w^T`` with ``w[n, k] = E2M1[nib[n, k]] * 2^(X[n, k // 32] - 127)``
(OCP Microscaling FP4: e2m1 elements, one e8m0 scale byte per block of 32 along K; 4.25 bits per
weight, no per-channel scale).

Activations, accumulation and outputs are those of the bf16 projections (:mod:`.gemm`); only the
weight stream changes.  For scale bytes in [2, 252] -- which the handle enforces and the quantiser
produces -- every weight is a normal bf16 number or zero, so the kernel feeds the MFMA the exact
weight: numerically a W4 projection is the bf16 projection of :meth:`W4.dequant`.  Up to
:data:`KERNEL_MAX_M` rows the hand-written decode GEMM (``csrc/kernels/gemm_w4.hip``: the W4
instantiations of the bf16 kernels' tile body, ``skinny_tile.h``) streams the block-packed nibbles
and scale words (:func:`pack_w4`) and widens them to bf16 in registers; above it the *wide path*
widens the projection (block scales applied, exact) into a bf16 scratch and runs the library GEMM on
it -- one bf16 rounding.  The ops mirror their bf16 namesakes and share their tiling rules, so the
fp32 slabs feed the same reducers.  CPU tensors take the fp32 reference
(:func:`..reference.w4_linear`).
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import torch

from . import gemm, native, reference
from .gemm import (DECODE_MAX_M, FUSED_MAX_M, HALF_BIT, NT_BIT, Partial, RowScale, choose_split, down_kr, gate_up_split,
                   partial_tiling)

# rows the kernel serves; above it the wide path (widen -> library GEMM).
# tools/bench_gemm_w4.py measures the crossover (profiles/w4_gemm.md)
KERNEL_MAX_M = DECODE_MAX_M
SCALE_MIN, SCALE_MAX = reference.MX_SCALE_MIN, reference.MX_SCALE_MAX


def pack_w4(nib: torch.Tensor, xs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-major nibbles ``[N, K / 2]`` (low nibble = even k) and scale bytes ``[N, K / 32]`` -> the
    block-packed layout of the W4 decode GEMM: (nibbles ``[N, K / 2]``, scales ``[N, K / 32]``, uint8).

    Nibbles: for every 128-row n-block (one workgroup) and 128-deep k-step the 8 KiB the workgroup
    consumes are contiguous: 8 row tiles x one load of 1 KiB in lane order; lane l = 16 g + r holds
    row r and 16 bytes, its 32-bit word s (0..3) the eight elements k = 32 s + 8 g + e, e = 0..7
    (byte b of the word: e = 2 b in the low nibble, 2 b + 1 in the high one) -- word s is the MFMA
    fragment of k-block s, which is one MX block of that row.
    Scales: ``[N / 128, K / 128, 8 tiles, 16 rows]`` words of 4 bytes, byte s = the scale of k-block
    s of the row; the 4 lanes that share a row read the same word."""
    N, K2 = nib.shape
    K = 2 * K2
    assert N % 128 == 0 and K % 256 == 0, f"W4 weights need N % 128 == 0 and K % 256 == 0 (got {N} x {K})"
    assert xs.shape == (N, K // 32), f"scales of {tuple(xs.shape)} for a {N} x {K} weight"
    # [nb, tile, r, ks, s, g, b] -> [nb, ks, tile, g, r, s, b]
    p = nib.view(N // 128, 8, 16, K // 128, 4, 4, 4).permute(0, 3, 1, 5, 2, 4, 6).contiguous().view(N, K2)
    # [nb, tile, r, ks, s] -> [nb, ks, tile, r, s]
    x = xs.view(N // 128, 8, 16, K // 128, 4).permute(0, 3, 1, 2, 4).contiguous().view(N, K // 32)
    return p, x


def unpack_w4(p: torch.Tensor, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    N, K2 = p.shape
    K = 2 * K2
    nib = p.view(N // 128, K // 128, 8, 4, 16, 4, 4).permute(0, 2, 4, 1, 5, 3, 6).contiguous().view(N, K2)
    xs = x.view(N // 128, K // 128, 8, 16, 4).permute(0, 2, 3, 1, 4).contiguous().view(N, K // 32)
    return nib, xs


@dataclasses.dataclass
class W4:
    """A quantised projection: block-packed nibbles ``[N, K / 2]`` and scale bytes ``[N, K / 32]``
    (uint8, :func:`pack_w4`).  ``scratch``: a flat bf16 buffer of at least N * K elements the wide
    path widens into (owned by the model, shared by its projections); None: the wide path allocates
    one per call."""
    packed: torch.Tensor
    scales: torch.Tensor
    shape: Tuple[int, int]
    scratch: Optional[torch.Tensor] = None

    @classmethod
    def from_weight(cls, w: torch.Tensor) -> "W4":
        """Quantise a row-major ``[N, K]`` weight (:func:`..reference.quantize_mxfp4_rows`)."""
        return cls.from_bytes(*reference.quantize_mxfp4_rows(w))

    @classmethod
    def from_bytes(cls, nib: torch.Tensor, xs: torch.Tensor) -> "W4":
        """From the interchange layout: nibbles ``uint8 [N, K / 2]`` (low nibble = even k), scales
        ``uint8 [N, K / 32]``.  Scale bytes outside [2, 252] (255 is NaN in e8m0; beyond the range a
        weight is no normal bf16 number, and the kernel's widening would not be exact) are refused."""
        if nib.dtype != torch.uint8 or xs.dtype != torch.uint8:
            raise ValueError("MXFP4 nibbles and scales are uint8 tensors")
        if xs.numel() and (int(xs.min()) < SCALE_MIN or int(xs.max()) > SCALE_MAX):
            raise ValueError(f"MXFP4 scale bytes must lie in [{SCALE_MIN}, {SCALE_MAX}] "
                             f"(got {int(xs.min())}..{int(xs.max())})")
        p, x = pack_w4(nib, xs)
        return cls(p, x, (nib.shape[0], 2 * nib.shape[1]))

    def bytes_rowmajor(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The interchange layout: (nibbles ``[N, K / 2]``, scales ``[N, K / 32]``), row-major uint8."""
        return unpack_w4(self.packed, self.scales)

    def dequant(self) -> torch.Tensor:
        """fp32 ``E2M1[nibble] * 2^(X - 127)``, row-major ``[N, K]`` (exact)."""
        return reference.dequantize_mxfp4(*self.bytes_rowmajor())

    @property
    def nbytes(self) -> int:
        return self.packed.numel() + self.scales.numel()

    @property
    def device(self) -> torch.device:
        return self.packed.device


# ---------------------------------------------------------------------------------- wide path
def widen(w: W4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major bf16 ``[N, K]`` of the weight, block scales applied (exact); ``out``: a flat bf16
    buffer."""
    N, K = w.shape
    if not w.packed.is_cuda:
        r = w.dequant().to(torch.bfloat16)
        return r if out is None else out[: N * K].view(N, K).copy_(r)
    if out is None:
        out = torch.empty(N * K, dtype=torch.bfloat16, device=w.device)
    assert out.numel() >= N * K and out.dtype == torch.bfloat16 and out.is_contiguous()
    native.call("pk_w4_widen", out.data_ptr(), w.packed.data_ptr(), w.scales.data_ptr(), N, K, native.stream_ptr())
    return out[: N * K].view(N, K)


def linear_wide(x: torch.Tensor, w: W4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The prefill path: widen into the handle's scratch (a buffer of this call's own when it has
    none), library GEMM (one bf16 rounding: the GEMM's output)."""
    N, K = w.shape
    wb = widen(w, w.scratch if w.scratch is not None and w.scratch.numel() >= N * K else None)
    if out is None:
        out = torch.empty((x.shape[0], N), dtype=x.dtype, device=x.device)
    return torch.mm(x, wb.t(), out=out)


# ------------------------------------------------------------------------------------ kernel
def kernel_ok(x: torch.Tensor, max_m: int = KERNEL_MAX_M) -> bool:
    """Activations the W4 decode GEMM takes (else: the wide path)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and 0 < x.shape[0] <= max_m and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)


def _nt(w: W4) -> int:
    """Non-temporal weight loads by the byte threshold of the bf16 kernel (gemm.NT_MIN_BYTES) on
    the packed nibble bytes."""
    return NT_BIT if w.packed.numel() >= gemm.NT_MIN_BYTES else 0


def _launch(mode: int, x: torch.Tensor, w: W4, S: int, out: Optional[torch.Tensor] = None,
            ws: Optional[torch.Tensor] = None, rowscale: Optional[RowScale] = None) -> None:
    M, K = x.shape
    N = w.shape[0]
    assert K == w.shape[1], f"x has {K} columns, the weight {w.shape[1]}"
    assert kernel_ok(x), "activations the W4 kernel does not take (see kernel_ok)"
    assert out is None or (out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.stride(0) % 4 == 0
                           and out.data_ptr() % 8 == 0 and out.shape[0] >= M), "unaligned output"
    assert ws is None or (ws.dtype == torch.float32 and ws.data_ptr() % 16 == 0), "unaligned workspace"
    assert w.packed.data_ptr() % 16 == 0 and w.scales.data_ptr() % 4 == 0, "unaligned weight"
    native.call("pk_w4_gemm", native.ptr(out) or 0, native.ptr(ws) or 0, x.data_ptr(), w.packed.data_ptr(),
                w.scales.data_ptr(), M, N, K, x.stride(0), out.stride(0) if out is not None else N, S, mode,
                rowscale.parts.data_ptr() if rowscale is not None else 0,
                rowscale.parts.shape[0] if rowscale is not None else 0,
                float(rowscale.eps) if rowscale is not None else 0.0, native.stream_ptr())


def _ref(x: torch.Tensor, w: W4, rowscale: Optional[RowScale] = None) -> torch.Tensor:
    """fp32 reference value of the projection (CPU tensors)."""
    rinv = None
    if rowscale is not None:
        rinv = torch.rsqrt(rowscale.parts.float().sum(0) / x.shape[1] + rowscale.eps)
    return reference.w4_linear(x, *w.bytes_rowmajor(), rinv)


def linear(x: torch.Tensor, w: W4, out: Optional[torch.Tensor] = None, max_m: int = KERNEL_MAX_M) -> torch.Tensor:
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


def linear_partial(x: torch.Tensor, w: W4, ws: torch.Tensor, S: Optional[int] = None, half: bool = False) -> Partial:
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


def linear_partial_rowscale(x: torch.Tensor, w: W4, ws: torch.Tensor, rowscale: RowScale, S: Optional[int] = None,
                            half: bool = False) -> Partial:
    """:func:`linear_partial` of a folded-norm projection: slabs of rinv[m] * acc."""
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


def linear_silu(x: torch.Tensor, w: W4, ws: Optional[torch.Tensor] = None, rowscale: Optional[RowScale] = None,
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


def linear_down(h: torch.Tensor, w: W4, ws: torch.Tensor) -> Partial:
    """The decode down projection, tiled as :func:`gemm.linear_down` -> fp32 slabs."""
    M, K = h.shape
    N = w.shape[0]
    S = choose_split(N, K, M)
    if h.is_cuda and down_kr(N, K, M) == 1 and M <= FUSED_MAX_M:
        assert ws.numel() >= S * M * N, "split-K workspace too small"
        _launch(gemm.MODE_PARTIAL | HALF_BIT, h, w, S, ws=ws)
        return Partial(ws, S, M, N)
    return linear_partial(h, w, ws, S)
