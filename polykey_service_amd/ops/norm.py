"""RMSNorm / fused residual-add RMSNorm / SiLU-and-mul (HIP on GPU, fp32 reference on CPU)."""
from __future__ import annotations

from typing import Optional

import torch

from . import native, reference


def check_rows(t: torch.Tensor, what: str) -> None:
    """The row kernels move 16-byte (8 x bf16) vectors: a 2-D view must have unit column stride, a
    16-byte aligned base and, with more than one row, a row stride that is a multiple of 8."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what}: a 2-D view with unit column stride is required, got strides {tuple(t.stride())}")
    if t.data_ptr() % 16:
        raise ValueError(f"{what}: the base is not 16-byte aligned (offset {t.data_ptr() % 16})")
    if t.shape[0] > 1 and t.stride(0) % 8:
        raise ValueError(f"{what}: the row stride {t.stride(0)} is not a multiple of 8 elements")


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x * rsqrt(mean(x^2) + eps) * w over the last dim of a 2-D [T, H] view.  ``x`` and ``out``
    may be column slices of wider tensors (see :func:`check_rows`)."""
    if not x.is_cuda:
        y = reference.rms_norm(x, weight, eps)
        return y if out is None else out.copy_(y.view(out.shape)).view(x.shape)
    H = x.shape[-1]
    x2 = x.reshape(-1, H)
    assert weight.is_contiguous() and weight.numel() == H and x.dtype == torch.bfloat16 == weight.dtype
    T = x2.shape[0]
    if out is None:
        out = torch.empty((T, H), dtype=x.dtype, device=x.device)
    assert out.shape == (T, H) and out.dtype == x.dtype
    check_rows(x2, "rms_norm input")
    check_rows(out, "rms_norm out")
    native.call("pk_rmsnorm", out.data_ptr(), x2.data_ptr(), weight.data_ptr(), T, H, x2.stride(0),
                out.stride(0), float(eps), native.stream_ptr())
    return out.view(x.shape)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float):
    """In place: residual += x; x = rms_norm(residual) * w.  Returns (x, residual)."""
    if not x.is_cuda:
        return reference.fused_add_rms_norm(x, residual, weight, eps)
    assert x.is_contiguous() and residual.is_contiguous() and x.shape == residual.shape
    H = x.shape[-1]
    T = x.numel() // H
    native.call("pk_fused_add_rmsnorm", x.data_ptr(), residual.data_ptr(), weight.data_ptr(), T, H, float(eps),
                native.stream_ptr())
    return x, residual


def silu_and_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: [T, 2I] = gate | up → silu(gate) * up: [T, I]; ``out``: a contiguous destination (e.g. a
    row slice of a larger buffer) written in place."""
    if not x.is_cuda:
        y = reference.silu_and_mul(x)
        return y if out is None else out.copy_(y.view(out.shape))
    assert x.is_contiguous() and x.dtype == torch.bfloat16
    I2 = x.shape[-1]
    T = x.numel() // I2
    if out is None:
        out = torch.empty(x.shape[:-1] + (I2 // 2,), dtype=x.dtype, device=x.device)
    assert out.is_contiguous() and out.numel() == T * (I2 // 2) and out.dtype == x.dtype
    native.call("pk_silu_and_mul", out.data_ptr(), x.data_ptr(), T, I2 // 2, native.stream_ptr())
    return out
