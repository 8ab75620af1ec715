"""Token sampling (HIP kernel on GPU, reference on CPU).

Per-row parameters are device tensors so a decode step (logits → tokens) can be captured in
a HIP graph: ``temperature`` f32 (0 → greedy), ``top_k`` i32 (0 → off), ``top_p`` f32
(1 → off), ``min_p`` f32 (0 → off), ``seeds`` i32 and ``offsets`` i32 (the per-request
token index, so a seeded request reproduces regardless of how it was batched).

:func:`logprobs` reports the log-probabilities of what was sampled, from the *raw* logits
(before temperature / top-k / top-p / min-p): per row one packed record of ``LOGPROB_WORDS``
32-bit words, ``[logprob | 20 top ids | 20 top logprobs]`` (see :func:`unpack_logprobs`).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import native, reference


def sample(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
           min_p: torch.Tensor, seeds: torch.Tensor, offsets: torch.Tensor,
           out: Optional[torch.Tensor] = None, alt: Optional[torch.Tensor] = None,
           alt_slots: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [B, V] (bf16 or fp32) → int32 token ids [B].

    ``alt`` fp32 ``[n, >= V]`` with ``alt_slots`` int32 ``[B]``: a row whose ``alt_slots[b]`` is in
    ``[0, n)`` is sampled from ``alt[alt_slots[b], :V]`` (its penalised copy, ops/penalties.py)
    instead of ``logits[b]``; every other row is sampled exactly as without them."""
    B, V = logits.shape
    assert (alt is None) == (alt_slots is None)
    if not logits.is_cuda:
        if alt is not None:
            rows = [b for b in range(B) if 0 <= int(alt_slots[b]) < alt.shape[0]]
            if rows:
                logits = logits.float().clone()
                logits[rows] = alt[alt_slots[rows].long(), :V]
        return reference.sample(logits, temperature, top_k, top_p, min_p, seeds, offsets).to(torch.int32)
    assert logits.stride(-1) == 1
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
    dtype = 0 if logits.dtype == torch.bfloat16 else 1
    assert logits.dtype in (torch.bfloat16, torch.float32)
    if alt is None:
        native.call("pk_sample", out.data_ptr(), logits.data_ptr(), temperature.data_ptr(), top_k.data_ptr(),
                    top_p.data_ptr(), min_p.data_ptr(), seeds.data_ptr(), offsets.data_ptr(), 0, B, V,
                    logits.stride(0), dtype, native.stream_ptr())
        return out
    assert alt.dtype == torch.float32 and alt.dim() == 2 and alt.stride(1) == 1 and alt.stride(0) >= V
    assert alt_slots.dtype == torch.int32 and alt_slots.is_contiguous() and alt_slots.numel() >= B
    native.call("pk_sample_alt", out.data_ptr(), logits.data_ptr(), temperature.data_ptr(), top_k.data_ptr(),
                top_p.data_ptr(), min_p.data_ptr(), seeds.data_ptr(), offsets.data_ptr(), B, V, logits.stride(0),
                dtype, alt.data_ptr(), alt.stride(0), alt_slots.data_ptr(), alt.shape[0], native.stream_ptr())
    return out


def greedy(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not logits.is_cuda:
        return torch.argmax(logits.float(), dim=-1).to(torch.int32)
    B, V = logits.shape
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
    dtype = 0 if logits.dtype == torch.bfloat16 else 1
    native.call("pk_sample", out.data_ptr(), logits.data_ptr(), 0, 0, 0, 0, 0, 0, 0, B, V, logits.stride(0), dtype,
                native.stream_ptr())
    return out


LOGPROB_NMAX = 20                       # longest top list (the kernel's compile-time constant)
LOGPROB_WORDS = 1 + 2 * LOGPROB_NMAX    # packed int32 words per row


def logprobs(logits: torch.Tensor, tokens: torch.Tensor, n_top: torch.Tensor,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [B, V] (bf16 or fp32), sampled ids int32 [B], ``n_top`` int32 [B] → packed int32
    ``[B, LOGPROB_WORDS]``.  ``n_top[b]``: -1 leaves row ``b`` of ``out`` untouched, 0 reports the
    sampled token's logprob only, 1..20 adds the top list in (value descending, id ascending)
    order; unused list slots hold id -1 / logprob -inf."""
    B, V = logits.shape
    if out is None:
        out = torch.zeros((B, LOGPROB_WORDS), dtype=torch.int32, device=logits.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.shape[0] >= B and out.shape[1] == LOGPROB_WORDS
    if not logits.is_cuda:
        return reference.logprobs(logits, tokens, n_top, out)
    assert logits.stride(-1) == 1 and logits.dtype in (torch.bfloat16, torch.float32)
    assert tokens.dtype == torch.int32 and n_top.dtype == torch.int32
    assert tokens.is_contiguous() and n_top.is_contiguous() and tokens.numel() >= B and n_top.numel() >= B
    dtype = 0 if logits.dtype == torch.bfloat16 else 1
    native.call("pk_logprobs", out.data_ptr(), logits.data_ptr(), tokens.data_ptr(), n_top.data_ptr(), B, V,
                logits.stride(0), dtype, native.stream_ptr())
    return out


PROMPT_LOGPROB_WORDS = 2 + 2 * LOGPROB_NMAX  # [logprob | rank | 20 ids | 20 logprobs]


def prompt_logprobs(logits: torch.Tensor, targets: torch.Tensor, n_top: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [R, V] (bf16 or fp32), target ids int32 [R], ``n_top`` int32 [R] → packed int32
    ``[R, PROMPT_LOGPROB_WORDS]``: the log-probability of ``targets[r]`` under row ``r``, its 1-based
    rank in the total order (value descending, id ascending; 1 = the greedy token) and the top
    list as :func:`logprobs` writes it.  A row with ``targets[r] < 0`` or ``n_top[r] < 0`` is left
    untouched; ``targets[r] >= V`` reports logprob -inf and rank 0."""
    R, V = logits.shape
    if out is None:
        out = torch.zeros((R, PROMPT_LOGPROB_WORDS), dtype=torch.int32, device=logits.device)
    assert (out.dtype == torch.int32 and out.is_contiguous() and out.shape[0] >= R
            and out.shape[1] == PROMPT_LOGPROB_WORDS)
    if not logits.is_cuda:
        return reference.prompt_logprobs(logits, targets, n_top, out)
    assert logits.stride(-1) == 1 and logits.dtype in (torch.bfloat16, torch.float32)
    assert targets.dtype == torch.int32 and n_top.dtype == torch.int32
    assert targets.is_contiguous() and n_top.is_contiguous() and targets.numel() >= R and n_top.numel() >= R
    dtype = 0 if logits.dtype == torch.bfloat16 else 1
    native.call("pk_prompt_logprobs", out.data_ptr(), logits.data_ptr(), targets.data_ptr(), n_top.data_ptr(), R, V,
                logits.stride(0), dtype, native.stream_ptr())
    return out


def unpack_prompt_logprobs(packed: torch.Tensor):
    """Packed rows (on the host) → (logprob f32 [R], rank i32 [R], top ids i32 [R, 20], top logprobs
    f32 [R, 20])."""
    n = LOGPROB_NMAX
    return (packed[:, 0].view(torch.float32), packed[:, 1], packed[:, 2:2 + n],
            packed[:, 2 + n:].view(torch.float32))


def prompt_logprob_entry(row, n: int):
    """One packed row (numpy int32 [PROMPT_LOGPROB_WORDS]) → ``(logprob, rank, [(id, logprob) × n])``."""
    f = row.view("float32")
    k = LOGPROB_NMAX
    return float(f[0]), int(row[1]), [(int(row[2 + j]), float(f[2 + k + j])) for j in range(n) if row[2 + j] >= 0]


def unpack_logprobs(packed: torch.Tensor):
    """Packed rows (on the host) → (logprob f32 [B], top ids i32 [B, 20], top logprobs f32 [B, 20])."""
    n = LOGPROB_NMAX
    return packed[:, 0].view(torch.float32), packed[:, 1:1 + n], packed[:, 1 + n:].view(torch.float32)


def logprob_entry(row, n: int):
    """One packed row (numpy int32 [LOGPROB_WORDS]) → ``(logprob, [(id, logprob) × n])``."""
    f = row.view("float32")
    k = LOGPROB_NMAX
    return float(f[0]), [(int(row[1 + j]), float(f[1 + k + j])) for j in range(n) if row[1 + j] >= 0]
