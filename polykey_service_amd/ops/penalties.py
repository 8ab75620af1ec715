"""Sampling penalties and logit bias (HIP kernels on GPU, reference on CPU).

State lives on the device so a pipelined decode step can use and update it without the host
(csrc/kernels/penalties.hip): one *slot* per penalised sequence holding a row of 16-bit words
(bit 15 = token is in the prompt, bits 0..14 = occurrences among the generated tokens), a
``logit_bias`` list of up to ``MAX_BIAS`` (id, value) pairs, and an fp32 output row.

Per step: :func:`apply` writes the penalised copy of every row that has a slot (the raw logits
are never written, logprobs keep describing them), ``sampler.sample(..., alt=state.out,
alt_slots=slots)`` samples those rows from the copy, :func:`update` counts the sampled ids.
:func:`seed` fills a slot from a sequence's prompt and generated ids.  Rows of one call have
distinct slots; slot -1 means "no penalties" and costs one early-returning workgroup.
"""
from __future__ import annotations

import torch

from . import native, reference

MAX_BIAS = reference.PENALTY_MAX_BIAS
ENTRY_WORDS = reference.PENALTY_ENTRY_WORDS
COUNT_MAX = 0x7FFF


class PenaltyState:
    """The device tables of ``n_slots`` slots over a vocabulary of ``vocab`` tokens."""

    def __init__(self, n_slots: int, vocab: int, device):
        self.n_slots, self.vocab = n_slots, vocab
        self.stride = (vocab + 7) // 8 * 8
        self.counts = torch.zeros((n_slots, self.stride), dtype=torch.int16, device=device)
        self.bias_ids = torch.zeros((n_slots, MAX_BIAS), dtype=torch.int32, device=device)
        self.bias_vals = torch.zeros((n_slots, MAX_BIAS), dtype=torch.float32, device=device)
        self.bias_n = torch.zeros(n_slots, dtype=torch.int32, device=device)
        self.out = torch.zeros((n_slots, self.stride), dtype=torch.float32, device=device)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.counts, self.bias_ids, self.bias_vals, self.bias_n,
                                                          self.out))


def seed(state: PenaltyState, entries: torch.Tensor, n_entries: int, ids: torch.Tensor, n_ids: int) -> None:
    """``entries`` int32 ``[>= n_entries * 6]``: (slot, start, n_prompt, n_out, n_bias, clear) per
    entry, indexing the int32 stream ``ids[:n_ids]`` (prompt ids, generated ids, bias ids, bias
    fp32 bit patterns).  ``clear`` wipes the slot first, otherwise the entry appends.  Entries of
    one call name distinct slots."""
    if n_entries <= 0:
        return
    assert entries.dtype == torch.int32 and ids.dtype == torch.int32
    assert entries.is_contiguous() and ids.is_contiguous()
    assert entries.numel() >= n_entries * ENTRY_WORDS and ids.numel() >= n_ids
    if not state.counts.is_cuda:
        reference.penalty_seed(state.counts, state.bias_ids, state.bias_vals, state.bias_n,
                               entries.reshape(-1)[:n_entries * ENTRY_WORDS].numpy(), ids.reshape(-1)[:n_ids].numpy(),
                               state.vocab)
        return
    native.call("pk_penalty_seed", state.counts.data_ptr(), state.stride, state.bias_ids.data_ptr(),
                state.bias_vals.data_ptr(), state.bias_n.data_ptr(), entries.data_ptr(), n_entries, ids.data_ptr(),
                n_ids, state.n_slots, state.vocab, native.stream_ptr())


def apply(state: PenaltyState, logits: torch.Tensor, slots: torch.Tensor, rep: torch.Tensor, freq: torch.Tensor,
          pres: torch.Tensor) -> torch.Tensor:
    """logits ``[B, V]`` (bf16 or fp32, never written), ``slots`` int32 ``[B]``, ``rep`` / ``freq``
    / ``pres`` fp32 ``[B]`` → ``state.out`` with row ``slots[b]`` = the penalised fp32 row of every
    ``b`` whose slot is in range; other rows of ``state.out`` are untouched."""
    B, V = logits.shape
    assert V <= state.stride and B <= slots.numel()
    if not logits.is_cuda:
        if bool((slots[:B] < 0).all()):
            return state.out
        return reference.penalty_apply(logits, state.counts, slots, rep, freq, pres, state.bias_ids, state.bias_vals,
                                       state.bias_n, state.out)
    assert logits.stride(-1) == 1 and logits.dtype in (torch.bfloat16, torch.float32)
    assert slots.dtype == torch.int32 and all(t.dtype == torch.float32 for t in (rep, freq, pres))
    assert all(t.is_contiguous() and t.numel() >= B for t in (slots, rep, freq, pres))
    native.call("pk_penalty_apply", state.out.data_ptr(), state.stride, logits.data_ptr(), logits.stride(0),
                0 if logits.dtype == torch.bfloat16 else 1, B, V, state.counts.data_ptr(), state.stride,
                slots.data_ptr(), rep.data_ptr(), freq.data_ptr(), pres.data_ptr(), state.bias_ids.data_ptr(),
                state.bias_vals.data_ptr(), state.bias_n.data_ptr(), state.n_slots, native.stream_ptr())
    return state.out


def update(state: PenaltyState, slots: torch.Tensor, tokens: torch.Tensor, n: int) -> None:
    """Count the sampled ``tokens[:n]`` (int32) in the rows ``slots[:n]`` (saturating; -1 = skip)."""
    if n <= 0:
        return
    if not state.counts.is_cuda:
        if bool((slots[:n] < 0).all()):
            return
        reference.penalty_update(state.counts, slots[:n], tokens[:n], state.vocab)
        return
    assert slots.dtype == torch.int32 and tokens.dtype == torch.int32
    assert slots.is_contiguous() and tokens.is_contiguous() and slots.numel() >= n and tokens.numel() >= n
    native.call("pk_penalty_update", state.counts.data_ptr(), state.stride, slots.data_ptr(), tokens.data_ptr(), n,
                state.n_slots, state.vocab, native.stream_ptr())


def read_slot(state: PenaltyState, slot: int):
    """Read-back of one slot for tests: (set of prompt-flagged ids, {id: count > 0})."""
    w = state.counts[slot, :state.vocab].cpu().numpy().view("uint16")
    flags = set(int(i) for i in (w & 0x8000).nonzero()[0])
    cnt = w & COUNT_MAX
    return flags, {int(i): int(cnt[i]) for i in cnt.nonzero()[0]}
