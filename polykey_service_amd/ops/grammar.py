"""Guided decoding on the device (HIP kernels on GPU, reference on CPU).

A constrained sequence owns a byte DFA (engine/grammar.py) and a current state; both live on the
device so that a pipelined decode step can mask and advance without the host
(csrc/kernels/grammar.hip).  :class:`GrammarState` holds a pool of ``N_TABLES`` automata of up to
``MAX_STATES`` states, one record per *penalty slot* (table entry, state, up to 17 end ids) and the
byte string of every vocabulary id.

Per step, between ``penalties.apply`` and the sampler: :func:`mask` writes ``-inf`` into the fp32
copy ``out[slot]`` of every row whose slot holds a table, for each id the automaton does not admit;
after the sampler :func:`advance` moves the state along the sampled id's bytes.  :func:`load`
writes a table (or a chunk of one) into a pool entry, :func:`seed` writes slot records; both are
eager only.  The semantics are written once, in ops/reference.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import native, reference

MAX_STATES = reference.GRAMMAR_MAX_STATES
N_TABLES = reference.GRAMMAR_N_TABLES
MAX_END = reference.GRAMMAR_MAX_END
TABLE_WORDS = reference.GRAMMAR_TABLE_WORDS
SLOT_WORDS = reference.GRAMMAR_SLOT_WORDS
SEED_WORDS = reference.GRAMMAR_SEED_WORDS
pack = reference.grammar_pack


class GrammarState:
    """Device state for ``n_slots`` slots over the vocabulary described by ``off`` int32 ``[V + 1]``
    and ``data`` uint8 (engine/grammar.py token_bytes)."""

    def __init__(self, n_slots: int, off: np.ndarray, data: np.ndarray, device, n_tables: int = N_TABLES):
        off = np.ascontiguousarray(off, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self.vocab = off.size - 1
        self.n_bytes = int(data.size)
        # the kernels index `data` by these offsets: hold them to the table before they reach the device
        assert self.vocab >= 1 and off[0] == 0 and (np.diff(off) >= 0).all() and int(off[-1]) == self.n_bytes
        self.n_slots, self.n_tables = n_slots, n_tables
        self.off_np, self.data_np = off, data
        self.off = torch.from_numpy(off).to(device)
        self.data = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(device)
        self.pool = torch.zeros((n_tables, TABLE_WORDS), dtype=torch.int32, device=device)
        self.rec = torch.full((n_slots, SLOT_WORDS), -1, dtype=torch.int32, device=device)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.off, self.data, self.pool, self.rec))


def load(state: GrammarState, entry: int, word_off: int, words: torch.Tensor, n_words: int) -> None:
    """``pool[entry, word_off:word_off + n_words] = words[:n_words]`` (int32, on the state's device)."""
    if n_words <= 0:
        return
    assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() >= n_words
    assert 0 <= entry < state.n_tables and 0 <= word_off and word_off + n_words <= TABLE_WORDS
    if not state.pool.is_cuda:
        reference.grammar_load(state.pool, entry, word_off, words.reshape(-1)[:n_words].numpy())
        return
    native.call("pk_grammar_load", state.pool.data_ptr(), state.n_tables, entry, word_off, words.data_ptr(), n_words,
                native.stream_ptr())


def seed(state: GrammarState, entries: torch.Tensor, n_entries: int) -> None:
    """``entries`` int32 ``[>= n_entries * 21]``: (slot, table entry or -1, state, number of end ids,
    17 end ids) per entry.  Entries of one call name distinct slots."""
    if n_entries <= 0:
        return
    assert entries.dtype == torch.int32 and entries.is_contiguous() and entries.numel() >= n_entries * SEED_WORDS
    if not state.rec.is_cuda:
        reference.grammar_seed(state.rec, entries.reshape(-1)[:n_entries * SEED_WORDS].numpy())
        return
    native.call("pk_grammar_seed", state.rec.data_ptr(), state.n_slots, entries.data_ptr(), n_entries,
                native.stream_ptr())


def mask(state: GrammarState, out: torch.Tensor, slots: torch.Tensor, B: int, V: int) -> torch.Tensor:
    """In place on the fp32 rows ``out[slots[b]]``, ``b < B``: ``-inf`` into every id ``< V`` the
    slot's automaton does not admit from its current state; rows without a table are untouched."""
    assert V <= state.vocab and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1
    assert out.shape[0] >= state.n_slots and out.shape[1] >= V and B <= slots.numel()
    if B <= 0:
        return out
    if not out.is_cuda:
        if bool((slots[:B] < 0).all()):
            return out
        reference.grammar_mask(out, V, state.pool, state.rec, slots, B, state.off_np, state.data_np)
        return out
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    native.call("pk_grammar_mask", out.data_ptr(), out.stride(0), B, V, state.pool.data_ptr(), state.n_tables,
                state.rec.data_ptr(), state.n_slots, slots.data_ptr(), state.off.data_ptr(), state.data.data_ptr(),
                state.n_bytes, native.stream_ptr())
    return out


def advance(state: GrammarState, slots: torch.Tensor, tokens: torch.Tensor, n: int, V: int) -> None:
    """Move the state of every row ``< n`` with a table along the bytes of its sampled id."""
    if n <= 0:
        return
    assert V <= state.vocab
    if not state.rec.is_cuda:
        if bool((slots[:n] < 0).all()):
            return
        reference.grammar_advance(state.pool, state.rec, slots, tokens, n, state.off_np, state.data_np, V)
        return
    assert slots.dtype == torch.int32 and tokens.dtype == torch.int32
    assert slots.is_contiguous() and tokens.is_contiguous() and slots.numel() >= n and tokens.numel() >= n
    native.call("pk_grammar_advance", state.pool.data_ptr(), state.n_tables, state.rec.data_ptr(), state.n_slots,
                slots.data_ptr(), tokens.data_ptr(), n, state.off.data_ptr(), state.data.data_ptr(), state.n_bytes, V,
                native.stream_ptr())


def read_slot(state: GrammarState, slot: int):
    """Read-back of one slot for tests: (table entry, state)."""
    r = state.rec[slot, :2].cpu().tolist()
    return int(r[0]), int(r[1])
