"""Speculative decoding: draft proposers (README "Speculative decoding").

A proposer guesses the next tokens of a sequence; the engine feeds the guesses through one *verify
step* (one forward over ``1 + d`` rows of the sequence, ops/attention.py ``paged_verify``), samples
every row with the sequence's own sampler state and keeps the longest prefix of drafts that equal
the samples, plus one token more.  Drafts are deterministic, so this is exact rejection sampling:
the emitted tokens are those of the engine without speculation.

:class:`NgramProposer` ("prompt lookup") needs no second model: it finds the most recent earlier
occurrence of the sequence's last few tokens and proposes what followed it.
"""
from __future__ import annotations

from typing import Dict, List, Protocol, Tuple

from .sequence import Sequence

METHODS = ("ngram",)
VERIFY_COLUMNS = 16  # columns of the verify attention's MFMA tile: (k + 1) * (n_q / n_kv) must fit


class Proposer(Protocol):
    def propose(self, seq: Sequence, k: int) -> List[int]:
        """At most ``k`` draft tokens that may follow ``seq``'s last token; [] for none."""


def max_draft_tokens(group: int) -> int:
    """Largest k a model whose GQA group (q heads per kv head) is ``group`` can verify."""
    return VERIFY_COLUMNS // group - 1


def ngram_lookup(t: List[int], k: int, n_max: int, n_min: int) -> List[int]:
    """The definition, by search (tests compare :class:`NgramProposer` against it).  Over the tokens
    ``t`` of length L: for n = n_max .. n_min, the largest i with ``i + n <= L - 1`` and
    ``t[i:i+n] == t[L-n:L]`` -- the most recent earlier occurrence of the last n tokens, which may
    overlap them; the first n that has one wins and the drafts are ``t[i+n : min(i+n+k, L)]``."""
    L = len(t)
    for n in range(n_max, n_min - 1, -1):
        if L < n + 1:
            continue
        suffix = t[L - n:]
        for i in range(L - 1 - n, -1, -1):
            if t[i:i + n] == suffix:
                return t[i + n:min(i + n + k, L)]
    return []


class _Index:
    """Per-sequence state: the tokens seen so far and, for every n-gram (n_min <= n <= n_max) that
    ends before the last of them, the start of its last occurrence (one map: tuples of different
    lengths are different keys)."""
    __slots__ = ("tokens", "last")

    def __init__(self):
        self.tokens: List[int] = []
        self.last: Dict[Tuple[int, ...], int] = {}


class NgramProposer:
    """``ngram_lookup`` with an incremental index kept on the sequence (``Sequence.spec_state``): a
    call costs the tokens appended since the last one (times the number of n-gram lengths), not the
    length of the sequence."""

    def __init__(self, n_max: int = 4, n_min: int = 2):
        if not 1 <= n_min <= n_max:
            raise ValueError(f"ngram_min / ngram_max must satisfy 1 <= min <= max (got {n_min}, {n_max})")
        self.n_max, self.n_min = int(n_max), int(n_min)
        self._lengths = tuple(range(self.n_min, self.n_max + 1))
        self._lengths_desc = self._lengths[::-1]

    def propose(self, seq: Sequence, k: int) -> List[int]:
        ix = seq.spec_state
        if ix.__class__ is not _Index:
            ix = seq.spec_state = _Index()
        t, last = ix.tokens, ix.last
        L0 = len(t)
        n_prompt = len(seq.prompt_ids)
        if L0 < n_prompt:
            t.extend(seq.prompt_ids[L0:])
        out = seq.output_ids
        if len(t) < n_prompt + len(out):
            t.extend(out[len(t) - n_prompt:])
        L = len(t)
        n_max = self.n_max
        # token e (L0 <= e < L) becoming "not the last" completes the n-grams that end at e - 1:
        # starts e - n.  Increasing e, so the map ends up holding the largest start of each gram.
        for e in range(max(L0, 1), L):
            tail = tuple(t[max(0, e - n_max):e])
            m = len(tail)
            for n in self._lengths:
                if n > m:
                    break
                last[tail[m - n:]] = e - n
        if k <= 0:
            return []
        tail = tuple(t[max(0, L - n_max):])
        m = len(tail)
        for n in self._lengths_desc:
            if n >= L:   # needs an earlier occurrence: L >= n + 1
                continue
            i = last.get(tail[m - n:])
            if i is not None:
                return t[i + n:min(i + n + k, L)]
        return []
