"""Wire formats of per-token log-probabilities (engine entries → OpenAI JSON / gRPC struct).

An engine entry is ``(logprob, [(token id, logprob) × n])`` for one generated token
(:class:`~polykey_service_amd.engine.sequence.RequestOutput` ``.logprobs``).  Non-finite values
(-inf for a token of zero probability) are clamped to ``CLAMP`` here, at the JSON boundary, so
every response stays valid JSON.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

CLAMP = -9999.0
MAX_TOP = 20


def finite(v: float) -> float:
    v = float(v)
    return v if math.isfinite(v) else CLAMP


def _tok(tok, i: int) -> str:
    return tok.decode([int(i)], keep_special=True)


def _item(tok, i: int, lp: float) -> dict:
    s = _tok(tok, i)
    return {"token": s, "logprob": finite(lp), "bytes": list(s.encode("utf-8"))}


def chat_content(tok, ids: Sequence[int], entries: Sequence) -> List[dict]:
    """``choices[].logprobs.content`` of /v1/chat/completions: one item per generated token."""
    out = []
    for i, (lp, top) in zip(ids, entries):
        d = _item(tok, i, lp)
        d["top_logprobs"] = [_item(tok, j, v) for j, v in top]
        out.append(d)
    return out


def completion_block(tok, ids: Sequence[int], entries: Sequence, offset: int = 0) -> dict:
    """``choices[].logprobs`` of /v1/completions.  ``text_offset`` counts the characters of the
    tokens' own decodings from ``offset`` (the completion only: the prompt is not echoed)."""
    tokens, lps, tops, offs = [], [], [], []
    for i, (lp, top) in zip(ids, entries):
        s = _tok(tok, i)
        tokens.append(s)
        lps.append(finite(lp))
        d: dict = {}
        for j, v in top:  # ids that decode to the same string share a key: the most likely one stays
            d.setdefault(_tok(tok, j), finite(v))
        tops.append(d)
        offs.append(offset)
        offset += len(s)
    return {"tokens": tokens, "token_logprobs": lps, "top_logprobs": tops, "text_offset": offs}


def struct_block(ids: Sequence[int], entries: Sequence) -> dict:
    """``logprobs`` of the gRPC struct summary of ``llm.chat`` / ``llm.generate``."""
    n = min(len(ids), len(entries))
    return {"token_ids": [int(i) for i in ids[:n]],
            "token_logprobs": [finite(lp) for lp, _ in entries[:n]],
            "top_logprobs": [[{"id": int(j), "logprob": finite(v)} for j, v in top] for _, top in entries[:n]]}


def parse_openai(body: dict, chat: bool) -> Optional[int]:
    """The request's ``SamplingParams.logprobs`` (None = off); ValueError for a bad request.
    Chat: ``logprobs: bool`` + ``top_logprobs: 0..20``; completions: ``logprobs: 0..20``."""
    def _int(v, name):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_TOP:
            raise ValueError(f"'{name}' must be an integer in [0, {MAX_TOP}]")
        return v

    lp = body.get("logprobs")
    if not chat:
        return None if lp is None else _int(lp, "logprobs")
    if lp is not None and not isinstance(lp, bool):
        raise ValueError("'logprobs' must be a boolean")
    top = body.get("top_logprobs")
    if top is not None:
        top = _int(top, "top_logprobs")
        if not lp:
            raise ValueError("'top_logprobs' requires 'logprobs': true")
    return (top or 0) if lp else None
