"""Wire formats of per-token log-probabilities (engine entries → OpenAI JSON / gRPC struct).

An engine entry is ``(logprob, [(token id, logprob) × n])`` for one generated token
(:class:`~polykey_service_amd.engine.sequence.RequestOutput` ``.logprobs``).  Non-finite values
(-inf for a token of zero probability) are clamped to ``CLAMP`` here, at the JSON boundary, so
every response stays valid JSON.

A prompt-logprob entry is ``None`` (the first prompt token) or ``(logprob, rank, [(token id,
logprob) × n])`` for one prompt token given the tokens before it (``RequestOutput.prompt_logprobs``):
:func:`prompt_list` (the vLLM-style ``prompt_logprobs`` of both OpenAI routes), :func:`echo_block`
(``echo`` of /v1/completions: one block over prompt + completion) and :func:`struct_prompt_block`
(gRPC).
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


def prompt_list(tok, ids: Sequence[int], entries: Sequence, n: Optional[int] = None) -> List[Optional[dict]]:
    """``choices[].prompt_logprobs``: ``[null, {token_id, token, logprob, rank, top_logprobs: [{token_id,
    token, logprob}]}, ...]``, one item per prompt token; ``n`` trims the top lists."""
    out: List[Optional[dict]] = []
    for i, e in zip(ids, entries):
        if e is None:
            out.append(None)
            continue
        lp, rank, top = e
        out.append({"token_id": int(i), "token": _tok(tok, i), "logprob": finite(lp), "rank": int(rank),
                    "top_logprobs": [{"token_id": int(j), "token": _tok(tok, j), "logprob": finite(v)}
                                     for j, v in (top if n is None else top[:n])]})
    return out


def echo_block(tok, prompt_ids: Sequence[int], prompt_entries: Sequence, ids: Sequence[int], entries: Sequence,
               n: Optional[int] = None) -> dict:
    """``choices[].logprobs`` of /v1/completions with ``echo``: :func:`completion_block` over the prompt
    followed by the completion.  Entry 0 of ``token_logprobs`` and ``top_logprobs`` is ``null`` (the first
    token has no context); ``text_offset`` starts at 0.  ``n`` trims the prompt's top lists."""
    first = [e is None for e in prompt_entries]
    pe = [(0.0, []) if e is None else (e[0], e[2] if n is None else e[2][:n]) for e in prompt_entries]
    block = completion_block(tok, list(prompt_ids) + list(ids), pe + list(entries))
    for k, none in enumerate(first):
        if none:
            block["token_logprobs"][k] = None
            block["top_logprobs"][k] = None
    return block


def struct_prompt_block(ids: Sequence[int], entries: Sequence) -> dict:
    """``prompt_logprobs`` of the gRPC struct summary: ``{token_ids, token_logprobs (first null), ranks
    (first null), top_logprobs: [[{id, logprob}]]}``."""
    return {"token_ids": [int(i) for i in ids],
            "token_logprobs": [None if e is None else finite(e[0]) for e in entries],
            "ranks": [None if e is None else int(e[1]) for e in entries],
            "top_logprobs": [[] if e is None else [{"id": int(j), "logprob": finite(v)} for j, v in e[2]]
                             for e in entries]}


def parse_prompt_logprobs(body: dict, chat: bool):
    """The request's ``(SamplingParams.prompt_logprobs, echo)``; ValueError for a bad request.
    ``prompt_logprobs: 0..20`` (both routes); ``echo: bool`` (completions only): with ``logprobs: k``
    the prompt is scored with top lists of k, without ``logprobs`` it only prepends the text."""
    def _int(v, name):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_TOP:
            raise ValueError(f"'{name}' must be an integer in [0, {MAX_TOP}]")
        return v

    pl = body.get("prompt_logprobs")
    if pl is not None:
        pl = _int(pl, "prompt_logprobs")
    echo = body.get("echo")
    if echo is not None and not isinstance(echo, bool):
        raise ValueError("'echo' must be a boolean")
    if echo and chat:
        raise ValueError("'echo' is only supported on /v1/completions")
    if echo and body.get("logprobs") is not None:
        k = _int(body["logprobs"], "logprobs")
        pl = k if pl is None else max(pl, k)
    return pl, bool(echo)


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
