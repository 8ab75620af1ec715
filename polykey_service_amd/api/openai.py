"""OpenAI-compatible HTTP route (config 4 of BASELINE.json: "70B TP=8, OpenAI-compatible chat
route").  No reference counterpart (no HTTP/OpenAI route in polykey).

Endpoints: ``POST /v1/chat/completions`` and ``POST /v1/completions`` (``stream: true`` →
server-sent events ending with ``data: [DONE]``), ``GET /v1/models``, ``GET /health``.
Chat requests accept OpenAI ``tools`` / ``tool_choice`` (calls returned as ``tool_calls`` with
``finish_reason: "tool_calls"``) plus the polykey extensions ``execute_tools`` (route the calls
to the gateway's own tools and continue the chat), ``tool_secret_id`` and ``max_tool_rounds``
(service/tool_calls.py).  A tool-enabled chat is decided whole before it is streamed, so its
SSE stream carries the content or the calls in one delta.
Requests are served by the same :class:`ToolRouter` model tools as gRPC, so both fronts share
one continuous-batching engine; ``model`` selects the backend like ``llm.chat:<model>``.

Log-probabilities: chat accepts ``logprobs: true`` with ``top_logprobs: 0..20`` and answers with
``choices[0].logprobs.content``; completions accept ``logprobs: 0..20`` and answer with
``{tokens, token_logprobs, top_logprobs, text_offset}``.  They come from the raw logits (before
temperature / top-k / top-p / min-p) and cover every token the engine generated: they are NOT
cut at a stop string, so they may describe a few tokens past the returned text.  Streamed chunks
carry the entries of the tokens that arrived with them (also when the detokenizer holds the text
back and the chunk's content is ``""``).  Non-finite values are sent as ``-9999.0``.  Logprobs
cannot be combined with function tools (400).

Prompt logprobs: ``prompt_logprobs: 0..20`` (the vLLM extension, both endpoints) adds
``prompt_logprobs: [null, {token_id, token, logprob, rank, top_logprobs: [{token_id, token, logprob}]},
...]`` to every choice: each prompt token scored given the tokens before it, from the raw logits.
``echo: true`` on ``/v1/completions`` prepends the decoded prompt to ``text``; with ``logprobs: k`` the
``logprobs`` block then covers prompt + completion (entry 0 of ``token_logprobs`` / ``top_logprobs`` is
``null``, ``text_offset`` starts at 0), without ``logprobs`` it costs no GPU work.  ``max_tokens: 0`` is
accepted only together with ``echo``: one token is generated and dropped (``completion_tokens`` 0,
``finish_reason`` ``"length"``).  Neither can be streamed or combined with function tools (400).

Penalties: ``frequency_penalty`` / ``presence_penalty`` (-2..2), ``repetition_penalty`` (> 0) and
``logit_bias`` ({token id: -100..100}, at most 300 entries) are applied before sampling
(ops/penalties.py); out-of-range values are a 400.  They may be combined with function tools, and
logprobs keep describing the raw logits.

Guided decoding: ``guided_regex``, ``guided_choice`` and ``guided_json`` (extensions, both
endpoints) and ``response_format: {"type": "json_schema", "json_schema": {"schema": ...}}`` (mapped
to ``guided_json``) constrain the completion on the GPU (engine/grammar.py, ops/grammar.py); an
unsupported pattern or schema keyword is a 400 carrying the compiler's message.
``response_format: {"type": "json_object"}`` is ignored.  A completion cut by ``max_tokens``
(``finish_reason: "length"``) may be a prefix of a match.

Parallel sampling: ``n`` (1..16 and at most the engine's ``max_num_seqs``; anything else is a 400) on
both endpoints answers with n ``choices`` ordered by ``index``, each with its own ``finish_reason``,
``logprobs`` and stop-string cut; ``usage.prompt_tokens`` counts the prompt once and
``completion_tokens`` sums the choices.  Streamed chunks carry their choice's ``index`` (chat: one role
chunk per index), every index gets exactly one chunk with a ``finish_reason``, and ``usage`` rides the
last of them.  ``n > 1`` cannot be combined with function tools (400): a tool chat is multi-round.
"""


import asyncio
import json
import time
import uuid
from typing import Any, Dict, List, Optional

from ..engine.sequence import SamplingParams, check_n
from ..service import logprob_format as lpf
from ..service.base import ToolError
from ..service.tool_calls import run_chat, tool_rounds, validate_tools

_SAMPLING_KEYS = ("max_tokens", "temperature", "top_p", "top_k", "min_p", "seed", "stop", "ignore_eos",
                  "stop_token_ids", "cache_salt", "repetition_penalty", "frequency_penalty", "presence_penalty",
                  "logit_bias", "guided_regex", "guided_choice", "guided_json", "speculative", "n")



def _usage(n_prompt: int, n_out: int, metrics) -> dict:
    """OpenAI usage block; ``prompt_tokens_details.cached_tokens`` = prompt tokens whose KV came
    from the prefix cache (engine/scheduler.py)."""
    return {"prompt_tokens": n_prompt, "completion_tokens": n_out, "total_tokens": n_prompt + n_out,
            "prompt_tokens_details": {"cached_tokens": int((metrics or {}).get("cached_prompt_tokens") or 0)}}


def _llm(router, model: Optional[str]):
    """The AsyncLLM serving ``model`` (the ``llm.chat`` tool registered for it)."""
    models = router.models("llm.chat")
    if not models:
        raise ToolError("UNAVAILABLE", "no local LLM backend attached")
    if model and model not in models:
        raise ToolError("NOT_FOUND", f"model {model!r} not served; available: {models}")
    tool = router.resolve("llm.chat" + (f":{model}" if model else ""), {})
    return tool.llm, tool.model_name


def _lora(router, model: Optional[str]) -> Optional[str]:
    """The LoRA adapter ``model`` names (an adapter is served as a model of its own), or None."""
    tool = router.resolve("llm.chat" + (f":{model}" if model else ""), {})
    return getattr(tool, "lora", None)


def _params(body: Dict[str, Any], chat: bool = True) -> SamplingParams:
    d = {k: body[k] for k in _SAMPLING_KEYS if k in body and body[k] is not None}
    d["logprobs"] = lpf.parse_openai(body, chat)
    if "guided_choice" in d and not d["guided_choice"]:
        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
    rf = body.get("response_format")
    if isinstance(rf, dict) and rf.get("type") == "json_schema":  # (json_object and text: ignored)
        js = rf.get("json_schema")
        if not isinstance(js, dict) or not isinstance(js.get("schema"), (dict, str)):
            raise ValueError("response_format json_schema needs 'json_schema': {'schema': {...}}")
        if any(k in d for k in ("guided_regex", "guided_choice", "guided_json")):
            raise ValueError("at most one of response_format json_schema, guided_regex, guided_choice and "
                             "guided_json may be set")
        d["guided_json"] = js["schema"]
    if "max_completion_tokens" in body and "max_tokens" not in d:
        d["max_tokens"] = body["max_completion_tokens"]
    d.setdefault("max_tokens", 256)
    d.setdefault("temperature", 1.0)
    sp = SamplingParams.from_dict(d)
    sp.validate(1 << 30)
    return sp


def create_app(router):
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, StreamingResponse

    app = FastAPI(title="polykey OpenAI-compatible API")

    def err(status: int, msg: str, typ: str = "invalid_request_error"):
        return JSONResponse({"error": {"message": msg, "type": typ}}, status_code=status)

    @app.get("/health")
    async def health():
        llm = getattr(router, "llm", None)
        ok = llm is None or llm.healthy()
        return JSONResponse({"status": "ok" if ok else "unhealthy"}, status_code=200 if ok else 503)

    @app.get("/v1/models")
    async def models():
        now = int(time.time())
        data = []
        for m in router.models("llm.chat"):
            entry = {"id": m, "object": "model", "created": now, "owned_by": "polykey"}
            parent = getattr(router.resolve(f"llm.chat:{m}", {}), "parent", None)
            if parent is not None:  # a LoRA adapter of that base model
                entry["parent"] = parent
            data.append(entry)
        return {"object": "list", "data": data}

    async def _run(body: Dict[str, Any], chat: bool):
        drop = False  # echo with max_tokens 0: the one generated token is not reported
        try:
            llm, model = _llm(router, body.get("model"))
            n_pl, echo = lpf.parse_prompt_logprobs(body, chat)
            if echo and body.get("max_tokens") == 0 and not isinstance(body["max_tokens"], bool):
                body, drop = {**body, "max_tokens": 1}, True
            sp = _params(body, chat)
            sp.prompt_logprobs = n_pl
            n_pl = body.get("prompt_logprobs")  # the length of the lists the client asked for itself
            sp.lora = _lora(router, body.get("model"))
            check_n(llm, sp)
            if body.get("stream") and (echo or sp.prompt_logprobs is not None):
                raise ValueError("'echo' / 'prompt_logprobs' cannot be combined with 'stream'")
        except ToolError as e:
            return err(404 if e.code == "NOT_FOUND" else 503, e.message)
        except (ValueError, TypeError) as e:
            return err(400, str(e))
        tok = llm.tokenizer
        if chat:
            msgs = body.get("messages")
            if not isinstance(msgs, list) or not msgs:
                return err(400, "'messages' must be a non-empty list")
            try:
                tools, choice = validate_tools(body.get("tools"), body.get("tool_choice"))
            except ValueError as e:
                return err(400, str(e))
            if tools and choice != "none":
                if sp.logprobs is not None:
                    return err(400, "'logprobs' cannot be combined with function tools")
                if sp.n > 1:
                    return err(400, "'n' > 1 cannot be combined with function tools")
                if sp.prompt_logprobs is not None:
                    return err(400, "'prompt_logprobs' cannot be combined with function tools")
                return await _run_tools(body, llm, model, msgs, sp, tools, choice)
            prompt_ids = tok.encode(tok.apply_chat_template(msgs))
        else:
            p = body.get("prompt")
            if isinstance(p, list) and p and isinstance(p[0], int):
                prompt_ids = [int(x) for x in p]
            elif isinstance(p, str) and p:
                prompt_ids = tok.encode(p)
            else:
                return err(400, "'prompt' must be a non-empty string or token id list")
        rid = ("chatcmpl-" if chat else "cmpl-") + uuid.uuid4().hex[:24]
        created = int(time.time())
        obj = "chat.completion" if chat else "text_completion"

        if body.get("stream"):
            async def sse():
                from ..engine.tokenizer import IncrementalDetokenizer
                n = sp.n
                toks: List[List[int]] = [[] for _ in range(n)]
                detoks = [IncrementalDetokenizer(tok) for _ in range(n)]
                finish: List[Optional[str]] = [None] * n
                final_metrics = None
                offset = [0] * n  # completions: text_offset of the next token
                left, last_index = n, 0
                chunk_obj = obj + (".chunk" if chat else "")

                def chunk(choice, **kw):
                    ch = {"id": rid, "object": chunk_obj, "created": created, "model": model, "choices": [choice], **kw}
                    return f"data: {json.dumps(ch)}\n\n"

                def finish_choice(i):
                    return ({"index": i, "delta": {}, "finish_reason": finish[i]} if chat
                            else {"index": i, "text": "", "finish_reason": finish[i]})

                if chat:
                    for i in range(n):
                        yield chunk({"index": i, "delta": {"role": "assistant"}, "finish_reason": None})
                agen = llm.generate(prompt_ids, sp, request_id=rid)
                try:
                    async for out in agen:
                        i = out.index
                        toks[i].extend(out.new_token_ids)
                        finish[i] = out.finish_reason
                        if i == 0 or final_metrics is None:
                            final_metrics = out.metrics or final_metrics
                        delta = detoks[i].push(out.new_token_ids)
                        lp = None
                        if sp.logprobs is not None and out.logprobs:
                            if chat:
                                lp = {"content": lpf.chat_content(tok, out.new_token_ids, out.logprobs)}
                            else:
                                lp = lpf.completion_block(tok, out.new_token_ids, out.logprobs, offset[i])
                                offset[i] += sum(len(t) for t in lp["tokens"])
                        if delta or lp is not None:
                            choice = ({"index": i, "delta": {"content": delta}, "finish_reason": None} if chat
                                      else {"index": i, "text": delta, "finish_reason": None})
                            if lp is not None:
                                choice["logprobs"] = lp
                            yield chunk(choice)
                        if out.finished:
                            left -= 1
                            if left:  # the last choice's finish chunk carries the usage, below
                                yield chunk(finish_choice(i))
                            else:
                                last_index = i
                finally:
                    await agen.aclose()
                yield chunk(finish_choice(last_index),
                            usage=_usage(len(prompt_ids), sum(len(t) for t in toks), final_metrics))
                yield "data: [DONE]\n\n"

            return StreamingResponse(sse(), media_type="text/event-stream")

        if sp.n > 1:
            try:
                all_toks, lasts = await llm.generate_choices(prompt_ids, sp, request_id=rid)
            except ValueError as e:  # refused by the engine itself (n above a remote engine's max_num_seqs)
                return err(400, str(e))
        else:
            toks, last = await llm.generate_all(prompt_ids, sp, request_id=rid)
            all_toks, lasts = [toks], [last]
        choices = []
        plp = lasts[0].prompt_logprobs if lasts[0] is not None else None  # the request's, on choice 0's output
        if drop:
            all_toks = [[] for _ in all_toks]
        for i, (toks, last) in enumerate(zip(all_toks, lasts)):
            text = tok.decode(toks)
            if sp.stop:
                cuts = [text.find(s) for s in sp.stop if text.find(s) >= 0]
                if cuts:
                    text = text[:min(cuts)]
            if echo:
                text = tok.decode(prompt_ids) + text
            reason = "length" if drop else (last.finish_reason if last else None)
            choice = ({"index": i, "message": {"role": "assistant", "content": text}, "finish_reason": reason} if chat
                      else {"index": i, "text": text, "finish_reason": reason})
            if sp.logprobs is not None:
                entries = (last.logprobs if last else None) or []
                if echo:
                    choice["logprobs"] = lpf.echo_block(tok, prompt_ids, plp or [None] * len(prompt_ids), toks, entries,
                                                        sp.logprobs)
                else:
                    choice["logprobs"] = ({"content": lpf.chat_content(tok, toks, entries)} if chat
                                          else lpf.completion_block(tok, toks, entries))
            if n_pl is not None:
                choice["prompt_logprobs"] = lpf.prompt_list(tok, prompt_ids, plp or [None] * len(prompt_ids), n_pl)
            choices.append(choice)
        return {"id": rid, "object": obj, "created": created, "model": model, "choices": choices,
                "usage": _usage(len(prompt_ids), sum(len(t) for t in all_toks), lasts[0].metrics if lasts[0] else None)}

    async def _run_tools(body, llm, model, msgs, sp, tools, choice):
        rid = "chatcmpl-" + uuid.uuid4().hex[:24]
        created = int(time.time())
        try:
            rounds = tool_rounds(body.get("max_tool_rounds"))
            oc = await run_chat(llm, llm.tokenizer.chat_template, msgs, sp, tools, choice, router=router,
                                execute=bool(body.get("execute_tools")), secret_id=body.get("tool_secret_id"),
                                max_rounds=rounds, request_id=rid)
        except (ValueError, TypeError) as e:
            return err(400, str(e))
        usage = _usage(oc.prompt_tokens, oc.completion_tokens, oc.metrics)
        extra = {"polykey_tool_results": oc.executed} if oc.executed else {}
        if not body.get("stream"):
            msg = {"role": "assistant", "content": oc.content if oc.content or not oc.tool_calls else None}
            if oc.tool_calls:
                msg["tool_calls"] = oc.tool_calls
            return {"id": rid, "object": "chat.completion", "created": created, "model": model,
                    "choices": [{"index": 0, "message": msg, "finish_reason": oc.finish_reason}], "usage": usage,
                    **extra}

        async def sse():
            def chunk(delta, finish=None, **kw):
                return "data: " + json.dumps({"id": rid, "object": "chat.completion.chunk", "created": created,
                                              "model": model, "choices": [{"index": 0, "delta": delta,
                                                                           "finish_reason": finish}], **kw}) + "\n\n"
            yield chunk({"role": "assistant"})
            if oc.tool_calls:
                yield chunk({"tool_calls": [{"index": i, **c} for i, c in enumerate(oc.tool_calls)]})
            elif oc.content:
                yield chunk({"content": oc.content})
            yield chunk({}, oc.finish_reason, usage=usage, **extra)
            yield "data: [DONE]\n\n"

        return StreamingResponse(sse(), media_type="text/event-stream")

    @app.post("/v1/chat/completions")
    async def chat_completions(request: Request):
        try:
            body = await request.json()
        except json.JSONDecodeError:
            return err(400, "invalid JSON")
        return await _run(body, chat=True)

    @app.post("/v1/completions")
    async def completions(request: Request):
        try:
            body = await request.json()
        except json.JSONDecodeError:
            return err(400, "invalid JSON")
        return await _run(body, chat=False)

    return app


class _HttpHandle:
    def __init__(self, server, task):
        self.server = server
        self.task = task

    async def shutdown(self):
        self.server.should_exit = True
        await self.task


async def serve_openai(router, addr: str, logger):
    import uvicorn
    host, _, port = addr.rpartition(":")
    cfg = uvicorn.Config(create_app(router), host=host or "0.0.0.0", port=int(port), log_level="warning",
                         lifespan="off")
    server = uvicorn.Server(cfg)
    task = asyncio.create_task(server.serve())
    logger.info("openai route listening", address=addr)
    return _HttpHandle(server, task)
