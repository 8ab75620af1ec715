"""Parallel sampling (``n``) through the public interfaces on the CPU engine (tiny-llama): both OpenAI
routes plain and streamed, the gRPC struct ``choices``, every refusal, a remote-engine round trip, and
the wire frames of an n = 1 request, which stay what they were."""
import asyncio
import dataclasses
import json
import threading

import grpc
import msgpack
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import ReplicaPool, attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig
from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.engine import remote as remote_mod
from polykey_service_amd.engine.async_llm import AsyncLLM
from polykey_service_amd.engine.remote import EngineServer, RemoteEngine
from polykey_service_amd.engine.sequence import SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.utils import slog

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
TOOLS = [{"type": "function", "function": {"name": "f", "description": "d",
                                           "parameters": {"type": "object", "properties": {}}}}]


def make_engine():
    return LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                                  hip_graphs=False, device="cpu"), ParallelState())


@pytest.fixture(scope="module")
def router():
    r = ToolRouter()
    attach_local_llm(r, ServerConfig(model="tiny-llama", backend="local"), slog.Logger(open("/dev/null", "w")),
                     engine=make_engine())
    yield r
    r.llm.shutdown()


@pytest.fixture(scope="module")
def client(router):
    from fastapi.testclient import TestClient

    from polykey_service_amd.api.openai import create_app
    return TestClient(create_app(router))


# -------------------------------------------------------------------------------- OpenAI
def test_chat_route_returns_n_choices(client):
    base = {"model": "tiny-llama", "max_tokens": 6, "ignore_eos": True, "messages": MSGS, "seed": 7}
    r = client.post("/v1/chat/completions", json={**base, "n": 3, "logprobs": True, "top_logprobs": 2})
    body = r.json()
    assert r.status_code == 200, body
    assert [c["index"] for c in body["choices"]] == [0, 1, 2]
    assert all(c["finish_reason"] == "length" and len(c["logprobs"]["content"]) == 6 for c in body["choices"])
    one = client.post("/v1/chat/completions", json={**base, "logprobs": True, "top_logprobs": 2}).json()
    assert len(one["choices"]) == 1
    assert body["usage"]["prompt_tokens"] == one["usage"]["prompt_tokens"]  # the prompt counts once
    assert body["usage"]["completion_tokens"] == 18 and one["usage"]["completion_tokens"] == 6
    assert body["usage"]["total_tokens"] == body["usage"]["prompt_tokens"] + 18
    # choice 0 is the n = 1 request; the seeded choices are not all one stream
    assert body["choices"][0]["message"] == one["choices"][0]["message"]
    assert body["choices"][0]["logprobs"]["content"][0] == one["choices"][0]["logprobs"]["content"][0]
    assert len({json.dumps(c["logprobs"]["content"]) for c in body["choices"]}) > 1


def test_completions_route_returns_n_choices_with_stop_cut(client):
    req = {"model": "tiny-llama", "prompt": [1, 4, 5, 9, 2], "max_tokens": 5, "ignore_eos": True, "temperature": 0,
           "n": 2}
    body = client.post("/v1/completions", json=req).json()
    assert [c["index"] for c in body["choices"]] == [0, 1] and body["usage"]["completion_tokens"] == 10
    assert body["choices"][0]["text"] == body["choices"][1]["text"]  # greedy choices are identical
    text = body["choices"][0]["text"]
    if len(text) > 1:  # the stop cut applies to every choice
        cut = client.post("/v1/completions", json={**req, "stop": [text[1:]]}).json()
        assert [c["text"] for c in cut["choices"]] == [text[:1]] * 2


def _sse(client, route, req):
    with client.stream("POST", route, json=req) as resp:
        assert resp.status_code == 200
        lines = [l for l in resp.iter_lines() if l]
    assert lines[-1] == "data: [DONE]"
    return [json.loads(l[len("data: "):]) for l in lines[:-1]]


@pytest.mark.parametrize("chat", [True, False])
def test_streams_carry_the_index_and_one_finish_chunk_per_choice(client, chat):
    req = {"model": "tiny-llama", "stream": True, "max_tokens": 5, "ignore_eos": True, "seed": 3, "n": 3,
           "logprobs": True if chat else 0}
    req.update({"messages": MSGS} if chat else {"prompt": [1, 4, 5]})
    chunks = _sse(client, "/v1/chat/completions" if chat else "/v1/completions", req)
    assert all(len(ch["choices"]) == 1 for ch in chunks)
    if chat:
        roles = [ch["choices"][0]["index"] for ch in chunks if ch["choices"][0]["delta"].get("role")]
        assert roles == [0, 1, 2]
    fin = [ch["choices"][0]["index"] for ch in chunks if ch["choices"][0]["finish_reason"] is not None]
    assert sorted(fin) == [0, 1, 2]
    assert [("usage" in ch) for ch in chunks] == [False] * (len(chunks) - 1) + [True]
    assert chunks[-1]["choices"][0]["finish_reason"] == "length"
    assert chunks[-1]["usage"]["completion_tokens"] == 15
    per = {0: 0, 1: 0, 2: 0}
    for ch in chunks:
        c = ch["choices"][0]
        lp = c.get("logprobs")
        if lp is not None:
            per[c["index"]] += len(lp["content"] if chat else lp["tokens"])
    assert per == {0: 5, 1: 5, 2: 5}


def test_n1_stream_is_what_it_was(client):
    req = {"model": "tiny-llama", "stream": True, "max_tokens": 4, "ignore_eos": True, "messages": MSGS, "n": 1}
    chunks = _sse(client, "/v1/chat/completions", req)
    assert chunks[0]["choices"] == [{"index": 0, "delta": {"role": "assistant"}, "finish_reason": None}]
    assert chunks[-1]["choices"] == [{"index": 0, "delta": {}, "finish_reason": "length"}]
    assert chunks[-1]["usage"]["completion_tokens"] == 4
    assert all(ch["choices"][0]["index"] == 0 and ch["choices"][0]["finish_reason"] is None for ch in chunks[:-1])


def test_openai_refusals_are_400_and_name_n(client):
    base = {"model": "tiny-llama", "max_tokens": 2, "messages": MSGS}
    for bad in (True, "2", 2.5, 0, 17, 9):  # 9 > max_num_seqs = 8
        r = client.post("/v1/chat/completions", json={**base, "n": bad})
        assert r.status_code == 400 and "n must be" in r.json()["error"]["message"], (bad, r.json())
        r = client.post("/v1/completions", json={"model": "tiny-llama", "prompt": "x", "n": bad})
        assert r.status_code == 400 and "n must be" in r.json()["error"]["message"], (bad, r.json())
    r = client.post("/v1/chat/completions", json={**base, "n": 2, "tools": TOOLS})
    assert r.status_code == 400 and "'n'" in r.json()["error"]["message"] and "tools" in r.json()["error"]["message"]
    assert client.post("/v1/chat/completions", json={**base, "n": 1, "tools": TOOLS}).status_code == 200
    assert client.post("/v1/chat/completions", json={**base, "n": 8}).status_code == 200


# ---------------------------------------------------------------------------------- gRPC
def _grpc_req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_grpc_struct_choices_and_refusals(router):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        st = ch.unary_stream(proto.EXECUTE_TOOL_STREAM, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                             response_deserializer=proto.ExecuteToolResponse.FromString)
        kw = dict(prompt_token_ids=[1, 5, 6], max_tokens=5, ignore_eos=True, seed=4, temperature=1.0)
        r = call(_grpc_req("llm.generate", n=3, logprobs=1, return_token_ids=True, **kw, **{"return": "struct"}),
                 timeout=60)
        d = proto.struct_to_dict(r.struct_output)
        assert [int(c["index"]) for c in d["choices"]] == [0, 1, 2]
        for c in d["choices"]:
            assert set(c) == {"index", "text", "finish_reason", "token_ids", "logprobs"}
            assert c["finish_reason"] == "length" and len(c["token_ids"]) == 5 and len(c["logprobs"]["token_ids"]) == 5
        assert d["text"] == d["choices"][0]["text"] and d["finish_reason"] == d["choices"][0]["finish_reason"]
        assert d["token_ids"] == d["choices"][0]["token_ids"] and d["logprobs"] == d["choices"][0]["logprobs"]
        assert d["usage"] == {"prompt_tokens": 3, "completion_tokens": 15, "total_tokens": 18}
        one = proto.struct_to_dict(call(_grpc_req("llm.generate", return_token_ids=True, **kw, **{"return": "struct"}),
                                        timeout=60).struct_output)
        assert "choices" not in one and one["token_ids"] == d["choices"][0]["token_ids"]
        r = call(_grpc_req("llm.chat", messages=MSGS, max_tokens=3, n=2, **{"return": "struct"}), timeout=60)
        assert len(proto.struct_to_dict(r.struct_output)["choices"]) == 2

        def refused(fn, req, *words):
            with pytest.raises(grpc.RpcError) as ei:
                out = fn(req, timeout=20)
                list(out) if fn is st else None
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT, ei.value
            assert all(w in ei.value.details() for w in words), ei.value.details()

        for bad in (True, "2", 2.5, 0, 17, 9):
            refused(call, _grpc_req("llm.generate", prompt="x", n=bad, **{"return": "struct"}), "n must be")
        refused(call, _grpc_req("llm.generate", prompt="x", n=2), "'n'", "struct")
        refused(call, _grpc_req("llm.chat", messages=MSGS, n=2, tools=TOOLS, **{"return": "struct"}), "'n'", "tools")
        refused(st, _grpc_req("llm.generate", prompt="x", n=2, **{"return": "struct"}), "'n'", "ExecuteToolStream")
        # n = 1 still streams and still answers with a string
        assert call(_grpc_req("llm.generate", prompt="x", n=1, max_tokens=2), timeout=60).WhichOneof("output") == \
            "string_output"
        assert len(list(st(_grpc_req("llm.generate", prompt="x", n=1, max_tokens=2), timeout=60))) >= 1


# ------------------------------------------------------------------------- remote engine
def test_remote_engine_serves_n3_and_n1_frames_are_unchanged(monkeypatch):
    sent = []
    real_send = remote_mod._send

    def spy_send(sock, lock, obj):
        sent.append(msgpack.packb(obj, use_bin_type=True))
        return real_send(sock, lock, obj)
    monkeypatch.setattr(remote_mod, "_send", spy_send)
    llm = AsyncLLM(make_engine())
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="t")
    pool = ReplicaPool([remote])
    prompt = [3, 1, 4, 1, 5, 9, 2, 6]
    sp3 = SamplingParams(max_tokens=5, ignore_eos=True, temperature=1.0, seed=8, logprobs=1, n=3)
    sp1 = SamplingParams(max_tokens=5, ignore_eos=True, temperature=1.0, seed=8, logprobs=1)

    async def go():
        local = await llm.generate_choices(prompt, sp3)
        far = await pool.generate_choices(prompt, sp3)                      # final-only on the wire
        steps = [o async for o in remote.generate(prompt, sp3)]             # per step
        mark = len(sent)
        one = await remote.generate_all(prompt, sp1, request_id="one")
        return local, far, steps, sent[mark:], one
    try:
        (ltoks, llast), (rtoks, rlast), steps, frames, (otoks, olast) = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert rtoks == ltoks and len(rtoks) == 3 and all(len(t) == 5 for t in rtoks)
    assert [o.index for o in rlast] == [0, 1, 2] and all(o.finished and o.finish_reason == "length" for o in rlast)
    assert [o.logprobs for o in rlast] == [o.logprobs for o in llast]
    assert {o.index for o in steps} == {0, 1, 2} and sum(o.finished for o in steps) == 3
    for i in range(3):
        assert sum((o.new_token_ids for o in steps if o.index == i), []) == ltoks[i]
    assert otoks == ltoks[0] and olast.index == 0
    assert not srv._final and not srv._final_lp and not srv._left and not srv._owner
    # the n = 1 request's frames, byte for byte: no "n" in its params, no index in its item
    add = [msgpack.unpackb(f, raw=False) for f in frames]
    add = [m for m in add if m.get("op") == "add"]
    assert len(add) == 1 and "n" not in add[0]["params"]
    want = {f.name: getattr(sp1, f.name) for f in dataclasses.fields(sp1) if f.name != "n"}
    assert set(add[0]["params"]) == set(want)
    outs = [m for m in (msgpack.unpackb(f, raw=False) for f in frames) if m.get("op") == "out"]
    items = [it for m in outs for it in m["items"] if it[0] == "one"]
    assert len(items) == 1 and len(items[0]) == 9
    lps = [[lp, [list(t) for t in top]] for lp, top in olast.logprobs]
    assert items[0] == ["one", otoks, True, "length", len(prompt), 5, olast.metrics, None, lps]


def test_dropped_client_aborts_every_choice():
    eng = make_engine()
    llm = AsyncLLM(eng)
    nb = eng.bm.num_blocks

    async def go():
        agen = llm.generate(list(range(3, 60)), SamplingParams(max_tokens=400, ignore_eos=True, n=4), request_id="gone")
        first = await agen.__anext__()
        await agen.aclose()  # the client went away after its first output
        return first
    try:
        first = asyncio.run(go())
    finally:
        llm.shutdown()  # the engine thread drains its commands (the abort) before it stops
    assert first.request_id == "gone" and not first.finished
    # (a step of the aborted choices may still be in flight; the scheduler and the pool hold nothing)
    assert not eng.scheduler.has_work() and eng.bm.num_free == nb and not eng.scheduler.by_request
    assert not eng.scheduler.groups and not eng.scheduler.parked


def test_n_above_a_remote_engines_cap_is_a_value_error_at_the_front_end():
    """A remote front end cannot see the engine's max_num_seqs: the engine refuses, and the refusal
    arrives as the ValueError the routes answer with 400 / INVALID_ARGUMENT."""
    llm = AsyncLLM(LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=2, max_num_batched_tokens=128,
                                          max_model_len=256, hip_graphs=False, device="cpu"), ParallelState()))
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="cap")

    async def go():
        with pytest.raises(ValueError, match="n must be at most max_num_seqs"):
            await ReplicaPool([remote]).generate_choices([1, 2, 3], SamplingParams(max_tokens=2, n=3))
        return await remote.generate_choices([1, 2, 3], SamplingParams(max_tokens=2, n=2))
    try:
        toks, _ = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert [len(t) for t in toks] == [2, 2] and not srv._left and not srv._owner
