"""Per-token logprobs through the public interfaces on the CPU engine (tiny Llama, reference ops):
the OpenAI chat route (plain and streamed) and completions route, the gRPC ``llm.generate`` /
``llm.chat`` struct (unary and stream), the 400s, the JSON clamp, and a remote-engine round trip
including the ``final_only`` accumulation."""
import asyncio
import json
import threading

import grpc
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig
from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.engine.async_llm import AsyncLLM
from polykey_service_amd.engine.remote import EngineServer, RemoteEngine
from polykey_service_amd.engine.sequence import SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.service import logprob_format as lpf
from polykey_service_amd.utils import slog

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]


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


def _check_chat_items(items, n_tokens, n_top):
    assert len(items) == n_tokens
    for it in items:
        assert set(it) == {"token", "logprob", "bytes", "top_logprobs"}
        assert it["logprob"] <= 0.0 and it["bytes"] == list(it["token"].encode("utf-8"))
        assert len(it["top_logprobs"]) == n_top
        lps = [t["logprob"] for t in it["top_logprobs"]]
        assert lps == sorted(lps, reverse=True) and all(set(t) == {"token", "logprob", "bytes"} for t in it["top_logprobs"])


def test_chat_route_returns_logprobs(client):
    base = {"model": "tiny-llama", "max_tokens": 6, "ignore_eos": True, "temperature": 0, "messages": MSGS}
    r = client.post("/v1/chat/completions", json={**base, "logprobs": True, "top_logprobs": 3})
    body = r.json()
    assert r.status_code == 200, body
    items = body["choices"][0]["logprobs"]["content"]
    _check_chat_items(items, body["usage"]["completion_tokens"], 3)
    for it in items:  # greedy: the sampled token heads its own top list
        assert it["top_logprobs"][0]["token"] == it["token"] and it["top_logprobs"][0]["logprob"] == it["logprob"]
    # logprobs: true alone → the sampled token only; no logprobs → no field, same text
    r0 = client.post("/v1/chat/completions", json={**base, "logprobs": True}).json()
    _check_chat_items(r0["choices"][0]["logprobs"]["content"], 6, 0)
    plain = client.post("/v1/chat/completions", json=base).json()
    assert "logprobs" not in plain["choices"][0]
    assert plain["choices"][0]["message"]["content"] == body["choices"][0]["message"]["content"]
    assert [it["logprob"] for it in r0["choices"][0]["logprobs"]["content"]] == [it["logprob"] for it in items]


def test_chat_route_streams_logprobs_for_every_token(client):
    req = {"model": "tiny-llama", "stream": True, "max_tokens": 9, "ignore_eos": True, "messages": MSGS,
           "logprobs": True, "top_logprobs": 2, "seed": 5}
    with client.stream("POST", "/v1/chat/completions", json=req) as resp:
        lines = [l for l in resp.iter_lines() if l]
    assert lines[-1] == "data: [DONE]"
    chunks = [json.loads(l[len("data: "):]) for l in lines[:-1]]
    items = []
    for ch in chunks:
        lp = ch["choices"][0].get("logprobs")
        if lp is not None:
            assert "content" in ch["choices"][0]["delta"]  # emitted even when the text is held back ("")
            items += lp["content"]
    assert chunks[-1]["usage"]["completion_tokens"] == 9
    _check_chat_items(items, 9, 2)


def test_completions_route_returns_logprobs(client):
    r = client.post("/v1/completions", json={"model": "tiny-llama", "prompt": [1, 4, 5], "max_tokens": 5,
                                             "ignore_eos": True, "temperature": 0, "logprobs": 2})
    body = r.json()
    assert r.status_code == 200, body
    lp = body["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == 5
    assert all(v <= 0.0 for v in lp["token_logprobs"])
    assert all(isinstance(d, dict) and 1 <= len(d) <= 2 for d in lp["top_logprobs"])
    assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])
    for tok, v, d in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert max(d.values()) == v and d.get(tok) == v  # greedy
    r = client.post("/v1/completions", json={"model": "tiny-llama", "prompt": [1, 4, 5], "max_tokens": 3,
                                             "ignore_eos": True, "logprobs": 0})
    assert [len(d) for d in r.json()["choices"][0]["logprobs"]["top_logprobs"]] == [0, 0, 0]
    assert "logprobs" not in client.post("/v1/completions", json={"model": "tiny-llama", "prompt": [1, 4, 5],
                                                                  "max_tokens": 2}).json()["choices"][0]


def test_bad_requests_are_400(client):
    base = {"model": "tiny-llama", "max_tokens": 2, "messages": MSGS}
    assert client.post("/v1/chat/completions", json={**base, "top_logprobs": 2}).status_code == 400
    assert client.post("/v1/chat/completions", json={**base, "logprobs": False, "top_logprobs": 2}).status_code == 400
    assert client.post("/v1/chat/completions", json={**base, "logprobs": True, "top_logprobs": 21}).status_code == 400
    assert client.post("/v1/chat/completions", json={**base, "logprobs": True, "top_logprobs": -1}).status_code == 400
    assert client.post("/v1/completions", json={"model": "tiny-llama", "prompt": "x", "logprobs": 21}
                       ).status_code == 400
    tools = [{"type": "function", "function": {"name": "f", "description": "d",
                                               "parameters": {"type": "object", "properties": {}}}}]
    r = client.post("/v1/chat/completions", json={**base, "logprobs": True, "tools": tools})
    assert r.status_code == 400 and "tools" in r.json()["error"]["message"]
    assert client.post("/v1/chat/completions", json={**base, "logprobs": True, "top_logprobs": 20}).status_code == 200


class _Tok:
    def decode(self, ids, keep_special=False):
        return "".join(chr(97 + i) for i in ids)


def test_non_finite_values_are_clamped_to_valid_json():
    ninf = float("-inf")
    entries = [(ninf, [(0, -0.5), (1, ninf)]), (-0.25, [(2, float("nan"))])]
    for block in (lpf.chat_content(_Tok(), [3, 4], entries), lpf.completion_block(_Tok(), [3, 4], entries),
                  lpf.struct_block([3, 4], entries)):
        text = json.dumps(block, allow_nan=False)  # raises on inf / nan
        assert str(lpf.CLAMP) in text
    assert lpf.CLAMP == -9999.0 and lpf.finite(ninf) == -9999.0 and lpf.finite(-1.5) == -1.5
    c = lpf.chat_content(_Tok(), [3, 4], entries)
    assert c[0]["logprob"] == -9999.0 and c[0]["top_logprobs"][1]["logprob"] == -9999.0 and c[1]["logprob"] == -0.25
    assert lpf.completion_block(_Tok(), [3, 4], entries)["text_offset"] == [0, 1]


def _grpc_req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_grpc_struct_unary_and_stream(router):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        r = call(_grpc_req("llm.generate", prompt_token_ids=[1, 5, 6], max_tokens=5, ignore_eos=True, logprobs=2,
                           return_token_ids=True, **{"return": "struct"}), timeout=60)
        d = proto.struct_to_dict(r.struct_output)
        lp = d["logprobs"]
        assert [int(t) for t in lp["token_ids"]] == [int(t) for t in d["token_ids"]] and len(lp["token_ids"]) == 5
        assert len(lp["token_logprobs"]) == 5 and all(v <= 0.0 for v in lp["token_logprobs"])
        assert [len(t) for t in lp["top_logprobs"]] == [2] * 5
        for tid, v, top in zip(lp["token_ids"], lp["token_logprobs"], lp["top_logprobs"]):
            assert set(top[0]) == {"id", "logprob"} and int(top[0]["id"]) == int(tid) and top[0]["logprob"] == v
        # not asking for the struct: the plain string, as before
        r = call(_grpc_req("llm.generate", prompt_token_ids=[1, 5, 6], max_tokens=5, ignore_eos=True, logprobs=2),
                 timeout=60)
        assert r.WhichOneof("output") == "string_output" and r.string_output == d["text"]
        # no logprobs asked: no field
        r = call(_grpc_req("llm.generate", prompt_token_ids=[1, 5, 6], max_tokens=2, **{"return": "struct"}), timeout=60)
        assert "logprobs" not in proto.struct_to_dict(r.struct_output)
        with pytest.raises(grpc.RpcError) as ei:
            call(_grpc_req("llm.generate", prompt="x", logprobs=21), timeout=10)
        assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        st = ch.unary_stream(proto.EXECUTE_TOOL_STREAM, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                             response_deserializer=proto.ExecuteToolResponse.FromString)
        chunks = list(st(_grpc_req("llm.chat", messages=MSGS, max_tokens=7, ignore_eos=True, logprobs=0), timeout=60))
        final = proto.struct_to_dict(chunks[-1].struct_output)
        assert final["usage"]["completion_tokens"] == 7
        assert len(final["logprobs"]["token_ids"]) == len(final["logprobs"]["token_logprobs"]) == 7
        assert final["logprobs"]["top_logprobs"] == [[]] * 7


def test_remote_engine_round_trip_and_final_only_merge():
    llm = AsyncLLM(make_engine())
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="t")
    prompt = [3, 1, 4, 1, 5, 9, 2, 6]
    sp = SamplingParams(max_tokens=6, ignore_eos=True, logprobs=2)

    async def go():
        ltoks, llast = await llm.generate_all(prompt, sp)
        rtoks, rlast = await remote.generate_all(prompt, sp)                       # final_only on the wire
        chunks = [o async for o in remote.generate(prompt, sp)]                    # per step
        finals = [o async for o in remote.generate(prompt, sp, final_only=True)]
        plain = [o async for o in remote.generate(prompt, SamplingParams(max_tokens=3, ignore_eos=True))]
        return ltoks, llast, rtoks, rlast, chunks, finals, plain
    try:
        ltoks, llast, rtoks, rlast, chunks, finals, plain = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert rtoks == ltoks and len(llast.logprobs) == 6
    assert rlast.logprobs == llast.logprobs  # same types after the wire: (float, [(int, float)])
    assert all(len(c.logprobs) == len(c.new_token_ids) for c in chunks)
    assert sum((c.logprobs for c in chunks), []) == llast.logprobs
    assert len(finals) == 1 and finals[0].logprobs == llast.logprobs
    assert all(o.logprobs is None for o in plain)
    assert not srv._final and not srv._final_lp
