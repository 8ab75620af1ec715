"""Guided decoding through the public interfaces on the CPU engine (tiny Llama, byte tokenizer,
reference ops): the OpenAI routes take ``response_format`` json_schema and the ``guided_*``
extensions (streaming too), gRPC takes the same keys, what the compiler refuses is a 400 /
INVALID_ARGUMENT carrying its message, and a strict forced tool call always yields arguments that
parse and conform.  A random model writes none of this by itself."""
import json
import re

import grpc
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig
from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.utils import slog

from tests import grammar_cases as gc
from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
SCHEMA = {"type": "object", "properties": {"city": {"type": "string", "maxLength": 6},
                                           "unit": {"enum": ["celsius", "fahrenheit"]}}, "required": ["city"]}
RF = {"type": "json_schema", "json_schema": {"name": "weather", "schema": SCHEMA}}
BASE = {"model": "tiny-llama", "max_tokens": 96, "temperature": 0.8, "seed": 3}


@pytest.fixture(scope="module")
def router():
    r = ToolRouter()
    eng = LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=1024,
                                 hip_graphs=False, device="cpu"), ParallelState())
    attach_local_llm(r, ServerConfig(model="tiny-llama", backend="local"), slog.Logger(open("/dev/null", "w")), engine=eng)
    yield r
    r.llm.shutdown()


@pytest.fixture(scope="module")
def client(router):
    from fastapi.testclient import TestClient

    from polykey_service_amd.api.openai import create_app
    return TestClient(create_app(router))


def _conforms(text):
    return gc.conforms(SCHEMA, json.loads(text))


def test_response_format_json_schema_on_both_endpoints(client):
    r = client.post("/v1/chat/completions", json={**BASE, "messages": MSGS, "response_format": RF})
    assert r.status_code == 200, r.json()
    c = r.json()["choices"][0]
    assert c["finish_reason"] == "stop" and _conforms(c["message"]["content"]), c
    r = client.post("/v1/completions", json={**BASE, "prompt": "weather:", "response_format": RF})
    assert r.status_code == 200, r.json()
    c = r.json()["choices"][0]
    assert c["finish_reason"] == "stop" and _conforms(c["text"]), c
    # json_object and text stay ignored: the model writes what it likes
    r = client.post("/v1/completions", json={**BASE, "max_tokens": 8, "prompt": "x", "response_format": {"type": "json_object"}})
    assert r.status_code == 200
    with pytest.raises(ValueError):
        json.loads(r.json()["choices"][0]["text"])


def test_guided_extensions_on_both_endpoints(client):
    r = client.post("/v1/chat/completions", json={**BASE, "messages": MSGS, "guided_choice": ["alpha", "beta"]})
    assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] in ("alpha", "beta"), r.json()
    r = client.post("/v1/completions", json={**BASE, "prompt": "id:", "guided_regex": r"[A-F]{3}-\x30[1-9]"})
    assert r.status_code == 200 and re.fullmatch(r"[A-F]{3}-0[1-9]", r.json()["choices"][0]["text"]), r.json()
    r = client.post("/v1/completions", json={**BASE, "prompt": "id:", "guided_json": json.dumps(SCHEMA)})
    assert r.status_code == 200 and _conforms(r.json()["choices"][0]["text"]), r.json()


def test_streaming_chat_is_constrained_too(client):
    with client.stream("POST", "/v1/chat/completions", json={**BASE, "messages": MSGS, "response_format": RF,
                                                             "stream": True}) as r:
        assert r.status_code == 200
        lines = [ln[6:] for ln in r.iter_lines() if ln.startswith("data: ")]
    assert lines[-1] == "[DONE]"
    chunks = [json.loads(ln) for ln in lines[:-1]]
    text = "".join(c["choices"][0]["delta"].get("content") or "" for c in chunks if c.get("choices"))
    assert _conforms(text), text
    assert [c["choices"][0]["finish_reason"] for c in chunks if c.get("choices")][-1] == "stop"


def test_what_the_compiler_refuses_is_a_400_with_its_message(client):
    chat = {**BASE, "messages": MSGS}
    comp = {**BASE, "prompt": "x"}
    for bad, word in (({"guided_regex": "(?<=a)b"}, "lookbehind"), ({"guided_regex": "a$"}, "anchor"),
                      ({"guided_json": {"type": "string", "pattern": "a+"}}, "pattern"),
                      ({"response_format": {"type": "json_schema", "json_schema": {"schema": {"$ref": "#/x"}}}}, "$ref"),
                      ({"response_format": {"type": "json_schema"}}, "json_schema"),
                      ({"guided_choice": []}, "guided_choice"), ({"guided_choice": ["a"], "guided_regex": "a"}, "at most one"),
                      ({"guided_regex": "a", "response_format": RF}, "at most one"),
                      ({"guided_regex": "a", "ignore_eos": True}, "ignore_eos")):
        for url, body in (("/v1/chat/completions", chat), ("/v1/completions", comp)):
            r = client.post(url, json={**body, **bad})
            assert r.status_code == 400 and word in r.json()["error"]["message"], (bad, r.json())


def _grpc_req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_grpc_params(router):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        r = call(_grpc_req("llm.generate", prompt="pick:", max_tokens=32, guided_choice=["left", "right"]), timeout=60)
        assert r.string_output in ("left", "right")
        r = call(_grpc_req("llm.chat", messages=MSGS, max_tokens=96, temperature=0.8, seed=1, guided_json=SCHEMA,
                           **{"return": "struct"}), timeout=60)
        d = proto.struct_to_dict(r.struct_output)
        assert d["finish_reason"] == "stop" and _conforms(d["text"]), d
        r = call(_grpc_req("llm.generate", prompt="n:", max_tokens=32, guided_regex="-?[1-9][0-9]{0,3}"), timeout=60)
        assert re.fullmatch("-?[1-9][0-9]{0,3}", r.string_output)
        for bad, word in (({"guided_regex": "(a)\\1"}, "back-reference"), ({"guided_json": {"type": "integer", "minimum": 1.0}}, "minimum"),
                          ({"guided_choice": "ab"}, "guided_choice")):
            with pytest.raises(grpc.RpcError) as ei:
                call(_grpc_req("llm.generate", prompt="x", **bad), timeout=10)
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT and word in ei.value.details(), bad


def _tool(strict, params=SCHEMA):
    fn = {"name": "get_weather", "description": "d", "parameters": params}
    if strict is not None:
        fn["strict"] = strict
    return [{"type": "function", "function": fn}]


def _forced(client, tools, **kw):
    return client.post("/v1/chat/completions", json={**BASE, "messages": MSGS, "tools": tools,
                                                     "tool_choice": {"type": "function", "function": {"name": "get_weather"}},
                                                     **kw})


def test_a_strict_forced_tool_call_yields_conforming_arguments(client):
    for seed in range(3):
        r = _forced(client, _tool(True), seed=seed)
        assert r.status_code == 200, r.json()
        c = r.json()["choices"][0]
        call, = c["message"]["tool_calls"]
        assert c["finish_reason"] == "tool_calls" and call["function"]["name"] == "get_weather"
        assert _conforms(call["function"]["arguments"]), call
    r = _forced(client, _tool(True, {"type": "object", "properties": {"d": {"type": "string", "format": "date"}}}))
    assert r.status_code == 400 and "format" in r.json()["error"]["message"]


def test_a_non_strict_forced_call_is_unchanged(client):
    got = [_forced(client, _tool(strict)).json()["choices"][0]["message"]["tool_calls"][0]["function"]
           for strict in (None, False)]
    assert got[0] == got[1] and got[0]["name"] == "get_weather"
    with pytest.raises(ValueError):  # the model's own text: no JSON
        json.loads(got[0]["arguments"])


def test_strict_params_and_the_mistral_closing():
    from polykey_service_amd.engine.chat_template import LLAMA3, MISTRAL
    from polykey_service_amd.engine.sequence import SamplingParams
    from polykey_service_amd.service.tool_calls import strict_params
    sp = SamplingParams(max_tokens=8)
    assert strict_params(sp, _tool(None), "get_weather", LLAMA3) is sp
    assert strict_params(sp, _tool(True), "other", LLAMA3) is sp
    a, b = strict_params(sp, _tool(True), "get_weather", LLAMA3), strict_params(sp, _tool(True), "get_weather", MISTRAL)
    assert (a.guided_suffix, b.guided_suffix) == ("}", "}]") and a.guided_json == json.dumps(SCHEMA, sort_keys=True)
    from polykey_service_amd.engine import grammar as G
    x = json.dumps({"city": "Oslo", "unit": "celsius"})
    assert G.grammar_for(b).accepts(x + "}]") and not G.grammar_for(b).accepts(x) and G.grammar_for(a).accepts(x + "}")
