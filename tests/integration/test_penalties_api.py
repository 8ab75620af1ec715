"""Sampling penalties and logit_bias through the public interfaces on the CPU engine (tiny Llama,
reference ops): both OpenAI routes honour ``logit_bias`` and ``frequency_penalty``, bad values
are 400 / INVALID_ARGUMENT, the gRPC ``llm.generate`` Struct form works, penalties combine with
function tools, and the remote-engine wire keeps the parameters."""
import asyncio
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
PROMPT = [1, 4, 5]
FORCED, OTHER = 90, 61


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


def _ids(body):
    """Token ids of a completions answer that asked for ``logprobs: 0`` on a token-id prompt."""
    return body["choices"][0]["logprobs"]["tokens"]


def test_completions_route_honours_bias_and_frequency_penalty(client, router):
    tok = router.llm.tokenizer
    a, b = lpf._tok(tok, FORCED), lpf._tok(tok, OTHER)
    assert a != b
    base = {"model": "tiny-llama", "prompt": PROMPT, "max_tokens": 10, "ignore_eos": True, "temperature": 0,
            "logprobs": 0}
    plain = client.post("/v1/completions", json=base)
    assert plain.status_code == 200, plain.json()
    bias = {str(FORCED): 100, str(OTHER): 90}
    r = client.post("/v1/completions", json={**base, "logit_bias": bias})
    assert r.status_code == 200, r.json()
    assert _ids(r.json()) == [a] * 10               # 10 ahead of the runner-up at every step
    # each repeat costs the favourite 2 (and 2 once): after five it falls behind the runner-up
    pen = client.post("/v1/completions", json={**base, "logit_bias": bias, "frequency_penalty": 2,
                                               "presence_penalty": 2})
    assert pen.status_code == 200, pen.json()
    assert set(_ids(pen.json())) == {a, b} and _ids(pen.json())[0] == a
    assert _ids(client.post("/v1/completions", json=base).json()) == _ids(plain.json())


def test_chat_route_honours_bias_and_penalties(client, router):
    tok = router.llm.tokenizer
    base = {"model": "tiny-llama", "max_tokens": 6, "ignore_eos": True, "temperature": 0, "messages": MSGS}
    plain = client.post("/v1/chat/completions", json=base).json()
    forced = client.post("/v1/chat/completions", json={**base, "logit_bias": {str(FORCED): 100}})
    assert forced.status_code == 200, forced.json()
    assert forced.json()["choices"][0]["message"]["content"] == tok.decode([FORCED] * 6)
    pen = client.post("/v1/chat/completions", json={**base, "max_tokens": 10, "frequency_penalty": 2.0,
                                                    "presence_penalty": 2.0, "logprobs": True,
                                                    "logit_bias": {str(FORCED): 100, str(OTHER): 90}})
    assert pen.status_code == 200, pen.json()
    toks = [it["token"] for it in pen.json()["choices"][0]["logprobs"]["content"]]
    assert set(toks) == {lpf._tok(tok, FORCED), lpf._tok(tok, OTHER)} and toks[0] == lpf._tok(tok, FORCED)
    assert client.post("/v1/chat/completions", json=base).json()["choices"][0]["message"] == \
        plain["choices"][0]["message"]


def test_bad_values_are_400(client):
    chat = {"model": "tiny-llama", "max_tokens": 2, "messages": MSGS}
    comp = {"model": "tiny-llama", "max_tokens": 2, "prompt": PROMPT}
    for bad in ({"frequency_penalty": 2.5}, {"presence_penalty": -3}, {"repetition_penalty": 0},
                {"repetition_penalty": -1.5}, {"logit_bias": {"5": 101}}, {"logit_bias": {"x": 1}},
                {"logit_bias": {str(i): 1 for i in range(301)}}, {"logit_bias": {"-4": 1}},
                {"frequency_penalty": "a lot"}):
        assert client.post("/v1/chat/completions", json={**chat, **bad}).status_code == 400, bad
        assert client.post("/v1/completions", json={**comp, **bad}).status_code == 400, bad
    ok = {"frequency_penalty": -2, "presence_penalty": 2, "repetition_penalty": 0.5, "logit_bias": {"5": -100}}
    assert client.post("/v1/chat/completions", json={**chat, **ok}).status_code == 200
    assert client.post("/v1/completions", json={**comp, **ok}).status_code == 200


def test_penalties_combine_with_function_tools(client):
    tools = [{"type": "function", "function": {"name": "f", "description": "d",
                                               "parameters": {"type": "object", "properties": {}}}}]
    r = client.post("/v1/chat/completions", json={"model": "tiny-llama", "max_tokens": 4, "messages": MSGS,
                                                  "tools": tools, "frequency_penalty": 0.5,
                                                  "logit_bias": {str(FORCED): 5}})
    assert r.status_code == 200, r.json()


def _grpc_req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_grpc_generate_takes_a_struct_bias_and_rejects_bad_values(router):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        r = call(_grpc_req("llm.generate", prompt_token_ids=PROMPT, max_tokens=5, ignore_eos=True,
                           logit_bias={str(FORCED): 100.0}, return_token_ids=True, **{"return": "struct"}), timeout=60)
        d = proto.struct_to_dict(r.struct_output)
        assert [int(t) for t in d["token_ids"]] == [FORCED] * 5
        r = call(_grpc_req("llm.generate", prompt_token_ids=PROMPT, max_tokens=5, ignore_eos=True,
                           repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5,
                           return_token_ids=True, **{"return": "struct"}), timeout=60)
        assert len(proto.struct_to_dict(r.struct_output)["token_ids"]) == 5
        for bad in ({"frequency_penalty": 3.0}, {"repetition_penalty": 0.0}, {"logit_bias": {"7": 1000.0}},
                    {"logit_bias": {"seven": 1.0}}):
            with pytest.raises(grpc.RpcError) as ei:
                call(_grpc_req("llm.generate", prompt="x", **bad), timeout=10)
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT, bad


def test_remote_engine_round_trip():
    llm = AsyncLLM(make_engine())
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="t")
    sp = SamplingParams.from_dict({"max_tokens": 5, "ignore_eos": True, "logit_bias": {str(FORCED): 100},
                                   "repetition_penalty": 1.1})
    sp2 = SamplingParams(max_tokens=5, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5,
                         presence_penalty=0.5)

    async def go():
        return (await remote.generate_all(PROMPT, sp), await llm.generate_all(PROMPT, sp2),
                await remote.generate_all(PROMPT, sp2))
    try:
        (forced, _), (local, _), (far, _) = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert forced == [FORCED] * 5 and far == local and len(far) == 5
