"""Speculative decoding through the public interfaces on the CPU engine (tiny Llama, reference ops):
``speculative`` is accepted as a boolean and rejected otherwise by both OpenAI routes and both gRPC
tools, the three Prometheus counters move, a request's summary carries ``spec_drafted`` /
``spec_accepted`` only on an engine with speculation configured, and the remote-engine wire keeps
the field."""
import asyncio
import threading

import grpc
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig
from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.engine.async_llm import AsyncLLM
from polykey_service_amd.engine.remote import EngineServer, RemoteEngine, _params_dict
from polykey_service_amd.engine.sequence import SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.utils import slog
from polykey_service_amd.utils.metrics import Metrics

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
PROMPT = [1, 4, 5, 6, 4, 5, 6, 4, 5]


class Replay:
    """Drafts what a request without speculation emitted for the same prompt (recorded below);
    nothing for prompts it has not seen."""

    def __init__(self):
        self.rec = {}
        self.asked = []

    def propose(self, seq, k):
        self.asked.append(seq.params.speculative)
        n = len(seq.output_ids)
        return self.rec.get(tuple(seq.prompt_ids), [])[n:n + k]


def make_engine(speculative="ngram"):
    return LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                                  hip_graphs=False, device="cpu", dtype="float32", speculative=speculative),
                     ParallelState())


@pytest.fixture(scope="module")
def metrics():
    return Metrics()


@pytest.fixture(scope="module")
def router(metrics):
    r = ToolRouter()
    eng = make_engine()
    eng.proposer = Replay()
    attach_local_llm(r, ServerConfig(model="tiny-llama", backend="local", speculative="ngram"),
                     slog.Logger(open("/dev/null", "w")), engine=eng)
    r.llm.metrics = metrics
    yield r
    r.llm.shutdown()


@pytest.fixture(scope="module")
def client(router):
    from fastapi.testclient import TestClient

    from polykey_service_amd.api.openai import create_app
    return TestClient(create_app(router))


def _call(ch):
    return ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                          response_deserializer=proto.ExecuteToolResponse.FromString)


def _req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_openai_routes_accept_a_boolean_and_reject_anything_else(client):
    chat = {"model": "tiny-llama", "max_tokens": 3, "messages": MSGS, "temperature": 0}
    comp = {"model": "tiny-llama", "max_tokens": 3, "prompt": PROMPT, "temperature": 0}
    texts = {}
    for v in (True, False, None):
        r = client.post("/v1/chat/completions", json={**chat, "speculative": v})
        assert r.status_code == 200, r.json()
        texts[("chat", v)] = r.json()["choices"][0]["message"]["content"]
        r = client.post("/v1/completions", json={**comp, "speculative": v})
        assert r.status_code == 200, r.json()
        texts[("comp", v)] = r.json()["choices"][0]["text"]
    assert len({texts[("chat", v)] for v in (True, False, None)}) == 1
    assert len({texts[("comp", v)] for v in (True, False, None)}) == 1
    for bad in (1, 0, "yes", "false", 0.5, [True], {"on": True}):
        assert client.post("/v1/chat/completions", json={**chat, "speculative": bad}).status_code == 400, bad
        assert client.post("/v1/completions", json={**comp, "speculative": bad}).status_code == 400, bad


def test_grpc_tools_counters_and_summary(router, metrics):
    """llm.generate without drafts records the continuation; the same prompt then drafts it: fewer
    steps, the same tokens, counters and the summary's spec_* keys move; speculative=false does not
    draft; a non-boolean is INVALID_ARGUMENT on both tools."""
    eng = router.llm.engine
    replay = eng.proposer
    replay.asked.clear()
    val = metrics.registry.get_sample_value
    names = ("polykey_engine_spec_steps_total", "polykey_engine_spec_draft_tokens_total",
             "polykey_engine_spec_accepted_tokens_total")
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = _call(ch)
        base = dict(prompt_token_ids=PROMPT, max_tokens=12, ignore_eos=True, return_token_ids=True, **{"return": "struct"})
        first = proto.struct_to_dict(call(_req("llm.generate", **base, speculative=False), timeout=60).struct_output)
        toks = [int(t) for t in first["token_ids"]]
        assert len(toks) == 12
        assert first["metrics"]["spec_drafted"] == 0 and first["metrics"]["spec_accepted"] == 0
        assert eng.spec_steps == 0 and not replay.asked   # never asked for a request that opted out
        before = [val(n) or 0.0 for n in names]
        replay.rec[tuple(PROMPT)] = toks
        steps0 = eng.step_count
        second = proto.struct_to_dict(call(_req("llm.generate", **base), timeout=60).struct_output)
        assert [int(t) for t in second["token_ids"]] == toks
        assert eng.step_count - steps0 < 12
        m = second["metrics"]
        assert m["spec_drafted"] == m["spec_accepted"] > 0
        after = [val(n) for n in names]
        assert all(a is not None and a > b for a, b in zip(after, before)), (before, after)
        assert after[1] - before[1] == m["spec_drafted"] and after[2] - before[2] == m["spec_accepted"]
        assert replay.asked and set(replay.asked) == {None}
        third = proto.struct_to_dict(call(_req("llm.generate", **base, speculative=True), timeout=60).struct_output)
        assert [int(t) for t in third["token_ids"]] == toks and True in replay.asked
        r = call(_req("llm.chat", messages=MSGS, max_tokens=3, speculative=False, **{"return": "struct"}), timeout=60)
        assert "spec_drafted" in proto.struct_to_dict(r.struct_output)["metrics"]
        for tool, kw in (("llm.generate", dict(prompt="x")), ("llm.chat", dict(messages=MSGS))):
            for bad in (1.0, "true", [True]):
                with pytest.raises(grpc.RpcError) as ei:
                    call(_req(tool, speculative=bad, **kw), timeout=10)
                assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT, (tool, bad)


def test_summary_without_speculation_has_no_spec_keys():
    r = ToolRouter()
    attach_local_llm(r, ServerConfig(model="tiny-llama", backend="local"), slog.Logger(open("/dev/null", "w")),
                     engine=make_engine(None))
    m = Metrics()
    r.llm.metrics = m
    try:
        with ServerThread(r) as s, grpc.insecure_channel(s.addr) as ch:
            out = proto.struct_to_dict(_call(ch)(_req("llm.generate", prompt_token_ids=PROMPT, max_tokens=4,
                                                      ignore_eos=True, speculative=True, **{"return": "struct"}),
                                                 timeout=60).struct_output)
    finally:
        r.llm.shutdown()
    assert out["usage"]["completion_tokens"] == 4
    assert not any(k.startswith("spec_") for k in out["metrics"]), out["metrics"]
    assert (m.registry.get_sample_value("polykey_engine_spec_steps_total") or 0.0) == 0.0


def test_remote_engine_wire_carries_the_field():
    assert _params_dict(SamplingParams(speculative=False))["speculative"] is False
    assert _params_dict(SamplingParams())["speculative"] is None
    eng = make_engine()
    replay = eng.proposer = Replay()
    llm = AsyncLLM(eng)
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="t")

    async def go():
        off = await remote.generate_all(PROMPT, SamplingParams(max_tokens=8, ignore_eos=True, speculative=False))
        asked = list(replay.asked)
        replay.rec[tuple(PROMPT)] = list(off[0])
        on = await remote.generate_all(PROMPT, SamplingParams(max_tokens=8, ignore_eos=True))
        return off, asked, on
    try:
        (off, _), asked, (on, last) = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert asked == [] and replay.asked and off == on and len(on) == 8
    assert last.metrics["spec_accepted"] > 0
