"""Prompt logprobs and ``echo`` through the public interfaces on the CPU engine (tiny-llama): both OpenAI
routes, the gRPC struct, every refusal, and a replay of lm-evaluation-harness's ``local-completions``
loglikelihood request."""
import grpc
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.service import logprob_format as lpf
from polykey_service_amd.utils import slog

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
TOOLS = [{"type": "function", "function": {"name": "f", "description": "d",
                                           "parameters": {"type": "object", "properties": {}}}}]
PROMPT = [1, 40, 41, 42, 43, 44, 45, 46, 47]


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


@pytest.fixture(scope="module")
def engine_entries():
    """The engine's own entries for PROMPT with top lists of 2: what every front end must format."""
    e = make_engine()
    s = e.add_request(PROMPT, SamplingParams(max_tokens=1, prompt_logprobs=2, ignore_eos=True))
    outs = []
    while e.has_unfinished():
        outs += e.step()
    return outs[0].prompt_logprobs


def post(client, path, **body):
    r = client.post(path, json={"model": "tiny-llama", **body})
    return r.status_code, r.json()


# -------------------------------------------------------------------------------- OpenAI
def test_completions_prompt_logprobs_field(client, router, engine_entries):
    code, body = post(client, "/v1/completions", prompt=PROMPT, max_tokens=3, ignore_eos=True, temperature=0,
                      prompt_logprobs=2, n=2)
    assert code == 200, body
    tok = router.llm.tokenizer
    assert len(body["choices"]) == 2
    for c in body["choices"]:  # every choice carries the request's list
        pl = c["prompt_logprobs"]
        assert len(pl) == len(PROMPT) and pl[0] is None
        assert pl == lpf.prompt_list(tok, PROMPT, engine_entries)
        for t, item in zip(PROMPT[1:], pl[1:]):
            assert set(item) == {"token_id", "token", "logprob", "rank", "top_logprobs"}
            assert item["token_id"] == t and item["token"] == tok.decode([t], keep_special=True)
            assert item["rank"] >= 1 and item["logprob"] <= 0 and len(item["top_logprobs"]) == 2
            assert all(set(x) == {"token_id", "token", "logprob"} for x in item["top_logprobs"])
            assert (item["rank"] == 1) == (item["top_logprobs"][0]["token_id"] == t)
        assert "logprobs" not in c and not c["text"].startswith(tok.decode(PROMPT))
    assert body["usage"]["prompt_tokens"] == len(PROMPT) and body["usage"]["completion_tokens"] == 6
    plain = post(client, "/v1/completions", prompt=PROMPT, max_tokens=3, ignore_eos=True, temperature=0)[1]
    assert plain["choices"][0]["text"] == body["choices"][0]["text"] and "prompt_logprobs" not in plain["choices"][0]


def test_chat_prompt_logprobs_field(client, router):
    code, body = post(client, "/v1/chat/completions", messages=MSGS, max_tokens=2, ignore_eos=True, prompt_logprobs=0)
    assert code == 200, body
    pl = body["choices"][0]["prompt_logprobs"]
    n = body["usage"]["prompt_tokens"]
    assert len(pl) == n and pl[0] is None and all(x["top_logprobs"] == [] and x["rank"] >= 1 for x in pl[1:])


def test_echo_with_token_ids_and_with_a_string(client, router, engine_entries):
    tok = router.llm.tokenizer
    code, body = post(client, "/v1/completions", prompt=PROMPT, max_tokens=3, ignore_eos=True, temperature=0,
                      echo=True, logprobs=2)
    assert code == 200, body
    c = body["choices"][0]
    plain = post(client, "/v1/completions", prompt=PROMPT, max_tokens=3, ignore_eos=True, temperature=0, logprobs=2)[1]
    p0 = plain["choices"][0]
    assert c["text"] == tok.decode(PROMPT) + p0["text"] and c["finish_reason"] == "length"
    lp = c["logprobs"]
    P = len(PROMPT)
    assert all(len(lp[k]) == P + 3 for k in ("tokens", "token_logprobs", "top_logprobs", "text_offset"))
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert lp["tokens"][:P] == [tok.decode([t], keep_special=True) for t in PROMPT]
    assert lp["token_logprobs"][1:P] == [lpf.finite(e[0]) for e in engine_entries[1:]]
    assert lp["text_offset"][0] == 0
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:k]) for k in range(P + 3)]
    for k in range(1, P):
        want = {}
        for j, v in engine_entries[k][2]:
            want.setdefault(tok.decode([j], keep_special=True), lpf.finite(v))
        assert lp["top_logprobs"][k] == want
    # the completion's part is what the request without echo reports
    assert lp["tokens"][P:] == p0["logprobs"]["tokens"] and lp["token_logprobs"][P:] == p0["logprobs"]["token_logprobs"]
    assert lp["top_logprobs"][P:] == p0["logprobs"]["top_logprobs"]
    assert body["usage"] == plain["usage"] and "prompt_logprobs" not in c
    # a string prompt
    code, body = post(client, "/v1/completions", prompt="hello world", max_tokens=2, ignore_eos=True, temperature=0,
                      echo=True, logprobs=0)
    assert code == 200, body
    ids = tok.encode("hello world")
    c = body["choices"][0]
    assert c["text"].startswith(tok.decode(ids)) and len(c["logprobs"]["tokens"]) == len(ids) + 2
    assert c["logprobs"]["token_logprobs"][0] is None and all(v is not None for v in c["logprobs"]["token_logprobs"][1:])
    assert c["logprobs"]["top_logprobs"][0] is None and c["logprobs"]["top_logprobs"][1:] == [{}] * (len(ids) + 1)


def test_echo_with_max_tokens_zero(client, router):
    tok = router.llm.tokenizer
    code, body = post(client, "/v1/completions", prompt=PROMPT, max_tokens=0, echo=True, logprobs=1)
    assert code == 200, body
    c = body["choices"][0]
    assert c["text"] == tok.decode(PROMPT) and c["finish_reason"] == "length"
    assert len(c["logprobs"]["tokens"]) == len(PROMPT) and c["logprobs"]["token_logprobs"][0] is None
    assert body["usage"]["completion_tokens"] == 0 and body["usage"]["total_tokens"] == len(PROMPT)
    code, body = post(client, "/v1/completions", prompt=PROMPT, max_tokens=0)
    assert code == 400 and "max_tokens" in body["error"]["message"]


def test_echo_without_logprobs_does_no_gpu_work(client, router):
    tok = router.llm.tokenizer
    eng = router.llm.engine
    rows = eng.runner.stats["prompt_lp_rows"]
    code, body = post(client, "/v1/completions", prompt=PROMPT, max_tokens=2, ignore_eos=True, temperature=0, echo=True,
                      n=2)
    assert code == 200, body
    plain = post(client, "/v1/completions", prompt=PROMPT, max_tokens=2, ignore_eos=True, temperature=0, n=2)[1]
    for c, p in zip(body["choices"], plain["choices"]):
        assert c["text"] == tok.decode(PROMPT) + p["text"] and "logprobs" not in c and "prompt_logprobs" not in c
    assert eng.runner.stats["prompt_lp_rows"] == rows and body["usage"] == plain["usage"]


def test_non_finite_values_are_sent_clamped(router):
    tok = router.llm.tokenizer
    ninf = float("-inf")
    entries = [None, (ninf, 7, [(3, -0.5), (4, ninf)]), (-1.0, 1, [])]
    pl = lpf.prompt_list(tok, [1, 5, 6], entries)
    assert pl[0] is None and pl[1]["logprob"] == -9999.0 and pl[1]["rank"] == 7
    assert [x["logprob"] for x in pl[1]["top_logprobs"]] == [-0.5, -9999.0]
    assert lpf.prompt_list(tok, [1, 5, 6], entries, 1)[1]["top_logprobs"] == pl[1]["top_logprobs"][:1]
    sb = lpf.struct_prompt_block([1, 5, 6], entries)
    assert sb == {"token_ids": [1, 5, 6], "token_logprobs": [None, -9999.0, -1.0], "ranks": [None, 7, 1],
                  "top_logprobs": [[], [{"id": 3, "logprob": -0.5}, {"id": 4, "logprob": -9999.0}], []]}
    eb = lpf.echo_block(tok, [1, 5, 6], entries, [9], [(ninf, [(9, ninf)])])
    assert eb["token_logprobs"] == [None, -9999.0, -1.0, -9999.0] and eb["top_logprobs"][0] is None
    assert eb["text_offset"][0] == 0 and len(eb["tokens"]) == 4


def test_openai_refusals_are_400(client):
    comp = dict(prompt=PROMPT, max_tokens=2)
    for bad in (True, "2", 2.5, -1, 21):
        for path, kw in (("/v1/completions", comp), ("/v1/chat/completions", dict(messages=MSGS, max_tokens=2))):
            code, body = post(client, path, prompt_logprobs=bad, **kw)
            assert code == 400 and "prompt_logprobs" in body["error"]["message"], (bad, body)
    for bad in (1, "true", 0.5):
        code, body = post(client, "/v1/completions", echo=bad, **comp)
        assert code == 400 and "'echo' must be a boolean" in body["error"]["message"], (bad, body)
    for path, kw in (("/v1/completions", dict(echo=True, logprobs=1, **comp)),
                     ("/v1/completions", dict(prompt_logprobs=1, **comp)),
                     ("/v1/chat/completions", dict(prompt_logprobs=1, messages=MSGS, max_tokens=2))):
        code, body = post(client, path, stream=True, **kw)
        assert code == 400 and "stream" in body["error"]["message"], body
    code, body = post(client, "/v1/chat/completions", messages=MSGS, max_tokens=2, prompt_logprobs=1, tools=TOOLS)
    assert code == 400 and "'prompt_logprobs'" in body["error"]["message"] and "tools" in body["error"]["message"]
    assert post(client, "/v1/completions", echo=False, **comp)[0] == 200
    assert post(client, "/v1/completions", stream=False, echo=True, **comp)[0] == 200


# ---------------------------------------------------------------------------------- gRPC
def _grpc_req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_grpc_struct_and_refusals(router, engine_entries):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        st = ch.unary_stream(proto.EXECUTE_TOOL_STREAM, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                             response_deserializer=proto.ExecuteToolResponse.FromString)
        kw = dict(prompt_token_ids=PROMPT, max_tokens=3, ignore_eos=True)
        d = proto.struct_to_dict(call(_grpc_req("llm.generate", prompt_logprobs=2, **kw, **{"return": "struct"}),
                                      timeout=60).struct_output)
        pl = d["prompt_logprobs"]
        assert set(pl) == {"token_ids", "token_logprobs", "ranks", "top_logprobs"}
        assert [int(t) for t in pl["token_ids"]] == PROMPT
        assert pl["token_logprobs"][0] is None and pl["ranks"][0] is None and len(pl["top_logprobs"]) == len(PROMPT)
        want = lpf.struct_prompt_block(PROMPT, engine_entries)
        assert pl["token_logprobs"][1:] == pytest.approx(want["token_logprobs"][1:], abs=0)
        assert [int(r) for r in pl["ranks"][1:]] == want["ranks"][1:]
        assert [[int(x["id"]) for x in top] for top in pl["top_logprobs"]] == \
            [[x["id"] for x in top] for top in want["top_logprobs"]]
        plain = proto.struct_to_dict(call(_grpc_req("llm.generate", **kw, **{"return": "struct"}), timeout=60).struct_output)
        assert "prompt_logprobs" not in plain and plain["text"] == d["text"]
        d2 = proto.struct_to_dict(call(_grpc_req("llm.generate", prompt_logprobs=0, n=2, temperature=1.0, seed=3, **kw,
                                                 **{"return": "struct"}), timeout=60).struct_output)
        assert len(d2["choices"]) == 2 and len(d2["prompt_logprobs"]["ranks"]) == len(PROMPT)
        assert all("prompt_logprobs" not in c for c in d2["choices"])
        r = call(_grpc_req("llm.chat", messages=MSGS, max_tokens=2, prompt_logprobs=1, **{"return": "struct"}), timeout=60)
        assert proto.struct_to_dict(r.struct_output)["prompt_logprobs"]["token_logprobs"][0] is None

        def refused(fn, req, *words):
            with pytest.raises(grpc.RpcError) as ei:
                out = fn(req, timeout=20)
                list(out) if fn is st else None
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT, ei.value
            assert all(w in ei.value.details() for w in words), ei.value.details()

        for bad in (True, "2", 2.5, -1, 21):
            refused(call, _grpc_req("llm.generate", prompt="x", prompt_logprobs=bad, **{"return": "struct"}),
                    "prompt_logprobs must be")
        refused(call, _grpc_req("llm.generate", prompt="x", prompt_logprobs=1), "'prompt_logprobs'", "struct")
        refused(call, _grpc_req("llm.chat", messages=MSGS, prompt_logprobs=1, tools=TOOLS, **{"return": "struct"}),
                "'prompt_logprobs'", "tools")
        refused(st, _grpc_req("llm.generate", prompt="x", prompt_logprobs=1, **{"return": "struct"}),
                "'prompt_logprobs'", "ExecuteToolStream")


# ------------------------------------------------------------------ lm-evaluation-harness
def test_lm_eval_local_completions_loglikelihood_replay(client, router, engine_entries):
    """What lm-eval's ``local-completions`` sends for one (context, continuation) pair, and how it reads
    the answer: the continuation's logprobs are ``token_logprobs[ctxlen:-1]``, and it is greedy when every
    continuation token is the first key of its ``top_logprobs`` entry."""
    ctxlen = 4
    payload = {"prompt": PROMPT, "max_tokens": 1, "temperature": 0, "logprobs": 1, "echo": True, "model": "tiny-llama"}
    r = client.post("/v1/completions", json=payload)
    assert r.status_code == 200, r.json()
    lp = r.json()["choices"][0]["logprobs"]
    token_logprobs = lp["token_logprobs"][ctxlen:-1]
    top_logprobs = lp["top_logprobs"][ctxlen:-1]
    tokens = lp["tokens"][ctxlen:-1]
    assert len(token_logprobs) == len(PROMPT) - ctxlen == len(top_logprobs)
    want = [e[0] for e in engine_entries[ctxlen:]]
    assert token_logprobs == want
    loglik = sum(token_logprobs)
    assert loglik == sum(want) and loglik < 0
    is_greedy = all(t == next(iter(top.keys())) for t, top in zip(tokens, top_logprobs))
    assert is_greedy == all(e[1] == 1 for e in engine_entries[ctxlen:])
    assert all(len(top) == 1 for top in top_logprobs)
