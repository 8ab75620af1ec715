"""An engine started with ``kv_cache_dtype=fp8`` behind the public interfaces (CPU engine, tiny
Llama, reference ops): the server configuration reaches the engine, ``/v1/chat/completions`` and
gRPC ``ExecuteTool`` (``llm.generate``) answer, and the answers are those of the engine itself."""
import grpc
import pytest
import torch

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import load_server_config
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.utils import slog

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
PROMPT = [1, 4, 5]


def make_engine(sc):
    import dataclasses
    ecfg = dataclasses.replace(EngineConfig.from_server_config(sc), max_num_seqs=8, max_num_batched_tokens=128,
                               max_model_len=512, hip_graphs=False, device="cpu")
    return LLMEngine(ecfg, ParallelState())


@pytest.fixture(scope="module")
def router():
    sc = load_server_config(["--model", "tiny-llama", "--backend", "local", "--kv-cache-dtype", "fp8"], {})
    eng = make_engine(sc)
    assert eng.cfg.kv_cache_dtype == "fp8" and eng.runner.kv_caches[0][0].dtype == torch.float8_e4m3fn
    r = ToolRouter()
    attach_local_llm(r, sc, slog.Logger(open("/dev/null", "w")), engine=eng)
    yield r
    r.llm.shutdown()


def test_chat_completions_on_an_fp8_engine(router):
    from fastapi.testclient import TestClient

    from polykey_service_amd.api.openai import create_app
    client = TestClient(create_app(router))
    body = {"model": "tiny-llama", "max_tokens": 6, "ignore_eos": True, "temperature": 0, "messages": MSGS}
    a = client.post("/v1/chat/completions", json=body)
    assert a.status_code == 200, a.json()
    assert a.json()["usage"]["completion_tokens"] == 6
    assert client.post("/v1/chat/completions", json=body).json()["choices"][0]["message"] == \
        a.json()["choices"][0]["message"]


def test_grpc_execute_tool_on_an_fp8_engine(router):
    sc = load_server_config(["--model", "tiny-llama", "--kv-cache-dtype", "fp8_e4m3"], {})
    want = make_engine(sc).generate([PROMPT], SamplingParams(max_tokens=5, temperature=0.0, ignore_eos=True))[0]
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        req = proto.ExecuteToolRequest(tool_name="llm.generate")
        req.parameters.update({"prompt_token_ids": PROMPT, "max_tokens": 5, "ignore_eos": True, "temperature": 0.0,
                               "return_token_ids": True, "return": "struct"})
        r = call(req, timeout=60)
        assert [int(t) for t in proto.struct_to_dict(r.struct_output)["token_ids"]] == want
