"""LoRA adapters through the public interfaces on the CPU engine (tiny Llama, reference ops): both
OpenAI routes and both gRPC tools pick an adapter by its name, ``/v1/models`` lists adapters under
their base model, an unknown adapter is the existing 404 / NOT_FOUND, and an adapter named like a
served model is refused at start-up."""
import grpc
import pytest

from polykey_service_amd import proto
from polykey_service_amd.adapters.local_llm import attach_local_llm
from polykey_service_amd.config.server_config import ServerConfig, load_server_config, parse_lora_modules
from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.models import get_config
from polykey_service_amd.models.lora import LoraAdapter
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service import ToolRouter
from polykey_service_amd.utils import slog

from tests.helpers import ServerThread

MSGS = [{"role": "user", "content": "hey"}]
IDS = [1, 5, 6, 7]


def make_engine(names=("fr", "de")):
    cfg = get_config("tiny-llama")
    mods = tuple((n, LoraAdapter.random(cfg, rank=8, alpha=16, seed=i + 1, b_std=0.08)) for i, n in enumerate(names))
    return LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512,
                                  hip_graphs=False, device="cpu", lora_modules=mods), ParallelState())


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


def test_server_config_flags_and_env(tmp_path):
    assert load_server_config([], {}).lora_modules == "" and load_server_config([], {}).max_lora_rank == 64
    sc = load_server_config(["--lora-modules", "fr=/a/fr,de=/a/de", "--max-lora-rank", "32"], {})
    assert parse_lora_modules(sc.lora_modules) == (("fr", "/a/fr"), ("de", "/a/de")) and sc.max_lora_rank == 32
    ec = EngineConfig.from_server_config(sc)
    assert ec.lora_modules == (("fr", "/a/fr"), ("de", "/a/de")) and ec.max_lora_rank == 32
    sc = load_server_config([], {"POLYKEY_LORA_MODULES": "x=/p", "POLYKEY_MAX_LORA_RANK": "16"})
    assert parse_lora_modules(sc.lora_modules) == (("x", "/p"),) and sc.max_lora_rank == 16
    for bad in ("fr", "fr=", "=p", "a=/p,a=/q"):
        with pytest.raises(ValueError, match="lora_modules"):
            load_server_config(["--lora-modules", bad], {})
    assert EngineConfig.from_server_config(load_server_config([], {})).lora_modules == ()


def test_models_route_lists_adapters_under_their_base(client):
    data = {m["id"]: m for m in client.get("/v1/models").json()["data"]}
    assert set(data) == {"tiny-llama", "fr", "de"}
    assert "parent" not in data["tiny-llama"]
    assert data["fr"]["parent"] == data["de"]["parent"] == "tiny-llama"


def test_both_openai_routes_pick_the_adapter_by_model_name(client):
    comp = lambda model: client.post("/v1/completions", json={"model": model, "prompt": IDS, "max_tokens": 8,
                                                              "ignore_eos": True, "temperature": 0})
    out = {}
    for m in ("tiny-llama", "fr", "de"):
        r = comp(m)
        assert r.status_code == 200, r.json()
        assert r.json()["model"] == m
        out[m] = r.json()["choices"][0]["text"]
    assert len({out["tiny-llama"], out["fr"], out["de"]}) == 3
    assert comp("fr").json()["choices"][0]["text"] == out["fr"]
    chat = lambda model: client.post("/v1/chat/completions", json={"model": model, "messages": MSGS, "max_tokens": 8,
                                                                   "ignore_eos": True, "temperature": 0})
    texts = {m: chat(m).json()["choices"][0]["message"]["content"] for m in ("tiny-llama", "fr", "de")}
    assert len(set(texts.values())) == 3
    # an unknown name is the existing 404
    r = comp("es")
    assert r.status_code == 404 and "es" in r.json()["error"]["message"]
    assert chat("es").status_code == 404


def _req(tool, **params):
    r = proto.ExecuteToolRequest(tool_name=tool)
    r.parameters.update(params)
    return r


def test_both_grpc_tools_route_adapters(router):
    with ServerThread(router) as s, grpc.insecure_channel(s.addr) as ch:
        call = ch.unary_unary(proto.EXECUTE_TOOL, request_serializer=proto.ExecuteToolRequest.SerializeToString,
                              response_deserializer=proto.ExecuteToolResponse.FromString)
        gen = lambda tool, **kw: proto.struct_to_dict(call(_req(tool, prompt_token_ids=IDS, max_tokens=8,
                                                                ignore_eos=True, return_token_ids=True,
                                                                **{"return": "struct"}, **kw), timeout=60).struct_output)
        base = gen("llm.generate")
        fr = gen("llm.generate:fr")
        de = gen("llm.generate", lora="de")
        assert "lora" not in base and base["model"] == "tiny-llama"
        assert fr["lora"] == "fr" and fr["model"] == "fr" and de["lora"] == "de" and de["model"] == "tiny-llama"
        assert len({tuple(base["token_ids"]), tuple(fr["token_ids"]), tuple(de["token_ids"])}) == 3
        assert gen("llm.generate", lora="fr")["token_ids"] == fr["token_ids"]
        assert gen("llm.generate:de")["token_ids"] == de["token_ids"]
        chat = lambda tool, **kw: proto.struct_to_dict(call(_req(tool, messages=MSGS, max_tokens=6, ignore_eos=True,
                                                                 **{"return": "struct"}, **kw), timeout=60).struct_output)
        c_base, c_fr = chat("llm.chat"), chat("llm.chat:fr")
        assert c_fr["lora"] == "fr" and "lora" not in c_base and c_fr["text"] != c_base["text"]
        assert chat("llm.chat", lora="fr")["text"] == c_fr["text"]
        for bad in (_req("llm.generate:es", prompt_token_ids=IDS), _req("llm.generate", prompt_token_ids=IDS, lora="es"),
                    _req("llm.chat:es", messages=MSGS), _req("llm.chat", messages=MSGS, lora="es")):
            with pytest.raises(grpc.RpcError) as ei:
                call(bad, timeout=10)
            assert ei.value.code() == grpc.StatusCode.NOT_FOUND


def test_an_adapter_named_like_a_served_model_is_refused_at_start_up():
    r = ToolRouter()
    eng = make_engine(names=("tiny-llama",))
    with pytest.raises(ValueError, match="collides with a served model"):
        attach_local_llm(r, ServerConfig(model="tiny-llama", backend="local"), slog.Logger(open("/dev/null", "w")),
                         engine=eng)
