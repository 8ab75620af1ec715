"""Qwen3 (``tiny-qwen3``: QK-norm, q_size != hidden) through the engine on the CPU: scheduling
variants equal the plain run, TP = 2 equals TP = 1, the routing switches, the ``chatml`` chat
template and a strict forced tool call through the OpenAI route."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.engine.chat_template import CHATML, LLAMA3, MISTRAL, ChatTemplate, family_for, load_chat_template
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.config import PRESETS
from polykey_service_amd.ops import attention as A
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.service.tool_calls import forced_call, parse_tool_calls, strict_params

CPU = torch.device("cpu")
MODEL = "tiny-qwen3"
SP = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)


def engine(**kw) -> LLMEngine:
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, device="cpu", hip_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(model=MODEL, **base), ParallelState(device=CPU))


# ------------------------------------------------------------------------------------ presets
def test_presets():
    c8, c32, t = PRESETS["qwen3-8b"], PRESETS["qwen3-32b"], PRESETS[MODEL]
    for c in (c8, c32, t):
        assert c.qk_norm and c.head_dim == 128 and c.rope_theta == 1e6 and c.rms_eps == 1e-6 and not c.tie_embeddings
        assert not c.is_moe and c.num_heads % c.num_kv_heads == 0
    assert (c8.vocab_size, c8.hidden_size, c8.intermediate_size, c8.num_layers, c8.num_heads, c8.num_kv_heads) == \
        (151936, 4096, 12288, 36, 32, 8)
    assert (c32.vocab_size, c32.hidden_size, c32.intermediate_size, c32.num_layers, c32.num_heads,
            c32.num_kv_heads) == (151936, 5120, 25600, 64, 64, 8)
    assert c8.max_position == c32.max_position == 40960 and (c8.bos_token_id, c8.eos_token_id) == (151643, 151645)
    assert c32.q_size == 8192 != c32.hidden_size and t.q_size == 2048 != t.hidden_size
    assert t.num_heads // t.num_kv_heads == 4 and t.hidden_size % 1024 == 0
    assert not any(c.qk_norm for n, c in PRESETS.items() if "qwen" not in n)
    # q_size != hidden in the parameter count: the real model holds exactly num_params() values
    m = build_model(t, ParallelState(device=CPU), torch.bfloat16, CPU).init_random(0)
    held = sum(v.numel() for v in m.hf_state_dict().values())
    assert held == t.num_params()
    assert m.layers[0].attn.o.shape == (t.hidden_size, t.q_size)
    # published sizes: 8.19 B and 32.8 B parameters
    assert abs(c8.num_params() / 1e9 - 8.19) < 0.01 and abs(c32.num_params() / 1e9 - 32.76) < 0.05


# ------------------------------------------------------------------------------------- engine
PROMPTS = [[1, 7, 8, 9, 10], [1] + list(range(40, 110)), [1, 300, 301]]


@pytest.fixture(scope="module")
def plain():
    e = engine(prefix_caching=False)
    return e.generate(PROMPTS, SP)


def test_generates_and_the_norm_weights_matter(plain):
    assert [len(o) for o in plain] == [8, 8, 8]
    e = engine(prefix_caching=False)
    assert e.mcfg.qk_norm and e.model.layers[0].attn.q_norm is not None
    e.runner.keep_logits = True
    e.generate([PROMPTS[1]], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    a = e.runner.last_logits.float().clone()
    for layer in e.model.layers:
        layer.attn.q_norm.data.fill_(1.0)
    e.generate([PROMPTS[1]], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    assert float((e.runner.last_logits.float() - a).abs().max()) > 1e-2


def test_chunked_prefill_equals_unchunked(plain):
    e = engine(prefix_caching=False, max_num_batched_tokens=32)  # the 71-token prompt takes three chunks
    assert e.generate(PROMPTS, SP) == plain


def test_prefix_cache_hit_changes_nothing():
    system = [1] + list(range(100, 170))
    first = system + [7, 8, 9]
    later = [system + [11, 12, 13, 14], system + list(range(500, 540)), system[:64] + [5, 6]]
    cold = engine(prefix_caching=False)
    exp = cold.generate([first], SP) + cold.generate(later, SP)
    warm = engine(prefix_caching=True)
    got = warm.generate([first], SP) + warm.generate(later, SP)
    assert warm.scheduler.num_cached_tokens == 3 * 64 and cold.scheduler.num_cached_tokens == 0
    assert got == exp


def test_preemption_and_recompute_change_nothing():
    prompts = [[1] + list(range(50 + 40 * i, 50 + 40 * i + 30)) for i in range(4)]
    sp = SamplingParams(max_tokens=40, temperature=0.0, ignore_eos=True)
    roomy = engine(prefix_caching=False)
    exp = roomy.generate(prompts, sp)
    assert roomy.scheduler.num_preemptions == 0
    tight = engine(prefix_caching=False, num_kv_blocks=7, watermark=0.0)
    got = tight.generate(prompts, sp)
    assert tight.scheduler.num_preemptions > 0
    assert got == exp


def test_fp8_switches_combine(plain):
    for kw in (dict(kv_cache_dtype="fp8"), dict(weight_dtype="fp8"), dict(kv_cache_dtype="fp8", weight_dtype="fp8")):
        e = engine(prefix_caching=False, **kw)
        out = e.generate(PROMPTS, SP)
        assert [len(o) for o in out] == [8, 8, 8] and out == e.generate(PROMPTS, SP)


def test_routing_switches():
    """A QK-norm model never takes the fused QKV-attention launch or the carried collective, and with
    an FP8 cache (no slab writer) neither the folded chain nor slab QKV."""
    from polykey_service_amd.ops import gemm
    FP8 = A.FP8
    md = A.AttnMetadata(num_decode=8, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0, slot_mapping=None)
    k16 = torch.zeros(2, 4, 32, 128, dtype=torch.bfloat16)
    k8 = torch.zeros(2, 4, 32, 128, dtype=torch.uint8).view(FP8)
    for name, qkn in (("tiny-llama-gqa4", False), (MODEL, True)):
        cfg = get_config(name)
        m = build_model(cfg, ParallelState(device=CPU), torch.bfloat16, CPU).init_random(0)
        at = m.layers[0].attn
        nparts = cfg.hidden_size // gemm.PART_COLS
        old = gemm.QKV_ATTN_MIN_KV
        gemm.QKV_ATTN_MIN_KV = 1
        try:
            assert m._qkv_attn_fused_ok(at, 8, nparts, md, k16) == (not qkn)
        finally:
            gemm.QKV_ATTN_MIN_KV = old
        assert at.slabs_ok(md, k16) and at.slabs_ok(md, k8) == (not qkn)
        m.carry_collectives = True
        if qkn:
            assert not m._carry_ok(torch.zeros(8, cfg.hidden_size, dtype=torch.bfloat16), md, k16)
        mdp = A.AttnMetadata(num_decode=2, num_prefill=1, num_prefill_tokens=6, max_prefill_q_len=6, slot_mapping=None)
        assert m._chain_step_ok(md, 8, True) and m._chain_step_ok(md, 8, False) == (not qkn)
        assert m._chain_step_ok(mdp, 8, True) and not m._chain_step_ok(mdp, 8, False) and not m._chain_step_ok(mdp, 65, True)


def test_lora_shapes_follow_q_size():
    from polykey_service_amd.models.lora import proj_dims
    cfg = get_config(MODEL)
    assert [proj_dims(cfg, p) for p in "qko"] == [(1024, 2048), (1024, 512), (2048, 1024)]


# ------------------------------------------------------------------------------------- TP = 2
TP_PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60)), [1, 2]]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_engine(st):
    return LLMEngine(EngineConfig(model=MODEL, max_num_seqs=8, max_num_batched_tokens=128, max_model_len=256,
                                  hip_graphs=False, device="cpu"), st)


def _first_step(eng):
    eng.runner.keep_logits = True
    seqs = [eng.add_request(p, SamplingParams(max_tokens=4)) for p in TP_PROMPTS]
    eng.step()
    logits = eng.runner.last_logits.float().clone()
    while eng.has_unfinished():
        eng.step()
    return logits, [s.output_ids for s in seqs]


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(4)
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=world, ep=1, device="cpu", backend="gloo")
    eng = _tp_engine(st)
    assert eng.model.layers[0].attn.q_norm.shape == (128,) and eng.model.layers[0].attn.nq == 8
    if st.tp_rank == 0:
        logits, toks = _first_step(eng)
        eng.runner.stop_workers()
        torch.save({"logits": logits, "tokens": toks}, out_path)
    else:
        eng.runner.worker_loop()
    destroy_parallel()


def test_tp2_matches_tp1(tmp_path):
    ref_logits, ref_toks = _first_step(_tp_engine(ParallelState()))
    out = str(tmp_path / "tp.pt")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    # bf16 row-parallel partials are rounded per rank before the all-reduce: ~1 bf16 ulp noise
    torch.testing.assert_close(got["logits"], ref_logits, atol=1e-1, rtol=5e-2)
    for row, (g, r) in enumerate(zip(got["tokens"], ref_toks)):
        if g[0] != r[0]:  # only where the reference itself has a near-tie
            lg = ref_logits[row]
            assert lg[g[0]] >= lg.max() - 0.1, (row, g[0], r[0])


# ------------------------------------------------------------------------------ chat template
TOOLS = [{"type": "function", "function": {"name": "get_weather", "description": "d", "strict": True, "parameters": {
    "type": "object", "properties": {"city": {"type": "string", "maxLength": 6}}, "required": ["city"]}}}]


def test_family_selection(tmp_path):
    assert family_for("qwen3-8b") == family_for("Qwen/Qwen3-32B") == family_for("x", qk_norm=True) == CHATML
    assert family_for("llama3-8b") == LLAMA3 and family_for("mixtral-8x7b") == MISTRAL and family_for("x", True) == MISTRAL
    (tmp_path / "tokenizer_config.json").write_text(json.dumps(
        {"chat_template": "{% for m in messages %}<|im_start|>{{ m.role }}\n{{ m.content }}<|im_end|>\n{% endfor %}",
         "eos_token": "<|im_end|>"}))
    t = load_chat_template(str(tmp_path), LLAMA3)
    assert t.family == CHATML and t.render([{"role": "user", "content": "hi"}]) == "<|im_start|>user\nhi<|im_end|>\n"
    assert engine().tokenizer.chat_template.family == CHATML


def test_chatml_rendering():
    t = ChatTemplate(CHATML)
    msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hi"},
            {"role": "assistant", "content": "hello"}, {"role": "user", "content": "weather?"}]
    assert t.render(msgs) == ("<|im_start|>system\nbe brief<|im_end|>\n<|im_start|>user\nhi<|im_end|>\n"
                              "<|im_start|>assistant\nhello<|im_end|>\n<|im_start|>user\nweather?<|im_end|>\n"
                              "<|im_start|>assistant\n")
    assert t.render(msgs[1:2], add_generation_prompt=False) == "<|im_start|>user\nhi<|im_end|>\n"
    # tools live in the system turn; a call and its result render in the family's markup
    call = {"id": "c1", "type": "function", "function": {"name": "get_weather", "arguments": '{"city": "Oslo"}'}}
    text = t.render([{"role": "user", "content": "weather?"}, {"role": "assistant", "content": None, "tool_calls": [call]},
                     {"role": "tool", "tool_call_id": "c1", "content": "4 C"},
                     {"role": "tool", "tool_call_id": "c2", "content": "rain"}], TOOLS)
    assert text.startswith("<|im_start|>system\n# Tools") and "<tools>\n" + json.dumps(
        {"type": "function", "function": {k: TOOLS[0]["function"][k] for k in ("name", "description", "parameters")}}
    ) + "\n</tools>" in text
    assert ('<|im_start|>assistant\n<tool_call>\n{"name": "get_weather", "arguments": {"city": "Oslo"}}\n</tool_call>'
            "<|im_end|>\n") in text
    assert ("<|im_start|>user\n<tool_response>\n4 C\n</tool_response>\n<tool_response>\nrain\n</tool_response>"
            "<|im_end|>\n<|im_start|>assistant\n") in text
    # what the template writes for a call is what parse_tool_calls reads
    body = text.split("<|im_start|>assistant\n")[1].split("<|im_end|>")[0]
    content, calls = parse_tool_calls(body + "<|im_end|>", ["get_weather"])
    assert content == "" and calls[0]["function"] == {"name": "get_weather", "arguments": '{"city": "Oslo"}'}
    assert parse_tool_calls("fine<|im_end|><|endoftext|>")[0] == "fine"


def test_forced_and_strict_calls_in_chatml():
    t = ChatTemplate(CHATML)
    assert t.call_prefix("get_weather") == '<tool_call>\n{"name": "get_weather", "arguments": '
    assert t.call_prefix(None) == '<tool_call>\n{"name": "'
    sp = strict_params(SamplingParams(max_tokens=8), TOOLS, "get_weather", CHATML)
    assert sp.guided_suffix == "}\n</tool_call>"
    from polykey_service_amd.engine import grammar as G
    x = json.dumps({"city": "Oslo"})
    g = G.grammar_for(sp)
    assert g.accepts(x + "}\n</tool_call>") and not g.accepts(x + "}") and not g.accepts(x)
    # the completion of a forced prompt, named and unnamed
    c = forced_call(x + "}\n</tool_call><|im_end|>", "get_weather", ["get_weather"], CHATML)
    assert c["function"] == {"name": "get_weather", "arguments": x}
    c = forced_call('get_weather", "arguments": ' + x + "}\n</tool_call><|im_end|>", None, ["get_weather", "b"], CHATML)
    assert c["function"] == {"name": "get_weather", "arguments": x}
    # the whole text the model would have written round-trips through parse_tool_calls
    _, calls = parse_tool_calls(t.call_prefix("get_weather") + x + "}\n</tool_call><|im_end|>", ["get_weather"])
    assert calls[0]["function"] == {"name": "get_weather", "arguments": x}


def test_strict_forced_tool_call_through_the_openai_route():
    from fastapi.testclient import TestClient

    from polykey_service_amd.adapters.local_llm import attach_local_llm
    from polykey_service_amd.api.openai import create_app
    from polykey_service_amd.config.server_config import ServerConfig
    from polykey_service_amd.service import ToolRouter
    from polykey_service_amd.utils import slog
    r = ToolRouter()
    eng = LLMEngine(EngineConfig(model=MODEL, max_num_seqs=8, max_num_batched_tokens=128, max_model_len=1024,
                                 hip_graphs=False, device="cpu"), ParallelState())
    attach_local_llm(r, ServerConfig(model=MODEL, backend="local"), slog.Logger(open("/dev/null", "w")), engine=eng)
    try:
        client = TestClient(create_app(r))
        assert MODEL in [m["id"] for m in client.get("/v1/models").json()["data"]]
        resp = client.post("/v1/chat/completions", json={
            "model": MODEL, "max_tokens": 96, "temperature": 0.8, "seed": 3, "messages": [{"role": "user", "content": "hey"}],
            "tools": TOOLS, "tool_choice": {"type": "function", "function": {"name": "get_weather"}}})
        assert resp.status_code == 200, resp.json()
        c = resp.json()["choices"][0]
        call, = c["message"]["tool_calls"]
        assert c["finish_reason"] == "tool_calls" and call["function"]["name"] == "get_weather"
        args = json.loads(call["function"]["arguments"])
        assert set(args) == {"city"} and isinstance(args["city"], str) and len(args["city"]) <= 6
    finally:
        r.llm.shutdown()
