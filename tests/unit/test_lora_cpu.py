"""LoRA adapters on the CPU engine: the PEFT directory format (round trip, rejections), the model
with an adapter against the same model with merged weights, engine construction and request
validation, the prefix cache's adapter-aware salt, and preemption by recompute."""
import copy
import json
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.lora import TARGETS, LoraAdapter, LoraState, lora_bytes, proj_dims
from polykey_service_amd.ops import gemm
from polykey_service_amd.parallel.state import ParallelState

CPU = torch.device("cpu")
NAME = "tiny-llama"
CFG = get_config(NAME)


def adapter(seed=1, rank=8, **kw):
    return LoraAdapter.random(CFG, rank=rank, alpha=16, seed=seed, b_std=kw.pop("b_std", 0.05), **kw)


def engine(lora_modules=(), model=None, name=NAME, st=None, **kw) -> LLMEngine:
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, device="cpu", hip_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(model=name, lora_modules=tuple(lora_modules), **base),
                     st or ParallelState(device=CPU), model=model)


# ------------------------------------------------------------------------------- PEFT format
def test_save_load_round_trip(tmp_path):
    a = LoraAdapter.random(CFG, rank=6, alpha=24, seed=3, targets=("q", "v", "down"), b_std=0.1)
    a.save(str(tmp_path / "a"))
    ac = json.load(open(tmp_path / "a" / "adapter_config.json"))
    assert ac["r"] == 6 and ac["lora_alpha"] == 24 and sorted(ac["target_modules"]) == ["down_proj", "q_proj", "v_proj"]
    sd = load_file(str(tmp_path / "a" / "adapter_model.safetensors"))
    assert "base_model.model.model.layers.1.self_attn.q_proj.lora_A.weight" in sd
    assert "base_model.model.model.layers.0.mlp.down_proj.lora_B.weight" in sd
    assert len(sd) == 2 * 3 * CFG.num_layers
    b = LoraAdapter.load(str(tmp_path / "a"), CFG)
    assert (b.rank, b.alpha, b.scale, b.targets) == (6, 24.0, 4.0, ("q", "v", "down"))
    assert set(b.tensors) == set(a.tensors)
    for k, (A, B) in a.tensors.items():
        assert torch.equal(A, b.tensors[k][0]) and torch.equal(B, b.tensors[k][1])
        K, N = proj_dims(CFG, k[1])
        assert A.shape == (6, K) and B.shape == (N, 6)
    # rsLoRA scale
    ac["use_rslora"] = True
    json.dump(ac, open(tmp_path / "a" / "adapter_config.json", "w"))
    assert LoraAdapter.load(str(tmp_path / "a"), CFG).scale == pytest.approx(24 / 6 ** 0.5)


def _saved(tmp_path, edit_cfg=None, edit_sd=None, **kw):
    d = str(tmp_path / "ad")
    adapter(**kw).save(d)
    if edit_cfg:
        p = os.path.join(d, "adapter_config.json")
        ac = json.load(open(p))
        edit_cfg(ac)
        json.dump(ac, open(p, "w"))
    if edit_sd:
        p = os.path.join(d, "adapter_model.safetensors")
        sd = load_file(p)
        edit_sd(sd)
        save_file(sd, p)
    return d


@pytest.mark.parametrize("what,edit,match", [
    ("dora", lambda ac: ac.update(use_dora=True), "use_dora"),
    ("bias", lambda ac: ac.update(bias="all"), "bias="),
    ("rank_pattern", lambda ac: ac.update(rank_pattern={"q_proj": 4}), "rank_pattern"),
    ("alpha_pattern", lambda ac: ac.update(alpha_pattern={"q_proj": 4}), "alpha_pattern"),
    ("modules_to_save", lambda ac: ac.update(modules_to_save=["lm_head"]), "modules_to_save"),
    ("target", lambda ac: ac["target_modules"].append("embed_tokens"), "embed_tokens"),
    ("rank", lambda ac: ac.update(r=65), r"r=65.*max_lora_rank=64"),
])
def test_config_rejections_name_the_key(tmp_path, what, edit, match):
    with pytest.raises(ValueError, match=match):
        LoraAdapter.load(_saved(tmp_path, edit_cfg=edit), CFG)


def test_tensor_rejections_name_the_key(tmp_path):
    key = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    with pytest.raises(ValueError, match=r"q_proj\.lora_A\.weight.*shape"):
        LoraAdapter.load(_saved(tmp_path, edit_sd=lambda sd: sd.update({key: sd[key][:, :-8].contiguous()})), CFG)
    head = "base_model.model.lm_head.lora_A.weight"
    with pytest.raises(ValueError, match="lm_head"):
        LoraAdapter.load(_saved(tmp_path, edit_sd=lambda sd: sd.update({head: torch.zeros(8, 512)})), CFG)
    deep = "base_model.model.model.layers.7.self_attn.q_proj.lora_A.weight"
    with pytest.raises(ValueError, match="layer 7"):
        LoraAdapter.load(_saved(tmp_path, edit_sd=lambda sd: sd.update({deep: sd[key].clone()})), CFG)
    with pytest.raises(ValueError, match="max_lora_rank=4"):
        LoraAdapter.load(_saved(tmp_path), CFG, max_rank=4)


# ------------------------------------------------------------------------------- the function
def test_store_layout_and_bytes():
    X, Y = adapter(1, 8), adapter(2, 3, targets=("q", "up"))
    st = LoraState(CFG, [("X", X), ("Y", Y)], 64, 16, CPU)
    assert st.nbytes == lora_bytes(CFG, 2, 64) == 2 * 64 * sum(sum(proj_dims(CFG, p)) for p in TARGETS) * 2 * 2
    l0 = st.layers[0]
    q, kv, I = CFG.q_size, CFG.kv_size, CFG.intermediate_size
    assert l0["qkv"].A.shape == (2, 192, 512) and l0["qkv"].B.shape == (2, q + 2 * kv, 64)
    assert (l0["qkv"].seg.b0, l0["qkv"].seg.b1) == (q, q + kv)
    # every sub-projection keeps its own A and B, zero-padded; an untargeted one is exactly zero
    assert torch.equal(l0["qkv"].A[0, 64:72], X.tensors[(0, "k")][0]) and not l0["qkv"].A[0, 72:128].any()
    assert torch.equal(l0["qkv"].B[0, q:q + kv, :8], X.tensors[(0, "k")][1])
    assert not l0["qkv"].A[1, 64:].any() and not l0["qkv"].B[1, q:].any()        # Y: q only
    assert torch.equal(l0["qkv"].A[1, :3], Y.tensors[(0, "q")][0])
    # gate_up: B rows interleaved by 16 like the weight
    g, u = gemm.deinterleave_gate_up(l0["gate_up"].B[0])
    assert torch.equal(g[:, :8], X.tensors[(0, "gate")][1]) and torch.equal(u[:, :8], X.tensors[(0, "up")][1])
    assert l0["gate_up"].seg.il == 16 and l0["gate_up"].A.shape == (2, 128, 512)
    assert st.scale.tolist() == [2.0, pytest.approx(16 / 3)] and st.ranks.tolist() == [8, 3]
    # a module nobody targets has no launches at all
    only_q = LoraState(CFG, [("Y", adapter(2, 3, targets=("q",)))], 64, 16, CPU)
    assert only_q.layers[0]["o"] is None and only_q.layers[0]["down"] is None and only_q.layers[0]["gate_up"] is None


def test_adapter_model_against_merged_weights_in_float32():
    """The engine with adapter X on a float32 model against a float32 engine whose weights are
    W + s B A.  They differ by the one bf16 rounding of t and by fp32 summation order (sums of at
    most 1024 terms): within 1e-3 of the logits' rms."""
    base = build_model(CFG, ParallelState(device=CPU), torch.float32, CPU).init_random(4)
    X = adapter(1, 8, b_std=0.08)
    merged = copy.deepcopy(base)
    for i, layer in enumerate(merged.layers):
        d = {p: X.merged_delta(i, p) for p in TARGETS}
        layer.attn.qkv.data += torch.cat([d["q"], d["k"], d["v"]])
        layer.attn.o.data += d["o"]
        layer.mlp.gate_up.data += gemm.interleave_gate_up(d["gate"], d["up"])
        layer.mlp.down.data += d["down"]
    prompts = [[1] + list(range(5, 45)), [1, 9, 8]]
    logits = {}
    for tag, model, mods, lora in (("adapter", base, (("X", X),), "X"), ("merged", merged, (), None),
                                   ("base", copy.deepcopy(base), (), None)):
        e = engine(mods, model=model, dtype="float32")
        e.runner.keep_logits = True
        e.generate(prompts, SamplingParams(max_tokens=1, lora=lora))
        logits[tag] = e.runner.last_logits.double().clone()
    rms = lambda t: float(t.pow(2).mean().sqrt())
    assert rms(logits["adapter"] - logits["base"]) > 0.3 * rms(logits["base"])   # the adapter matters
    assert rms(logits["adapter"] - logits["merged"]) <= 1e-3 * rms(logits["merged"])


# ------------------------------------------------------------------------------- the engine
def test_engine_construction_errors_name_the_setting():
    mods = (("X", adapter()),)
    with pytest.raises(ValueError, match=r"LoRA.*MoE.*follow-up"):
        engine(mods, name="tiny-mixtral")
    with pytest.raises(ValueError, match=r"LoRA.*tp=2.*follow-up"):
        engine(mods, st=ParallelState(world_size=2, tp_size=2, device=CPU))
    with pytest.raises(ValueError, match=r"LoRA.*ep=2.*follow-up"):
        engine(mods, st=ParallelState(world_size=2, ep_size=2, device=CPU))
    with pytest.raises(ValueError, match=r"LoRA.*weight_dtype=fp8.*follow-up"):
        engine(mods, weight_dtype="fp8")
    with pytest.raises(ValueError, match="max_lora_rank=4"):
        engine(mods, max_lora_rank=4)
    with pytest.raises(ValueError, match="unique"):
        engine(mods + mods)
    with pytest.raises(ValueError, match="at most 32"):
        engine(tuple((f"a{i}", mods[0][1]) for i in range(33)))
    # adapters combine with an FP8 KV cache
    e = engine(mods, kv_cache_dtype="fp8")
    assert len(e.generate([[1, 5, 6]], SamplingParams(max_tokens=3, lora="X"))[0]) == 3


def test_engine_loads_directories_and_reports_bytes(tmp_path, caplog):
    adapter(1).save(str(tmp_path / "x"))
    with caplog.at_level("INFO"):
        e = engine((("x", str(tmp_path / "x")),))
    assert e.lora_names == ["x"] and e.lora_bytes == lora_bytes(CFG, 1, 64)
    assert any("LoRA adapters: 1 resident (x)" in r.getMessage() and str(e.lora_bytes) in r.getMessage()
               for r in caplog.records)
    from polykey_service_amd.utils.metrics import Metrics
    m = Metrics()
    m.observe_step(e, 0.0, [])
    assert m.registry.get_sample_value("polykey_engine_lora_bytes") == float(e.lora_bytes)
    plain = Metrics()
    plain.observe_step(engine(), 0.0, [])
    assert plain.registry.get_sample_value("polykey_engine_lora_bytes") == 0.0


def test_unknown_adapter_at_add_request():
    e = engine((("X", adapter(1)), ("Y", adapter(2))))
    with pytest.raises(ValueError, match=r"unknown LoRA adapter 'nope'.*X, Y"):
        e.add_request([1, 2, 3], SamplingParams(lora="nope"))
    with pytest.raises(ValueError, match="no adapters"):
        engine().add_request([1, 2, 3], SamplingParams(lora="X"))
    assert SamplingParams.from_dict({"lora": "X", "max_tokens": 2}).lora == "X"
    assert SamplingParams.from_dict({"max_tokens": 2}).lora is None
    with pytest.raises(ValueError):
        SamplingParams.from_dict({"lora": 3})


def test_prefix_cache_is_keyed_by_adapter():
    e = engine((("X", adapter(1)), ("Y", adapter(2))))
    prompt = [1] + list(range(100, 170))  # two full blocks of 32
    sp = lambda l: SamplingParams(max_tokens=2, lora=l)
    e.generate([prompt], sp("X"))
    assert e.scheduler.num_cached_tokens == 0
    e.generate([prompt], sp("Y"))              # another adapter: no shared blocks
    assert e.scheduler.num_cached_tokens == 0
    e.generate([prompt], sp(None))             # nor with the base model
    assert e.scheduler.num_cached_tokens == 0
    a = e.generate([prompt], sp("X"))          # the same adapter: a hit on both blocks
    assert e.scheduler.num_cached_tokens == 64
    cold = engine((("X", adapter(1)), ("Y", adapter(2))), prefix_caching=False)
    assert cold.generate([prompt], sp("X")) == a
    e.generate([prompt], sp(None))
    assert e.scheduler.num_cached_tokens == 128


def test_preemption_by_recompute_keeps_the_adapter():
    mods = (("X", adapter(1, b_std=0.08)), ("Y", adapter(2, b_std=0.08)))
    prompts = [[1] + list(range(50 + 40 * i, 50 + 40 * i + 30)) for i in range(4)]
    loras = ["X", None, "Y", "X"]

    def run(e, loras=loras):
        seqs = [e.add_request(p, SamplingParams(max_tokens=40, ignore_eos=True, lora=l)) for p, l in zip(prompts, loras)]
        while e.has_unfinished():
            e.step()
        return [s.output_ids for s in seqs]
    roomy = engine(mods, prefix_caching=False)
    exp = run(roomy)
    assert roomy.scheduler.num_preemptions == 0 and roomy.runner.stats["lora_steps"] > 0
    tight = engine(mods, prefix_caching=False, num_kv_blocks=7, watermark=0.0)
    got = run(tight)
    assert tight.scheduler.num_preemptions > 0
    assert got == exp
    base = run(engine((), prefix_caching=False), [None] * 4)
    assert base[1] == exp[1] and base[0] != exp[0] and base[2] != exp[2]
