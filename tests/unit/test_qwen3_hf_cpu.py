"""Qwen3 dense against the upstream implementation (``transformers.Qwen3ForCausalLM``, fp32, CPU).

The semantic anchor of the QK-norm feature: a tiny Qwen3 built by transformers is saved, loaded by
the engine on the CPU (bf16, the fp32 reference ops) and compared on last-position logits with

    e = max|engine - HF| / rms(HF logits)

over three prompts of 5, 33 and 70 tokens.  The bound is 3 x the ``e`` the same harness measures for
a Llama twin (``transformers.LlamaForCausalLM``, same dimensions), which runs through code without
QK-norm: the factor covers the two extra normalisations per layer.  Both models' weights are bf16
values held in fp32, so the weights the two sides see are identical and ``e`` is the engine's bf16
arithmetic alone.  Every norm weight (q_norm, k_norm, layernorms) is overwritten with seeded values
in [0.5, 1.5]: HF initialises them to ones, which would hide a norm weight that is never applied.

Two mutants must exceed the bound: the engine with its q_norm / k_norm replaced by ones, and the
norm applied after the rotation.  (HF rounds the normalised head to the model dtype before it
rotates; the engine rounds once, after norm + rotation.  In HF's fp32 the two agree.)
"""
import json
import os

import pytest
import torch

transformers = pytest.importorskip("transformers")

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.config import from_hf_config
from polykey_service_amd.ops import reference
from polykey_service_amd.parallel.state import ParallelState

CPU = torch.device("cpu")
DIMS = dict(vocab_size=1024, hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=16,
            num_key_value_heads=4, head_dim=128, rms_norm_eps=1e-6, max_position_embeddings=2048,
            tie_word_embeddings=False, attention_bias=False, bos_token_id=1, eos_token_id=2)
THETA = 1e6
_g = torch.Generator().manual_seed(11)
PROMPTS = [[1] + torch.randint(3, 1024, (n - 1,), generator=_g).tolist() for n in (5, 33, 70)]


def _hf_model(kind: str):
    torch.manual_seed(7)
    if kind == "qwen3":
        cfg = transformers.Qwen3Config(**DIMS, rope_parameters={"rope_type": "default", "rope_theta": THETA})
        m = transformers.Qwen3ForCausalLM(cfg)
    else:
        cfg = transformers.LlamaConfig(**DIMS, rope_parameters={"rope_type": "default", "rope_theta": THETA})
        m = transformers.LlamaForCausalLM(cfg)
    m = m.float().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight") or "layernorm" in name:
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            p.copy_(p.bfloat16().float())  # the engine holds bf16 weights: give HF the same values
    return m


def _engine(path: str) -> LLMEngine:
    return LLMEngine(EngineConfig(model_path=path, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=256,
                                  device="cpu", hip_graphs=False), ParallelState(device=CPU))


def _engine_logits(eng: LLMEngine):
    eng.runner.keep_logits = True
    out = []
    for p in PROMPTS:
        eng.generate([p], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
        out.append(eng.runner.last_logits.float()[-1].clone())
    return out


def _hf_logits(m):
    with torch.no_grad():
        return [m(torch.tensor([p])).logits[0, -1].float() for p in PROMPTS]


def _err(got, want) -> float:
    return max(float((g - w).abs().max() / w.pow(2).mean().sqrt()) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def anchor(tmp_path_factory):
    """HF logits, checkpoint directories and the measured ``e`` of the Qwen3 model and its Llama twin."""
    out = {}
    for kind in ("llama", "qwen3"):
        d = str(tmp_path_factory.mktemp(kind))
        m = _hf_model(kind)
        m.save_pretrained(d)
        want = _hf_logits(m)
        out[kind] = dict(dir=d, want=want, e=_err(_engine_logits(_engine(d)), want), hf=m)
    out["bound"] = 3.0 * out["llama"]["e"]
    return out


def test_engine_matches_hf_qwen3(anchor):
    e_q, e_l, bound = anchor["qwen3"]["e"], anchor["llama"]["e"], anchor["bound"]
    print(f"e(qwen3) = {e_q:.3e}  e(llama twin) = {e_l:.3e}  bound = {bound:.3e}")
    assert e_l > 0.0
    assert e_q <= bound, (e_q, bound)


def test_loaded_config_and_norm_weights(anchor):
    d = anchor["qwen3"]["dir"]
    cfg = get_config(d)
    assert cfg.qk_norm and cfg.rope_theta == THETA and cfg.rms_eps == 1e-6 and cfg.q_size == 2048 != cfg.hidden_size
    assert not get_config(anchor["llama"]["dir"]).qk_norm
    eng = _engine(d)
    hf = anchor["qwen3"]["hf"].state_dict()
    for i, layer in enumerate(eng.model.layers):
        for n in ("q_norm", "k_norm"):
            w = getattr(layer.attn, n)
            assert w.shape == (128,) and w.dtype == torch.bfloat16
            assert torch.equal(w.float(), hf[f"model.layers.{i}.self_attn.{n}.weight"])
            assert float(w.float().min()) >= 0.5 and float((w.float() - 1).abs().max()) > 0.1


def test_mutant_norm_weights_ones_exceeds_bound(anchor):
    eng = _engine(anchor["qwen3"]["dir"])
    for layer in eng.model.layers:
        layer.attn.q_norm.data.fill_(1.0)
        layer.attn.k_norm.data.fill_(1.0)
    e = _err(_engine_logits(eng), anchor["qwen3"]["want"])
    print(f"e(norm weights = ones) = {e:.3e}  bound = {anchor['bound']:.3e}")
    assert e > anchor["bound"]


def test_mutant_norm_after_rope_exceeds_bound(anchor, monkeypatch):
    real = reference.rope_and_cache
    monkeypatch.setattr(reference, "rope_and_cache", lambda *a, **kw: real(*a, mutant="after_rope", **kw))
    e = _err(_engine_logits(_engine(anchor["qwen3"]["dir"])), anchor["qwen3"]["want"])
    print(f"e(norm after RoPE) = {e:.3e}  bound = {anchor['bound']:.3e}")
    assert e > anchor["bound"]


def test_missing_norm_weight_is_an_error(anchor, tmp_path):
    from safetensors.torch import load_file, save_file
    src = anchor["qwen3"]["dir"]
    sd = {k: v for k, v in load_file(os.path.join(src, "model.safetensors")).items()
          if k != "model.layers.1.self_attn.k_norm.weight"}
    save_file(sd, str(tmp_path / "model.safetensors"))
    with open(os.path.join(src, "config.json")) as f, open(tmp_path / "config.json", "w") as g:
        g.write(f.read())
    with pytest.raises(KeyError, match="k_norm"):
        _engine(str(tmp_path))


def _random_qwen3():
    return build_model(get_config("tiny-qwen3"), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(3)


def test_init_random_norm_weights_are_seeded_and_not_ones():
    a, b = _random_qwen3(), _random_qwen3()
    for la, lb in zip(a.layers, b.layers):
        for n in ("q_norm", "k_norm"):
            w = getattr(la.attn, n).float()
            assert torch.equal(w, getattr(lb.attn, n).float())
            assert 0.5 <= float(w.min()) and float(w.max()) <= 1.5 and float(w.std()) > 0.2
    assert not torch.equal(a.layers[0].attn.q_norm, a.layers[0].attn.k_norm)
    assert not torch.equal(a.layers[0].attn.q_norm, a.layers[1].attn.q_norm)
    llama = build_model(get_config("tiny-llama"), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(3)
    assert llama.layers[0].attn.q_norm is None and llama.layers[0].attn.k_norm is None


def test_save_hf_round_trip_and_hf_loads_it(tmp_path):
    m = _random_qwen3()
    d = str(tmp_path / "out")
    m.save_hf(d)
    with open(os.path.join(d, "config.json")) as f:
        c = json.load(f)
    assert c["architectures"] == ["Qwen3ForCausalLM"] and c["model_type"] == "qwen3"
    cfg = get_config(d)
    assert cfg.qk_norm
    again = build_model(cfg, ParallelState(device=CPU), torch.bfloat16, CPU).load_hf(d)
    a, b = m.hf_state_dict(), again.hf_state_dict()
    assert a.keys() == b.keys() and any("q_norm" in k for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # upstream reads the directory we wrote, and computes what the engine computes from it
    hf = transformers.Qwen3ForCausalLM.from_pretrained(d, dtype=torch.float32).eval()
    assert hf.config.rope_parameters["rope_theta"] == 1e6
    sd = hf.state_dict()
    assert torch.equal(sd["model.layers.0.self_attn.q_norm.weight"], a["model.layers.0.self_attn.q_norm.weight"].float())
    want = _hf_logits(hf)
    e = _err(_engine_logits(_engine(d)), want)
    print(f"e(engine vs HF on the engine's own checkpoint) = {e:.3e}")
    assert e < 0.1  # a loose sanity bound (the anchor test holds the tight one): ones / wrong theta give more


def test_rope_parameters_and_legacy_rope_theta_give_the_same_config(tmp_path):
    base = dict(DIMS, architectures=["Qwen3ForCausalLM"], model_type="qwen3")
    new = dict(base, rope_parameters={"rope_type": "default", "rope_theta": THETA})
    old = dict(base, rope_theta=THETA, rope_scaling=None)
    cfgs = []
    for name, c in (("new", new), ("old", old)):
        (tmp_path / name).mkdir()
        p = tmp_path / name / "config.json"
        p.write_text(json.dumps(dict(c, _name_or_path="m")))
        cfgs.append(from_hf_config(str(p)))
    assert cfgs[0] == cfgs[1] and cfgs[0].rope_theta == THETA and cfgs[0].rope_scaling is None and cfgs[0].qk_norm
    # a non-default rope type inside rope_parameters is the scaling
    scaled = dict(base, rope_parameters={"rope_type": "llama3", "rope_theta": THETA, "factor": 8.0,
                                         "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                         "original_max_position_embeddings": 8192})
    p = tmp_path / "scaled.json"
    p.write_text(json.dumps(scaled))
    c = from_hf_config(str(p))
    assert c.rope_theta == THETA and c.rope_scaling["rope_type"] == "llama3" and c.rope_scaling["factor"] == 8.0
    assert "rope_theta" not in c.rope_scaling


@pytest.mark.parametrize("extra,word", [
    (dict(architectures=["Qwen2ForCausalLM"], model_type="qwen2"), "Qwen2ForCausalLM"),
    (dict(architectures=["Qwen3MoeForCausalLM"], model_type="qwen3_moe"), "Qwen3MoeForCausalLM"),
    (dict(model_type="qwen2"), "Qwen2ForCausalLM"),
    (dict(architectures=["LlamaForCausalLM"], model_type="llama", attention_bias=True), "attention_bias"),
])
def test_refused_by_name(tmp_path, extra, word):
    p = tmp_path / "config.json"
    p.write_text(json.dumps(dict(DIMS, rope_theta=1e6, **{"attention_bias": False, **extra})))
    with pytest.raises(ValueError, match=word):
        from_hf_config(str(p))
    with pytest.raises(ValueError, match=word):
        get_config(str(tmp_path))


def test_llama_and_keyless_configs_load_as_before(tmp_path):
    bare = {k: v for k, v in DIMS.items() if k != "attention_bias"}
    for i, extra in enumerate((dict(), dict(architectures=["LlamaForCausalLM"], model_type="llama"),
                               dict(architectures=["MistralForCausalLM"], model_type="mistral"))):
        p = tmp_path / f"c{i}.json"
        p.write_text(json.dumps(dict(bare, rope_theta=5e5, _name_or_path="x", **extra)))
        c = from_hf_config(str(p))
        assert not c.qk_norm and c.rope_theta == 5e5 and c.name == "x" and c.rope_scaling is None
    p = tmp_path / "moe.json"
    p.write_text(json.dumps(dict(bare, architectures=["MixtralForCausalLM"], model_type="mixtral",
                                 num_local_experts=4, num_experts_per_tok=2)))
    c = from_hf_config(str(p))
    assert c.is_moe and not c.qk_norm and c.rope_theta == 10000.0
