"""The ``mxfp4`` weight dtype on the CPU: configuration (flag, env, the one name, error texts), the
refused combinations, tiny Llama and Qwen3 engines with MXFP4 projection weights on the fp32
reference path (what is quantised and when, bytes held, the gauge, the start-up line), and the
logits drift against the bf16 engine.

Every engine here is built by passing ``weight_dtype``."""
import copy
import dataclasses
import logging
import math

import pytest
import torch
from prometheus_client import generate_latest

from polykey_service_amd.config.server_config import load_server_config, normalize_weight_dtype
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.lora import LoraAdapter
from polykey_service_amd.ops import gemm, gemm_w4, gemm_w8
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.utils.metrics import Metrics

CPU = torch.device("cpu")
PROMPTS = [[1, 7, 8, 9, 10], [1] + list(range(40, 90)), [1, 300, 301]]
SP = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
PROJ = (("attn", "qkv", "ln1"), ("attn", "o", None), ("mlp", "gate_up", "ln2"), ("mlp", "down", None))


def engine(weight_dtype, model="tiny-llama", st=None, mdl=None, **kw) -> LLMEngine:
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, device="cpu", hip_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(model=model, weight_dtype=weight_dtype, **base), st or ParallelState(device=CPU),
                     model=mdl)


def fresh_model(name="tiny-llama", seed=3, random_ln=False):
    m = build_model(get_config(name), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(seed)
    g = torch.Generator().manual_seed(seed)
    if random_ln:
        for layer in m.layers:
            for n in ("ln1", "ln2"):
                getattr(layer, n).data.copy_((0.5 + torch.rand(getattr(layer, n).shape, generator=g)).to(torch.bfloat16))
    return m


def first_logits(e, prompt=PROMPTS[1]):
    e.runner.keep_logits = True
    e.generate([prompt], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    return e.runner.last_logits.float().clone()


# ------------------------------------------------------------------------------ configuration
def test_config_flag_env_the_one_name_and_error_texts(monkeypatch):
    monkeypatch.delenv("POLYKEY_WEIGHT_DTYPE", raising=False)
    assert load_server_config(["--weight-dtype", "mxfp4"], {}).weight_dtype == "mxfp4"
    assert load_server_config([], {"POLYKEY_WEIGHT_DTYPE": "mxfp4"}).weight_dtype == "mxfp4"
    assert load_server_config(["--weight-dtype", "mxfp4"], {"POLYKEY_WEIGHT_DTYPE": "fp8"}).weight_dtype == "fp8"
    assert [normalize_weight_dtype(v) for v in ("mxfp4", "MXFP4", " mxfp4 ")] == ["mxfp4"] * 3
    for bad in ("fp4", "int4", "mxfp4_e2m1", "nvfp4", "mxfp8", "e2m1"):   # the name is mxfp4 only
        with pytest.raises(ValueError) as e:
            normalize_weight_dtype(bad)
        assert all(c in str(e.value) for c in ("weight_dtype", "auto", "bf16", "fp8", "mxfp4"))
        with pytest.raises(ValueError, match="weight_dtype"):
            load_server_config(["--weight-dtype", bad], {})
    with pytest.raises(ValueError, match="weight_dtype"):
        engine("fp4")
    ec = EngineConfig.from_server_config(load_server_config(["--weight-dtype", "mxfp4", "--kv-cache-dtype", "fp8"], {}))
    assert ec.weight_dtype == "mxfp4" and ec.kv_cache_dtype == "fp8"
    # a config built without the field (the benchmark's) takes the environment's
    monkeypatch.setenv("POLYKEY_WEIGHT_DTYPE", "mxfp4")
    assert EngineConfig().weight_dtype == "mxfp4" and EngineConfig(weight_dtype="bf16").weight_dtype == "bf16"
    e = engine(EngineConfig().weight_dtype)
    assert e.cfg.weight_dtype == "mxfp4" and e.model.quantised_dtype == "mxfp4"


# ------------------------------------------------------------------------------- combinations
def test_unsupported_combinations_raise_and_name_the_setting():
    with pytest.raises(ValueError, match=r"weight_dtype=mxfp4.*MoE"):
        engine("mxfp4", model="tiny-mixtral")
    with pytest.raises(ValueError, match=r"weight_dtype=mxfp4.*tp=2"):
        engine("mxfp4", st=ParallelState(world_size=2, tp_size=2, device=CPU))
    with pytest.raises(ValueError, match=r"weight_dtype=mxfp4.*ep=2"):
        engine("mxfp4", st=ParallelState(world_size=2, ep_size=2, device=CPU))
    adapter = LoraAdapter.random(get_config("tiny-llama"), rank=8, alpha=16, seed=1, b_std=0.05)
    with pytest.raises(ValueError, match=r"LoRA.*weight_dtype=mxfp4.*follow-up"):
        engine("mxfp4", lora_modules=(("X", adapter),))
    # the model refuses too, whoever sets the attribute
    m = build_model(get_config("tiny-mixtral"), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(0)
    m.weight_dtype = "mxfp4"
    with pytest.raises(ValueError, match="weight_dtype=mxfp4"):
        m.pack_decode_weights()
    m = fresh_model()
    m.weight_dtype = "mxfp4"
    m.pack_decode_weights()
    with pytest.raises(ValueError, match=r"LoRA.*weight_dtype=mxfp4"):
        m.enable_lora((("X", adapter),), 8, 8)
    # projections the kernel does not tile: down's K = 1088 is no multiple of 256
    odd = dataclasses.replace(get_config("tiny-llama"), intermediate_size=1088)
    m = build_model(odd, ParallelState(device=CPU), torch.bfloat16, CPU).init_random(0)
    m.weight_dtype = "mxfp4"
    with pytest.raises(ValueError, match=r"weight_dtype=mxfp4 needs projections of N % 128 == 0 and K % 256 == 0"):
        m.pack_decode_weights()
    # bf16 engines of the same settings are untouched by the switch
    assert engine("auto", model="tiny-mixtral").cfg.weight_dtype == "bf16"


def test_a_model_quantised_to_one_format_serves_no_other():
    w4 = engine("mxfp4").model
    w8 = engine("fp8").model
    assert w4.quantised_dtype == "mxfp4" and not w4.w8 and w8.quantised_dtype == "fp8" and w8.w8
    with pytest.raises(ValueError, match=r"weight_dtype=bf16.*already MXFP4.*weight_dtype=mxfp4"):
        engine("bf16", mdl=w4)
    with pytest.raises(ValueError, match=r"weight_dtype=fp8.*already MXFP4"):
        engine("fp8", mdl=w4)
    with pytest.raises(ValueError, match=r"weight_dtype=mxfp4.*already FP8"):
        engine("mxfp4", mdl=w8)
    with pytest.raises(ValueError, match=r"weight_dtype=bf16.*already FP8: pass weight_dtype=fp8"):  # (unchanged)
        engine("bf16", mdl=w8)
    # the model refuses too
    w4.weight_dtype = "fp8"
    with pytest.raises(ValueError, match=r"already MXFP4 \(weight_dtype=mxfp4\); it cannot serve weight_dtype=fp8"):
        w4.pack_decode_weights()
    w4.weight_dtype = "mxfp4"
    # handed to a second engine of its own format it is not quantised twice
    assert engine("mxfp4", mdl=w4).model.layers[0].attn.qkv_p is w4.layers[0].attn.qkv_p


# ------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen3"])
def test_what_is_quantised_and_when(name, caplog):
    """After the fold, once: nibbles and scales are quantise(fold_norm(w, ln)) for QKV / gate_up and
    quantise(w) for o / down; the row-major attributes are meta placeholders, ln1 / ln2 ones with
    the originals kept; embedding, LM head and the norms (QK-norm included) untouched."""
    src = fresh_model(name, random_ln=True)
    with caplog.at_level(logging.INFO):
        e = engine("mxfp4", model=name, mdl=copy.deepcopy(src))
    m = e.model
    total = 0
    for ls, lq in zip(src.layers, m.layers):
        for owner, pname, ln in PROJ:
            h = getattr(getattr(lq, owner), pname + "_p")
            w = getattr(getattr(ls, owner), pname)
            assert isinstance(h, gemm_w4.W4) and not isinstance(h, gemm_w8.W8)
            nib, xs = ref.quantize_mxfp4_rows(w if ln is None else gemm.fold_norm(w, getattr(ls, ln)))
            got = h.bytes_rowmajor()
            assert torch.equal(got[0], nib) and torch.equal(got[1], xs), (owner, pname)
            assert h.shape == tuple(w.shape) and 2 <= int(xs.min()) and int(xs.max()) <= 252
            ph = getattr(getattr(lq, owner), pname)
            assert ph.is_meta and ph.shape == w.shape
            total += w.shape[0] * w.shape[1] // 2 + w.shape[0] * w.shape[1] // 32
        assert lq.attn.qkv_pf is lq.attn.qkv_p and lq.mlp.gate_up_pf is lq.mlp.gate_up_p
        for n in ("ln1", "ln2"):
            assert torch.equal(getattr(lq, n), torch.ones_like(getattr(ls, n)))
            assert torch.equal(getattr(lq, n + "_folded"), getattr(ls, n))
        if ls.attn.q_norm is not None:
            assert torch.equal(lq.attn.q_norm, ls.attn.q_norm) and torch.equal(lq.attn.k_norm, ls.attn.k_norm)
    assert (src.layers[0].attn.q_norm is not None) == (name == "tiny-qwen3")
    assert torch.equal(m.embed, src.embed) and torch.equal(m.norm, src.norm) and m.embed.dtype == torch.bfloat16
    assert m.lm_head.dtype == torch.bfloat16 and not m.lm_head.is_meta
    # bytes held by the layers' tensors: nibbles and scales, 4.25 bits per weight exactly
    nweights = sum(getattr(getattr(l, o), n).numel() for l in src.layers for o, n, _ in PROJ)
    assert e.weight_bytes == m.projection_bytes() == total == nweights * 17 // 32
    reg = Metrics()
    reg.observe_step(e, 0.001, [])
    text = generate_latest(reg.registry).decode()
    gauge = [l for l in text.splitlines() if l.startswith("polykey_engine_weight_bytes ")]
    assert len(gauge) == 1 and float(gauge[0].split()[1]) == float(total)
    assert m.widen_scratch_bytes() == 0          # the CPU engine has no wide path
    # one start-up line: dtype, projection bytes, scratch bytes
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith("weights:")]
    assert len(line) == 1 and "mxfp4" in line[0] and str(total) in line[0] and "scratch" in line[0]
    # greedy generation runs, repeatably, and gives its blocks back
    out = e.generate(PROMPTS, SP)
    assert [len(o) for o in out] == [8, 8, 8] and out == e.generate(PROMPTS, SP)
    assert e.bm.num_free == e.bm.num_blocks


def test_projections_compute_the_dequantised_weights_exactly():
    """Every W4 projection of the engine's model equals the fp32 reference path on the dequantised
    weight, which is exact in bf16."""
    e = engine("mxfp4", mdl=fresh_model(random_ln=True))
    g = torch.Generator().manual_seed(11)
    for lq in e.model.layers:
        for owner, name, _ in PROJ:
            h = getattr(getattr(lq, owner), name + "_p")
            deq = h.dequant().to(torch.bfloat16)
            assert torch.equal(deq.float(), h.dequant())                          # representable
            x = torch.randn((5, h.shape[1]), generator=g).to(torch.bfloat16)
            y = x.float() @ deq.float().t()
            if name == "gate_up":
                assert torch.equal(gemm_w4.linear_silu(x, h), ref.silu_and_mul_interleaved(y.to(torch.bfloat16)))
            assert torch.equal(gemm_w4.linear(x, h), y.to(torch.bfloat16)), (owner, name)


def test_with_an_fp8_kv_cache():
    e = engine("mxfp4", kv_cache_dtype="fp8")
    assert e.cfg.weight_dtype == "mxfp4" and e.cfg.kv_cache_dtype == "fp8"
    assert e.runner.kv_caches[0][0].dtype == torch.float8_e4m3fn and e.model.quantised_dtype == "mxfp4"
    out = e.generate(PROMPTS[:2], SP)
    assert [len(o) for o in out] == [8, 8] and out == engine("mxfp4", kv_cache_dtype="fp8").generate(PROMPTS[:2], SP)
    assert math.isfinite(float(first_logits(e).abs().max()))


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen3"])
def test_logits_drift_against_the_bf16_engine(name):
    """Distance of the first-token logits from the bf16 engine's, max |delta| / rms of the logits
    (random-init weights; printed).  Asserted only to be finite and below the drift of a mutant of
    the same quantised model whose scale bytes lost their low bit (every other block's weights
    halved): a measured comparison, not a constant."""
    src = fresh_model(name, random_ln=True)
    base = first_logits(engine("bf16", model=name, mdl=copy.deepcopy(src)))
    e = engine("mxfp4", model=name, mdl=copy.deepcopy(src))
    got = first_logits(e)
    for layer in e.model.layers:
        for owner, pname, _ in PROJ:
            h = getattr(getattr(layer, owner), pname + "_p")
            nib, xs = h.bytes_rowmajor()
            mutant = gemm_w4.W4.from_bytes(nib, xs & 0xFE)
            setattr(getattr(layer, owner), pname + "_p", mutant)
            if pname in ("qkv", "gate_up"):
                setattr(getattr(layer, owner), pname + "_pf", mutant)
    bad = first_logits(e)
    rms = float(base.pow(2).mean().sqrt())
    drift, drift_bad = float((got - base).abs().max()) / rms, float((bad - base).abs().max()) / rms
    print(f"{name}: mxfp4 logits drift {drift:.3f} of rms; scale-low-bit mutant {drift_bad:.3f}")
    assert math.isfinite(drift) and 0 < drift < drift_bad
