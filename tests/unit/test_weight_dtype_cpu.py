"""The weight dtype switch on the CPU: configuration (flag, env, alias, bad value), a tiny-llama
engine with FP8 projection weights on the fp32 reference path (what is quantised and when, what
the projections compute), the rejected combinations, the combination with an FP8 KV cache, and
the gauge.

Every engine here is built by passing ``weight_dtype``."""
import copy
import logging
import math

import pytest
import torch
from prometheus_client import generate_latest

from polykey_service_amd.config.server_config import load_server_config, normalize_weight_dtype
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import gemm, gemm_w8
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


def fresh_model(name="tiny-llama", seed=3, random_ln=False, pow2_rows=False):
    m = build_model(get_config(name), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(seed)
    g = torch.Generator().manual_seed(seed)
    for layer in m.layers:
        if random_ln:
            for n in ("ln1", "ln2"):
                getattr(layer, n).data.copy_((0.5 + torch.rand(getattr(layer, n).shape, generator=g)).to(torch.bfloat16))
        if pow2_rows:
            # the largest |w| of every row becomes 448 * 2^e exactly: the row's scale is then the
            # power of two 2^e, so bf16(scale * byte) is exact and the scale commutes with roundings
            for owner, name, _ in PROJ:
                w = getattr(getattr(layer, owner), name).data
                amax, idx = w.float().abs().max(dim=1)
                e = torch.ceil(torch.log2(amax / 448.0))
                rows = torch.arange(w.shape[0])
                w[rows, idx] = (torch.sign(w[rows, idx].float()) * 448.0 * torch.pow(2.0, e)).to(torch.bfloat16)
    return m


def folded(layer, owner, name, ln):
    w = getattr(getattr(layer, owner), name)
    return w if ln is None else gemm.fold_norm(w, getattr(layer, ln))


def first_logits(e, prompt=PROMPTS[1]):
    e.runner.keep_logits = True
    e.generate([prompt], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    return e.runner.last_logits.float().clone()


# ------------------------------------------------------------------------------ configuration
def test_config_flag_env_alias_and_bad_value(monkeypatch):
    monkeypatch.delenv("POLYKEY_WEIGHT_DTYPE", raising=False)
    assert load_server_config([], {}).weight_dtype == "bf16"                          # auto
    assert load_server_config(["--weight-dtype", "fp8"], {}).weight_dtype == "fp8"
    assert load_server_config([], {"POLYKEY_WEIGHT_DTYPE": "fp8_e4m3"}).weight_dtype == "fp8"
    assert load_server_config(["--weight-dtype", "fp8"], {"POLYKEY_WEIGHT_DTYPE": "bf16"}).weight_dtype == "bf16"
    assert [normalize_weight_dtype(v) for v in ("auto", "bf16", "FP8", "fp8_e4m3")] == ["bf16", "bf16", "fp8", "fp8"]
    for bad in ("fp16", "int8", "e5m2", "fp4", ""):
        with pytest.raises(ValueError) as e:
            normalize_weight_dtype(bad)
        assert all(c in str(e.value) for c in ("weight_dtype", "auto", "bf16", "fp8"))
    with pytest.raises(ValueError):
        load_server_config(["--weight-dtype", "int4"], {})
    with pytest.raises(ValueError, match="weight_dtype"):
        engine("int4")
    sc = load_server_config(["--weight-dtype", "fp8_e4m3", "--kv-cache-dtype", "fp8"], {})
    ec = EngineConfig.from_server_config(sc)
    assert ec.weight_dtype == "fp8" and ec.kv_cache_dtype == "fp8"
    assert EngineConfig().weight_dtype == "auto"
    # a config built without the field (the benchmark's) takes the environment's
    monkeypatch.setenv("POLYKEY_WEIGHT_DTYPE", "fp8")
    assert EngineConfig().weight_dtype == "fp8" and EngineConfig(weight_dtype="bf16").weight_dtype == "bf16"


# ------------------------------------------------------------------------------------- engine
def test_fp8_engine_generates_and_differs_from_bf16():
    a, b = engine("fp8"), engine("fp8_e4m3")
    out = a.generate(PROMPTS, SP)
    assert [len(o) for o in out] == [8, 8, 8]
    assert out == b.generate(PROMPTS, SP) == a.generate(PROMPTS, SP)
    assert a.cfg.weight_dtype == "fp8" and a.model.w8 and a.bm.num_free == a.bm.num_blocks
    f, g = first_logits(a), first_logits(engine("bf16"))
    d = (f - g).abs().max()
    assert 0 < float(d) < 0.5 * float(g.abs().max()), float(d)     # really quantised, and only a little off


def test_what_is_quantised_and_when():
    """After the fold, once: bytes and scales are quantise(fold_norm(w, ln)) for QKV / gate_up and
    quantise(w) for o / down; the row-major attributes are meta placeholders, ln1 / ln2 ones with
    the originals kept; embedding, LM head and final norm untouched."""
    src = fresh_model(random_ln=True)
    e = engine("fp8", mdl=copy.deepcopy(src))
    m = e.model
    total = 0
    for ls, lq in zip(src.layers, m.layers):
        for owner, name, ln in PROJ:
            h = getattr(getattr(lq, owner), name + "_p")
            assert isinstance(h, gemm_w8.W8)
            b, scale = ref.quantize_fp8_rows(folded(ls, owner, name, ln))
            assert torch.equal(h.bytes_rowmajor().view(torch.uint8), b.view(torch.uint8)), (owner, name)
            assert torch.equal(h.scale, scale) and h.shape == tuple(getattr(getattr(ls, owner), name).shape)
            ph = getattr(getattr(lq, owner), name)
            assert ph.is_meta and ph.shape == getattr(getattr(ls, owner), name).shape
            total += h.shape[0] * h.shape[1] + 4 * h.shape[0]
        assert lq.attn.qkv_pf is lq.attn.qkv_p and lq.mlp.gate_up_pf is lq.mlp.gate_up_p
        for n in ("ln1", "ln2"):
            assert torch.equal(getattr(lq, n), torch.ones_like(getattr(ls, n)))
            assert torch.equal(getattr(lq, n + "_folded"), getattr(ls, n))
    assert torch.equal(m.embed, src.embed) and torch.equal(m.norm, src.norm) and m.embed.dtype == torch.bfloat16
    assert m.lm_head.dtype == torch.bfloat16 and not m.lm_head.is_meta
    # bytes held by the layers' tensors: sum of N K + 4 N, exactly -- under half of bf16's
    assert e.weight_bytes == m.projection_bytes() == total
    assert engine("bf16", mdl=copy.deepcopy(src)).weight_bytes == sum(
        2 * getattr(getattr(l, o), n).numel() for l in src.layers for o, n, _ in PROJ)
    reg = Metrics()
    reg.observe_step(e, 0.001, [])
    text = generate_latest(reg.registry).decode()
    gauge = [l for l in text.splitlines() if l.startswith("polykey_engine_weight_bytes ")]
    assert len(gauge) == 1 and float(gauge[0].split()[1]) == float(total)
    # a model handed to a second engine is not quantised twice; a bf16 engine refuses it
    assert engine("fp8", mdl=m).model.layers[0].attn.qkv_p is m.layers[0].attn.qkv_p
    with pytest.raises(ValueError, match="weight_dtype=bf16.*already FP8"):
        engine("bf16", mdl=m)
    assert m.w8_scratch_bytes() == 0          # the CPU engine has no wide path


def test_projections_compute_the_dequantised_weights_exactly():
    """With power-of-two row scales bf16(scale * widen(byte)) is exact and the scale commutes with
    every rounding, so each W8 projection of the engine's model equals the fp32 reference path on
    the dequantised bf16 weight, bit for bit."""
    src = fresh_model(pow2_rows=True)
    e = engine("fp8", mdl=copy.deepcopy(src))
    g = torch.Generator().manual_seed(11)
    for ls, lq in zip(src.layers, e.model.layers):
        for owner, name, ln in PROJ:
            h = getattr(getattr(lq, owner), name + "_p")
            assert bool((torch.log2(h.scale) == torch.round(torch.log2(h.scale))).all()), (owner, name)
            deq = h.dequant().to(torch.bfloat16)
            assert torch.equal(deq.float(), h.dequant())                          # representable
            x = torch.randn((5, h.shape[1]), generator=g).to(torch.bfloat16)
            y = x.float() @ deq.float().t()
            if name == "gate_up":
                assert torch.equal(gemm_w8.linear_silu(x, h), ref.silu_and_mul_interleaved(y.to(torch.bfloat16)))
            assert torch.equal(gemm_w8.linear(x, h), y.to(torch.bfloat16)), (owner, name)


def test_fp8_engine_against_a_bf16_engine_on_the_dequantised_weights(monkeypatch):
    """The W8 engine's logits equal, bit for bit, those of a bf16 engine whose projection weights
    are bf16(scale * widen(byte)) of the same folded weights, when that engine's projections take
    the fp32 reference path (an fp32 matmul, one rounding) as the W8 ops do on the CPU.  With
    power-of-two row scales the dequantised weight is exact in bf16 and the scale commutes with
    the rounding, so both engines evaluate the same function with the same roundings in the same
    order.  (The bf16 engine's own CPU GEMM accumulates in another order; against it the logits
    agree to about 2^-7 in rms, which proves nothing either way.)"""
    src = fresh_model(pow2_rows=True)
    w8 = engine("fp8", mdl=copy.deepcopy(src))
    twin = copy.deepcopy(src)
    for lt, lq in zip(twin.layers, w8.model.layers):
        for owner, name, _ in PROJ:
            getattr(getattr(lt, owner), name).data.copy_(getattr(getattr(lq, owner), name + "_p").dequant())
    a = first_logits(w8)
    plain = first_logits(engine("bf16", mdl=copy.deepcopy(src)))

    def fp32_linear(x, w, out=None, packed=None, max_m=None):
        y = (x.float() @ w.float().t()).to(x.dtype)
        return y if out is None else out.copy_(y)

    monkeypatch.setattr(gemm, "linear", fp32_linear)
    b = first_logits(engine("bf16", mdl=twin))
    assert torch.equal(a, b)
    assert not torch.equal(a, plain)


def test_start_up_logs_dtype_bytes_and_scratch(caplog):
    with caplog.at_level(logging.INFO):
        e = engine("fp8")
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith("weights:")]
    assert len(line) == 1 and "fp8" in line[0] and str(e.weight_bytes) in line[0] and "scratch" in line[0]


# ------------------------------------------------------------------------------- combinations
def test_unsupported_combinations_raise_and_name_the_setting():
    with pytest.raises(ValueError, match=r"weight_dtype=fp8.*MoE"):
        engine("fp8", model="tiny-mixtral")
    with pytest.raises(ValueError, match=r"weight_dtype=fp8.*tp=2"):
        engine("fp8", st=ParallelState(world_size=2, tp_size=2, device=CPU))
    with pytest.raises(ValueError, match=r"weight_dtype=fp8.*ep=2"):
        engine("fp8", st=ParallelState(world_size=2, ep_size=2, device=CPU))
    # the model refuses too, whoever sets the attribute
    m = build_model(get_config("tiny-mixtral"), ParallelState(device=CPU), torch.bfloat16, CPU).init_random(0)
    m.weight_dtype = "fp8"
    with pytest.raises(ValueError, match="weight_dtype=fp8"):
        m.pack_decode_weights()
    # bf16 engines of the same settings are untouched by the switch
    assert engine("auto", model="tiny-mixtral").cfg.weight_dtype == "bf16"


def test_with_an_fp8_kv_cache():
    e = engine("fp8", kv_cache_dtype="fp8")
    assert e.cfg.weight_dtype == "fp8" and e.cfg.kv_cache_dtype == "fp8"
    assert e.runner.kv_caches[0][0].dtype == torch.float8_e4m3fn and e.model.w8
    out = e.generate(PROMPTS[:2], SP)
    assert [len(o) for o in out] == [8, 8] and out == engine("fp8", kv_cache_dtype="fp8").generate(PROMPTS[:2], SP)
    assert math.isfinite(float(first_logits(e).abs().max()))
