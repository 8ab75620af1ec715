"""The KV-cache dtype switch on the CPU: configuration (flag, env, alias, bad value), cache sizing
(half the bytes per block, twice the blocks), an FP8 tiny-llama engine on the CPU reference path
(greedy generation, determinism, prefix-cache hits, preemption + recompute), the checkpoint
round trip of the per-layer scales, and the reference writer / reader pair.

Every engine here is built by passing ``kv_cache_dtype``."""
import pytest
import torch
from prometheus_client import generate_latest

from polykey_service_amd.config.server_config import load_server_config, normalize_kv_cache_dtype
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.parallel.state import ParallelState
from polykey_service_amd.utils.metrics import Metrics

FP8 = torch.float8_e4m3fn


def engine(kv_cache_dtype, model="tiny-llama", **kw) -> LLMEngine:
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, device="cpu", hip_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(model=model, kv_cache_dtype=kv_cache_dtype, **base),
                     ParallelState(device=torch.device("cpu")))


# ------------------------------------------------------------------------------ configuration
def test_config_flag_env_alias_and_bad_value():
    assert load_server_config([], {}).kv_cache_dtype == "bf16"                       # auto
    assert load_server_config(["--kv-cache-dtype", "fp8"], {}).kv_cache_dtype == "fp8"
    assert load_server_config([], {"POLYKEY_KV_CACHE_DTYPE": "fp8_e4m3"}).kv_cache_dtype == "fp8"
    assert load_server_config(["--kv-cache-dtype", "fp8"], {"POLYKEY_KV_CACHE_DTYPE": "bf16"}).kv_cache_dtype == "bf16"
    assert [normalize_kv_cache_dtype(v) for v in ("auto", "bf16", "FP8", "fp8_e4m3")] == ["bf16", "bf16", "fp8", "fp8"]
    for bad in ("fp16", "int8", "e5m2", ""):
        with pytest.raises(ValueError) as e:
            normalize_kv_cache_dtype(bad)
        assert all(c in str(e.value) for c in ("auto", "bf16", "fp8"))
    with pytest.raises(ValueError):
        load_server_config(["--kv-cache-dtype", "fp4"], {})
    with pytest.raises(ValueError):
        engine("int4")
    sc = load_server_config(["--kv-cache-dtype", "fp8_e4m3"], {})
    assert EngineConfig.from_server_config(sc).kv_cache_dtype == "fp8"
    assert EngineConfig().kv_cache_dtype == "auto"


def test_bytes_per_block_halve_and_blocks_double():
    b, f = engine("auto"), engine("fp8")
    assert b.cfg.kv_cache_dtype == "bf16" and f.cfg.kv_cache_dtype == "fp8"
    assert f.runner.kv_bytes_per_block() * 2 == b.runner.kv_bytes_per_block()
    assert f.kv_bytes_per_token * 2 == b.kv_bytes_per_token
    # num_kv_blocks = 0: the automatic budget is a byte budget
    assert f.runner.num_blocks == 2 * b.runner.num_blocks == f.bm.num_blocks
    for (k, v), (kb, vb) in zip(f.runner.kv_caches, b.runner.kv_caches):
        assert k.dtype == v.dtype == FP8 and kb.dtype == vb.dtype == torch.bfloat16
        assert k.shape[1:] == kb.shape[1:] and v.shape[1:] == vb.shape[1:]
        assert int(k.view(torch.uint8).max()) == 0
    # an explicit block count is kept
    assert engine("fp8", num_kv_blocks=24).runner.num_blocks == 24
    m = Metrics()
    m.observe_step(f, 0.001, [])
    assert f"polykey_engine_kv_cache_bytes_per_token {float(f.kv_bytes_per_token)}" in generate_latest(m.registry).decode()


def test_routing_follows_the_dtype_of_the_cache_at_hand(monkeypatch):
    """The bf16-only launches are refused for an FP8 cache whoever allocated it: the model looks
    at the tensor, and the two GEMM wrappers assert bf16."""
    from polykey_service_amd.ops import gemm
    monkeypatch.setattr(gemm, "QKV_ATTN_MIN_KV", 1)
    cfg = get_config("tiny-llama-gqa4")
    m = build_model(cfg, ParallelState(device=torch.device("cpu")), torch.bfloat16, torch.device("cpu"))
    at = m.layers[0].attn
    md = A.AttnMetadata(num_decode=8, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0, slot_mapping=None)
    k16 = torch.zeros(2, at.nkv, 32, 128, dtype=torch.bfloat16)
    k8 = torch.zeros(2, at.nkv, 32, 128, dtype=torch.uint8).view(FP8)
    nparts = cfg.hidden_size // gemm.PART_COLS
    assert m._qkv_attn_fused_ok(at, 8, nparts, md, k16) and m._qkv_attn_fused_ok(at, 8, nparts, md)
    assert not m._qkv_attn_fused_ok(at, 8, nparts, md, k8)
    m.carry_collectives = True
    assert not m._carry_ok(torch.zeros(8, cfg.hidden_size, dtype=torch.bfloat16), md, k8)
    with pytest.raises(AssertionError, match="bf16 caches only"):
        gemm.qkv_reduce_rope_cache(None, None, None, k8, k8, None, at.nq, at.nkv)
    with pytest.raises(AssertionError, match="bf16 caches only"):
        gemm.qkv_attn_fused(torch.zeros(8, 4), None, None, None, None, None, k8, k8, md, 1.0, at.nq, at.nkv, None)


# ------------------------------------------------------------------------------------- engine
PROMPTS = [[1, 7, 8, 9, 10], [1] + list(range(40, 90)), [1, 300, 301]]
SP = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)


def test_fp8_engine_generates_deterministically():
    a, b = engine("fp8"), engine("fp8_e4m3")
    out = a.generate(PROMPTS, SP)
    assert [len(o) for o in out] == [8, 8, 8]
    assert out == b.generate(PROMPTS, SP) == a.generate(PROMPTS, SP)
    assert any(int(k.view(torch.uint8).max()) > 0 for k, _ in a.runner.kv_caches)     # the cache holds bytes
    assert a.bm.num_free == a.bm.num_blocks


def test_fp8_engine_prefix_cache_hits_change_nothing():
    system = [1] + list(range(100, 170))
    first = system + [7, 8, 9]
    later = [system + [11, 12, 13, 14], system + list(range(300, 340)), system[:64] + [5, 6]]
    cold = engine("fp8", prefix_caching=False)
    exp = cold.generate([first], SP) + cold.generate(later, SP)
    warm = engine("fp8", prefix_caching=True)
    got = warm.generate([first], SP) + warm.generate(later, SP)
    assert warm.scheduler.num_cached_tokens == 3 * 64 and cold.scheduler.num_cached_tokens == 0
    assert got == exp


def test_fp8_engine_preemption_and_recompute_change_nothing():
    prompts = [[1] + list(range(50 + 40 * i, 50 + 40 * i + 30)) for i in range(4)]
    sp = SamplingParams(max_tokens=40, temperature=0.0, ignore_eos=True)
    roomy = engine("fp8", prefix_caching=False)
    exp = roomy.generate(prompts, sp)
    assert roomy.scheduler.num_preemptions == 0
    # 4 sequences x 71 tokens need 12 blocks of 32: 7 force the youngest out and back in
    tight = engine("fp8", prefix_caching=False, num_kv_blocks=7, watermark=0.0)
    got = tight.generate(prompts, sp)
    assert tight.scheduler.num_preemptions > 0
    assert got == exp


def test_fp8_and_bf16_engines_are_different_caches_same_interface():
    """The FP8 engine really quantises: its first-step logits differ from bf16's, a little."""
    outs = {}
    for dt in ("bf16", "fp8"):
        e = engine(dt)
        e.runner.keep_logits = True
        e.generate([PROMPTS[1]], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
        outs[dt] = e.runner.last_logits.float().clone()
    d = (outs["fp8"] - outs["bf16"]).abs().max()
    assert 0 < float(d) < 0.5 * float(outs["bf16"].abs().max()), float(d)


def test_mixtral_fp8_engine_generates():
    e = engine("fp8", model="tiny-mixtral")
    out = e.generate(PROMPTS[:2], SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True))
    assert [len(o) for o in out] == [4, 4] and e.runner.kv_caches[0][0].dtype == FP8


# --------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("name", ["tiny-llama-gqa4", "tiny-mixtral"])
def test_scales_round_trip_through_a_checkpoint(tmp_path, name):
    cfg = get_config(name)
    st = ParallelState()
    a = build_model(cfg, st, torch.bfloat16, torch.device("cpu")).init_random(3)
    assert all(l.attn.k_scale == 1.0 and l.attn.v_scale == 1.0 for l in a.layers)
    assert not any("scale" in k for k in a.hf_state_dict())            # scales of 1 are not written
    for i, layer in enumerate(a.layers):
        layer.attn.k_scale, layer.attn.v_scale = 0.5 + 0.25 * i, 2.0 if i == 0 else 1.0
    sd = a.hf_state_dict()
    assert sd["model.layers.0.self_attn.k_scale"].shape == () and sd["model.layers.0.self_attn.k_scale"].dtype == torch.float32
    assert "model.layers.1.self_attn.v_scale" not in sd and "model.layers.0.self_attn.v_scale" in sd
    a.save_hf(str(tmp_path))
    b = build_model(get_config(str(tmp_path)), st, torch.bfloat16, torch.device("cpu")).load_hf(str(tmp_path))
    assert [(l.attn.k_scale, l.attn.v_scale) for l in b.layers] == [(l.attn.k_scale, l.attn.v_scale) for l in a.layers]


def test_engine_uses_the_checkpoint_scales(tmp_path):
    cfg = get_config("tiny-llama")
    a = build_model(cfg, ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(5)
    for layer in a.layers:
        layer.attn.k_scale, layer.attn.v_scale = 0.25, 0.125
    a.save_hf(str(tmp_path))
    e = engine("fp8", model_path=str(tmp_path))
    assert all((l.attn.k_scale, l.attn.v_scale) == (0.25, 0.125) for l in e.model.layers)
    plain = engine("fp8", seed=5)
    e.generate([PROMPTS[1]], SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    plain.generate([PROMPTS[1]], SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    # the same k / v stored at another scale: other bytes
    assert not torch.equal(e.runner.kv_caches[0][0].view(torch.uint8), plain.runner.kv_caches[0][0].view(torch.uint8))


# ----------------------------------------------------------------- reference writer and reader
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.5, 2.0), (0.3, 1.7)])
def test_reference_writer_and_reader(ks, vs):
    """rope_and_cache stores cast(x / scale) and paged_attention reads scale * byte."""
    nq, nkv, bs, hd = 2, 1, 32, 128
    vals = torch.tensor([1.0625, 1.1875, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.0 ** -10, 448.0, 464.0, 1e4, -0.0, -3.3])
    T = 3
    qkv = torch.zeros(T, nq + 2 * nkv, hd, dtype=torch.bfloat16)
    qkv[:, nq, :10] = vals.to(torch.bfloat16)            # k
    qkv[:, nq + 1, :10] = -vals.to(torch.bfloat16)       # v
    cs = torch.cat([torch.ones(8, 64), torch.zeros(8, 64)], dim=1)      # identity rotation
    kc = torch.zeros(2, nkv, bs, hd, dtype=torch.uint8).view(FP8)
    vc = torch.zeros(2, nkv, hd, bs, dtype=torch.uint8).view(FP8)
    slots = torch.tensor([33, -1, 5], dtype=torch.int32)
    A.rope_and_cache(qkv.view(T, -1), torch.arange(T, dtype=torch.int32), cs, kc, vc, slots, nq, nkv, hd,
                     k_scale=ks, v_scale=vs)
    want_k = (vals.to(torch.bfloat16).float() / ks).clamp(-448, 448).to(FP8)
    want_v = (-vals.to(torch.bfloat16).float() / vs).clamp(-448, 448).to(FP8)
    kl, vl = ref.k_cache_logical(kc.view(torch.uint8)), ref.v_cache_logical(vc.view(torch.uint8))
    for blk, off in ((1, 1), (0, 5)):
        assert torch.equal(kl[blk, 0, off, :10], want_k.view(torch.uint8))
        assert torch.equal(vl[blk, 0, off, :10], want_v.view(torch.uint8))
    assert int((kl != 0).sum()) <= 2 * 10 and int(kl[0, 0, 6].sum()) == 0       # slot -1: nothing stored
    # reader: one sequence of 6 keys in block 0; the only non-zero row is key 5
    k, v = ref.gather_kv(kc, vc, torch.tensor([0, 1]), 6)
    assert k.dtype == FP8 and torch.equal(ref.dequantize_fp8(k, ks)[5, 0, :10], want_k.float() * ks)
    q = torch.zeros(1, nq, hd, dtype=torch.bfloat16)
    out = ref.paged_attention(q, kc, vc, torch.tensor([[0, 1]]), torch.tensor([6]), torch.tensor([0, 1]), 1.0,
                              k_scale=ks, v_scale=vs)
    # zero queries: uniform weights 1/6 over the keys, five of them zero rows
    torch.testing.assert_close(out[0, 0, :10].float(), (want_v.float() * vs / 6).to(torch.bfloat16).float())
