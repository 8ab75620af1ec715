"""End-to-end engines with an FP8 (e4m3) KV cache on the GPU: against the CPU FP8 engine (the
reference path quantises and dequantises the same way), graphs against eager, continuations
against the synchronous loop, contexts crossing the 512-key partition, Mixtral, TP=2 on one GPU,
and the routing rule that an FP8 engine never takes the bf16-only fused QKV -> attention launch."""
import copy
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import gemm
from polykey_service_amd.parallel.state import ParallelState
from tests.model_cases import NORM_SEED, randomize_norms

pytestmark = pytest.mark.gpu
# norm-weight draws (tests/model_cases.py randomize_norms) per model: ones for which the CPU engine's first-token
# top-2 margins stay at least 0.19 of the logits' rms on every prompt of the first-token comparisons, the
# condition the model seeds were chosen by
NORM_SEEDS = {"tiny-mixtral": 0}
FP8 = torch.float8_e4m3fn


def _models(name, scales=None):
    cfg = get_config(name)
    cpu = build_model(cfg, ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    randomize_norms(cpu, NORM_SEEDS.get(name, NORM_SEED))  # before the copy: both engines share them
    for i, layer in enumerate(cpu.layers):
        if scales:
            layer.attn.k_scale, layer.attn.v_scale = scales[i % len(scales)]
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return cpu, gpu


def _engine(name, model, dev="cuda", graphs=True, **kw):
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512)
    base.update(kw)
    e = LLMEngine(EngineConfig(model=name, hip_graphs=graphs, device=dev, kv_cache_dtype="fp8", **base),
                  ParallelState(device=torch.device(dev)), model=model)
    assert all(k.dtype == FP8 and v.dtype == FP8 for k, v in e.runner.kv_caches)
    return e


@pytest.mark.parametrize("name,scales", [("tiny-llama", None), ("tiny-llama-gqa4", ((0.5, 2.0), (2.0, 0.5)))])
def test_first_tokens_match_the_cpu_fp8_engine(name, scales):
    cpu, gpu = _models(name, scales)
    prompts = [[1] + list(range(5, 5 + n)) for n in (3, 40, 77)]
    outs = {}
    for tag, m, dev, graphs in (("cpu", cpu, "cpu", False), ("gpu", gpu, "cuda", True)):
        e = _engine(name, m, dev, graphs, max_num_batched_tokens=64)
        outs[tag] = e.generate(prompts, SamplingParams(max_tokens=6))
    # random weights -> near-ties can flip late tokens; the first tokens must agree
    assert [a[0] for a in outs["cpu"]] == [b[0] for b in outs["gpu"]], outs


def test_graph_and_eager_decode_agree():
    _, gpu = _models("tiny-llama")
    prompts = [[1, 7, 8, 9], [1, 30, 31], [1] + list(range(50, 90))]
    res = []
    for graphs in (False, True):
        e = _engine("tiny-llama", gpu, graphs=graphs)
        res.append(e.generate(prompts, SamplingParams(max_tokens=12)))
        if graphs:
            assert e.runner.stats["graph_steps"] > 0
    assert res[0] == res[1]


def test_continuation_steps_match_synchronous_engine():
    _, gpu = _models("tiny-llama-gqa4")
    prompts = [[1] + list(range(5, 5 + n)) for n in (3, 17, 40, 9)]
    params = [SamplingParams(max_tokens=m, temperature=t, seed=7, ignore_eos=True)
              for m, t in ((20, 0.0), (13, 0.8), (31, 0.0), (5, 1.0))]
    res = []
    for overlap in (False, True):
        e = _engine("tiny-llama-gqa4", gpu, overlap=overlap)
        seqs = [e.add_request(p, sp) for p, sp in zip(prompts, params)]
        while e.has_unfinished():
            e.step()
        res.append([s.output_ids for s in seqs])
        if overlap:
            assert e.continuation_steps > 0
        assert e.bm.num_free == e.bm.num_blocks
    assert res[0] == res[1]


def test_contexts_crossing_the_partition_agree_with_eager():
    _, gpu = _models("tiny-llama-gqa4")
    prompts = [[1] + [(7 * i) % 200 + 2 for i in range(n)] for n in (490, 505, 60)]
    res = []
    for graphs in (False, True):
        e = _engine("tiny-llama-gqa4", gpu, graphs=graphs, max_num_batched_tokens=1024, max_model_len=1024)
        res.append(e.generate(prompts, SamplingParams(max_tokens=40, ignore_eos=True)))
        if graphs:
            st = e.runner.stats
            assert 0 < st["short_graph_steps"] < st["graph_steps"], st
    assert res[0] == res[1]


def test_fp8_engine_never_takes_the_fused_qkv_attention_launch(monkeypatch):
    """small-llama (4 kv heads, here 2 layers) takes gemm.qkv_attn_fused with a bf16 cache; with an
    FP8 cache the launch is bypassed (it would write bf16 rows into the byte cache)."""
    calls = []
    real = gemm.qkv_attn_fused
    monkeypatch.setattr(gemm, "qkv_attn_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    prompts = [[1, 7, 8, 9], [1] + list(range(50, 90))]
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    taken = {}
    for dt in ("bf16", "fp8"):
        calls.clear()
        e = LLMEngine(EngineConfig(model="small-llama", num_layers=2, max_num_seqs=8, max_num_batched_tokens=256,
                                   max_model_len=512, hip_graphs=False, device="cuda", kv_cache_dtype=dt),
                      ParallelState(device=torch.device("cuda")))
        out = e.generate(prompts, sp)
        assert [len(o) for o in out] == [6, 6] and (e.runner.kv_caches[0][0].dtype == FP8) == (dt == "fp8")
        taken[dt] = len(calls)
    assert taken["bf16"] > 0, "the bf16 engine no longer takes the fused launch: pick another model"
    assert taken["fp8"] == 0, taken


def test_mixtral_fp8():
    cpu, gpu = _models("tiny-mixtral")
    prompt = [[1] + list(range(5, 45))]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    got = _engine("tiny-mixtral", gpu).generate(prompt, sp)
    exp = _engine("tiny-mixtral", cpu, "cpu", False).generate(prompt, sp)
    assert len(got[0]) == 4 and got[0][0] == exp[0][0], (got, exp)


# ------------------------------------------------------------------------------- TP = 2, one GPU
PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60))]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      LOCAL_RANK="0", POLYKEY_CUSTOM_AR="force")
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=2, device="cuda", backend="gloo")
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=256,
                                 hip_graphs=True, device="cuda:0", kv_cache_dtype="fp8"), st)
    dtypes_ok = all(k.dtype == FP8 and v.dtype == FP8 for k, v in eng.runner.kv_caches)
    if st.tp_rank == 0:
        seqs = [eng.add_request(p, SamplingParams(max_tokens=6, ignore_eos=True)) for p in PROMPTS]
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [s.output_ids for s in seqs], "graph_steps": eng.runner.stats["graph_steps"],
                    "fp8": dtypes_ok}, out_path)
    else:
        eng.runner.worker_loop()
        torch.save({"fp8": dtypes_ok, "blocks": eng.runner.num_blocks}, out_path + ".w")
    destroy_parallel()


def test_tp2_fp8_on_one_gpu(tmp_path):
    """Both ranks allocate FP8 caches, replay graphs, and the first tokens are those of TP = 1."""
    out = str(tmp_path / "tp.pt")
    mp.start_processes(_tp_worker, args=(_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    wk = torch.load(out + ".w", weights_only=True)
    assert got["fp8"] and wk["fp8"] and got["graph_steps"] > 0
    e = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=256,
                               hip_graphs=False, device="cuda", kv_cache_dtype="fp8"),
                  ParallelState(device=torch.device("cuda")))
    exp = e.generate(PROMPTS, SamplingParams(max_tokens=6, ignore_eos=True))
    assert [t[0] for t in got["tokens"]] == [t[0] for t in exp] and all(len(t) == 6 for t in got["tokens"])
