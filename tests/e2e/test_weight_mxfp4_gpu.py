"""End-to-end engines with MXFP4 projection weights on the GPU: against the CPU W4 engine (the
reference path quantises and computes the same function), graphs against eager, continuations
against the synchronous loop, a prompt long enough for the wide path against the same prompt in
chunks, the bypass of the bf16-only fused launches, the bytes held, and the combinations with an
FP8 KV cache and with QK-norm (Qwen3)."""
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import gemm, gemm_w4
from polykey_service_amd.parallel.state import ParallelState
from tests.model_cases import NORM_SEED, randomize_norms

pytestmark = pytest.mark.gpu
# norm-weight draws (tests/model_cases.py randomize_norms) per (model, model seed): ones for which the CPU
# engine's first-token top-2 margins stay at least 0.19 of the logits' rms on every prompt of the first-token
# comparisons, the condition the model seeds were chosen by
NORM_SEEDS = {("tiny-llama-gqa4", 6): 42}
FP8 = torch.float8_e4m3fn
MIN_MARGIN = 0.19  # top-2 margin of the reference's logits, in their rms, below which a token may flip


def _models(name, seed=3):
    cpu = build_model(get_config(name), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(seed)
    randomize_norms(cpu, NORM_SEEDS.get((name, seed), NORM_SEED))  # before the copy: both engines share them
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return cpu, gpu


def _engine(name, model, dev="cuda", graphs=True, weight_dtype="mxfp4", **kw):
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512)
    base.update(kw)
    e = LLMEngine(EngineConfig(model=name, hip_graphs=graphs, device=dev, weight_dtype=weight_dtype, **base),
                  ParallelState(device=torch.device(dev)), model=model)
    if weight_dtype == "mxfp4":
        l0 = e.model.layers[0]
        assert e.model.quantised_dtype == "mxfp4" and not e.model.w8 and isinstance(l0.attn.qkv_pf, gemm_w4.W4)
        assert l0.attn.qkv.is_meta and l0.mlp.down.is_meta
    return e


def _first_logits(e, prompt):
    e.runner.keep_logits = True
    e.generate([prompt], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    return e.runner.last_logits.float().cpu().clone()


def _margin(logits):
    top = logits.view(-1).topk(2).values
    return float(top[0] - top[1]) / float(logits.pow(2).mean().sqrt())


@pytest.mark.parametrize("name,kv,seed", [("tiny-llama", "auto", 8), ("tiny-llama-gqa4", "auto", 6),
                                          ("tiny-llama-gqa4", "fp8", 6), ("tiny-qwen3", "auto", 2)])
def test_first_tokens_match_the_cpu_w4_engine(name, kv, seed):
    """Prompts of 3 / 40 / 77 tokens with a 64-token budget: chunked prefill and mixed steps run.
    tiny-llama (hidden 512) takes the general path, tiny-llama-gqa4 and tiny-qwen3 (QK-norm) the
    folded decode chain; ``kv="fp8"``: W4 weights with an FP8 KV cache, against the CPU engine in
    the same mode.  Random weights make near-ties common, so the top-2 margin of the CPU engine's own
    first-token logits is printed and checked first: the seeds are ones for which it is at least
    0.19 of the logits' rms on every prompt."""
    cpu, gpu = _models(name, seed)
    prompts = [[1] + list(range(5, 5 + n)) for n in (3, 40, 77)]
    outs, eng = {}, {}
    for tag, m, dev, graphs in (("cpu", cpu, "cpu", False), ("gpu", gpu, "cuda", True)):
        eng[tag] = e = _engine(name, m, dev, graphs, max_num_batched_tokens=64, kv_cache_dtype=kv)
        assert (e.runner.kv_caches[0][0].dtype == FP8) == (kv == "fp8")
        if tag == "cpu":
            margins = [_margin(_first_logits(e, p)) for p in prompts]
            print(f"{name} kv={kv} seed={seed}: top-2 margins / rms = {[round(v, 3) for v in margins]}")
            assert min(margins) >= MIN_MARGIN, margins
        outs[tag] = e.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
    # the same nibbles and scales on both devices
    for lc, lg in zip(eng["cpu"].model.layers, eng["gpu"].model.layers):
        for a, b in ((lc.attn.qkv_p, lg.attn.qkv_p), (lc.attn.o_p, lg.attn.o_p), (lc.mlp.gate_up_p, lg.mlp.gate_up_p),
                     (lc.mlp.down_p, lg.mlp.down_p)):
            assert torch.equal(a.packed, b.packed.cpu()) and torch.equal(a.scales, b.scales.cpu())
    # random weights -> near-ties can flip late tokens; the first tokens must agree
    assert all(len(o) == 6 for o in outs["gpu"])
    assert [a[0] for a in outs["cpu"]] == [b[0] for b in outs["gpu"]], outs


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-llama-gqa4", "tiny-qwen3"])
def test_graph_and_eager_decode_agree(name):
    _, gpu = _models(name)
    prompts = [[1, 7, 8, 9], [1, 30, 31], [1] + list(range(50, 90))]
    res = []
    for graphs in (False, True):
        e = _engine(name, gpu, graphs=graphs)
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


def test_a_600_token_prompt_takes_the_wide_path_and_agrees_with_chunks(monkeypatch):
    """One 600-row prefill step runs every projection on the wide path (widen, library GEMM);
    chunked at 64 the same prompt runs on the kernel.  Both compute the same function of the same
    dequantised weights, each with one bf16 rounding per projection, in another summation order
    and with the attention over one chunk instead of ten.  The measure and the bound are those of
    tests/e2e/test_weight_fp8_gpu.py: rms of the first-token logits' difference at most 2^-4 of
    their rms, and the same greedy token -- on a seed whose top-2 margin on this prompt (printed,
    checked first) is well above that."""
    _, gpu = _models("tiny-llama-gqa4", 7)
    prompt = [1] + [(7 * i) % 200 + 2 for i in range(599)]
    wide_calls = []
    real = gemm_w4.linear_wide
    monkeypatch.setattr(gemm_w4, "linear_wide", lambda *a, **k: (wide_calls.append(a[0].shape[0]), real(*a, **k))[1])
    whole = _engine("tiny-llama-gqa4", gpu, graphs=False, max_num_batched_tokens=1024, max_model_len=1024)
    lw = _first_logits(whole, prompt)
    assert wide_calls and max(wide_calls) == 600, wide_calls
    assert whole.model.widen_scratch_bytes() == 2 * 4096 * 1024   # the largest projection (gate_up), reserved at set-up
    assert all(h.scratch is whole.model._widen_scratch for l in whole.model.layers
               for h in (l.attn.qkv_p, l.attn.o_p, l.mlp.gate_up_p, l.mlp.down_p))
    wide_calls.clear()
    chunked = _engine("tiny-llama-gqa4", gpu, graphs=False, max_num_batched_tokens=64, max_model_len=1024)
    lc = _first_logits(chunked, prompt)
    assert not wide_calls
    rms = lambda t: float(t.pow(2).mean().sqrt())
    print(f"top-2 margin / rms = {_margin(lc):.3f}; wide vs chunked: rms diff / rms = {rms(lw - lc) / rms(lc):.3e}")
    assert _margin(lc) >= MIN_MARGIN
    assert rms(lw - lc) <= 2.0 ** -4 * rms(lc)
    assert int(lw.argmax()) == int(lc.argmax())


def test_w4_engine_never_takes_the_fused_launches(monkeypatch):
    """At the Llama-3-8B widths (here 2 layers) the bf16 engine's decode takes gemm.qkv_attn_fused
    and gemm.mlp_fused; with MXFP4 weights both are bypassed (they stream bf16 weights)."""
    calls = {"qkv_attn_fused": 0, "mlp_fused": 0}
    for fn in calls:
        real = getattr(gemm, fn)

        def counted(*a, _real=real, _fn=fn, **k):
            calls[_fn] += 1
            return _real(*a, **k)
        monkeypatch.setattr(gemm, fn, counted)
    prompts = [[128000, 1007, 1008, 1009], [128000] + list(range(1050, 1090))]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    taken = {}
    for wd in ("bf16", "mxfp4"):
        for fn in calls:
            calls[fn] = 0
        e = LLMEngine(EngineConfig(model="llama3-8b", num_layers=2, max_num_seqs=8, max_num_batched_tokens=256,
                                   max_model_len=512, num_kv_blocks=64, hip_graphs=False, device="cuda",
                                   prefix_caching=False, weight_dtype=wd), ParallelState(device=torch.device("cuda")))
        out = e.generate(prompts, sp)
        assert [len(o) for o in out] == [4, 4] and (e.model.quantised_dtype == "mxfp4") == (wd == "mxfp4")
        taken[wd] = dict(calls)
        del e
        torch.cuda.empty_cache()
    assert taken["bf16"]["qkv_attn_fused"] > 0 and taken["bf16"]["mlp_fused"] > 0, \
        "the bf16 engine no longer takes the fused launches: pick another model"
    assert taken["mxfp4"] == {"qkv_attn_fused": 0, "mlp_fused": 0}, taken


def test_bytes_held_by_the_layer_tensors():
    _, gpu = _models("tiny-llama-gqa4")
    shapes = [tuple(w.shape) for l in gpu.layers for w in (l.attn.qkv, l.attn.o, l.mlp.gate_up, l.mlp.down)]
    e = _engine("tiny-llama-gqa4", gpu, graphs=False)
    want = sum(n * k // 2 + n * k // 32 for n, k in shapes)
    held = 0
    for l in e.model.layers:
        for h in (l.attn.qkv_p, l.attn.o_p, l.mlp.gate_up_p, l.mlp.down_p):
            assert h.packed.dtype == torch.uint8 and h.scales.dtype == torch.uint8 and h.packed.is_cuda
            held += h.packed.numel() + h.scales.numel()
        # nothing else of the layer holds memory but the two norm vectors and their folded originals
        rest = [p for p in l.parameters() if not p.is_meta]
        assert [p.numel() for p in rest] == [e.model.cfg.hidden_size] * 4
    assert held == want == e.weight_bytes == e.model.projection_bytes()
    print(f"tiny-llama-gqa4: {held} projection bytes with mxfp4, {sum(2 * n * k for n, k in shapes)} in bf16")
