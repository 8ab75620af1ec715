"""End-to-end engines with resident LoRA adapters on the GPU, on tiny-llama (hidden 512: the general
path, bf16 add form) and tiny-llama-gqa4 (the folded decode chain, slab add form): a zero-B adapter
is exactly the base model inside a LoRA-form step, base-only traffic runs today's graphs, the GPU
engine agrees with the CPU LoRA engine (the reference ops compute the same function), graphs agree
with eager and continuations with the synchronous loop on a mixed batch, and adapters combine with
an FP8 KV cache.  Adapters come from ``LoraAdapter.random``."""
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.lora import LoraAdapter
from polykey_service_amd.parallel.state import ParallelState
from tests.model_cases import NORM_SEED, randomize_norms

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
NAMES = ["tiny-llama", "tiny-llama-gqa4"]
# model seed per model and the adapters' B scale: chosen on the CPU engine (conditions asserted in
# test_against_the_cpu_lora_engine): every first-token top-2 margin >= 0.19 of the logits' rms and
# every adapter-versus-base distance >= 0.5 of it
SEEDS = {"tiny-llama": 5, "tiny-llama-gqa4": 2, ("tiny-llama", "auto"): 5, ("tiny-llama-gqa4", "auto"): 2,
         ("tiny-llama-gqa4", "fp8"): 2}
B_STD = 0.08
# the norm-weight draws (tests/model_cases.py randomize_norms) chosen with them, by the same conditions
NORM_SEEDS = {("tiny-llama", "auto"): 12, ("tiny-llama-gqa4", "auto"): 4, ("tiny-llama-gqa4", "fp8"): 6}
PROMPTS = [[1] + list(range(5, 5 + n)) for n in (3, 40, 77)]


def adapters(name):
    cfg = get_config(name)
    return (("X", LoraAdapter.random(cfg, rank=8, alpha=16, seed=1, b_std=B_STD)),
            ("Y", LoraAdapter.random(cfg, rank=16, alpha=16, seed=2, b_std=B_STD,
                                     targets=("q", "v", "o", "up", "down"))),
            ("Z", LoraAdapter.random(cfg, rank=4, alpha=8, seed=3, b_std=0.0)))


def models(name, seed=None, norms=NORM_SEED):
    seed = SEEDS[name] if seed is None else seed
    cpu = build_model(get_config(name), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(seed)
    randomize_norms(cpu, norms)  # before the copy: both engines share them
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return cpu, gpu


def engine(name, model, dev="cuda", graphs=True, lora=True, **kw):
    base = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512)
    base.update(kw)
    return LLMEngine(EngineConfig(model=name, hip_graphs=graphs, device=dev,
                                  lora_modules=adapters(name) if lora else (), **base),
                     ParallelState(device=torch.device(dev)), model=model)


def run(e, prompts, loras, max_tokens=6, **sp):
    """-> (output ids per request, first-token logits per request): the logits of the eager
    (prefill) step that sampled each request's first token."""
    e.runner.keep_logits = True
    real, last = e.runner.launch, {}

    def launch(batch):
        last["sampling"] = batch.sampling_seqs()
        return real(batch)
    e.runner.launch = launch
    try:
        seqs = [e.add_request(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True, lora=l, **sp))
                for p, l in zip(prompts, loras)]
        first = {}
        while e.has_unfinished():
            e.runner.last_logits = None
            n_before = {s.seq_id: len(s.output_ids) for s in seqs}
            e.step()
            if e.runner.last_logits is not None:
                lg = e.runner.last_logits.float().cpu()
                for r, s in enumerate(last["sampling"]):
                    if n_before.get(s.seq_id) == 0 and s.seq_id not in first:
                        first[s.seq_id] = lg[r].clone()
    finally:
        del e.runner.launch  # (not "= real": a bound method stored on its own object is a reference cycle,
        #                       and an engine only the cyclic collector frees keeps its graphs alive)
    return [s.output_ids for s in seqs], [first.get(s.seq_id) for s in seqs]


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("name", NAMES)
def test_a_zero_b_adapter_is_exactly_the_base_model(name, monkeypatch):
    """[request 1 on Z (B = 0), request 2 on X] against [request 1 on no adapter, request 2 on X]:
    both steps are LoRA-form, request 1 differs by a delta that is exactly zero.  tiny-llama-gqa4
    runs the LoRA form of the folded chain (slab add form), tiny-llama the general path."""
    from polykey_service_amd.models.llama import LlamaForCausalLM
    chain_calls = []
    real = LlamaForCausalLM._forward_rowscale_lora
    monkeypatch.setattr(LlamaForCausalLM, "_forward_rowscale_lora",
                        lambda self, x, *a, **k: (chain_calls.append(x.shape[0]), real(self, x, *a, **k))[1])
    _, gpu = models(name)
    e = engine(name, gpu)
    assert bool(chain_calls) == (name == "tiny-llama-gqa4")  # (the LoRA graph variants were just captured)
    prompts = [PROMPTS[1], PROMPTS[0]]
    toks_z, lg_z = run(e, prompts, ["Z", "X"])
    toks_b, lg_b = run(e, prompts, [None, "X"])
    assert e.runner.stats["lora_graph_steps"] > 0
    assert torch.equal(lg_z[0], lg_b[0])
    assert toks_z[0] == toks_b[0]
    assert torch.equal(lg_z[1], lg_b[1]) and toks_z[1] == toks_b[1]


@pytest.mark.parametrize("name", NAMES)
def test_base_only_traffic_runs_the_base_graphs(name):
    _, gpu = models(name)
    plain = engine(name, gpu, lora=False)
    want = plain.generate(PROMPTS, SamplingParams(max_tokens=8, ignore_eos=True))
    assert plain.runner.lora is None and "lora_idx" not in plain.runner.layout.sections
    e = engine(name, copy.deepcopy(gpu))
    assert e.runner.lora_graphs and sorted(e.runner.lora_graphs) == sorted(e.runner.graphs)
    got = e.generate(PROMPTS, SamplingParams(max_tokens=8, ignore_eos=True))
    assert got == want
    assert e.runner.stats["graph_steps"] > 0
    assert e.runner.stats["lora_graph_steps"] == 0 and e.runner.stats["lora_steps"] == 0


@pytest.mark.parametrize("name,kv", [("tiny-llama", "auto"), ("tiny-llama-gqa4", "auto"), ("tiny-llama-gqa4", "fp8")])
def test_against_the_cpu_lora_engine(name, kv):
    """Prompts of 3 / 40 / 77 tokens under a 64-token budget (chunked prefill, mixed steps): one
    batch with two different adapters and a base request, then -- in the same engines, the same
    run -- the same prompts all on the base model.  The first tokens of the mixed batch agree; an
    adapter row's GPU logits are closer to the CPU engine's adapter logits than half the CPU
    engine's own adapter-versus-base distance on that prompt; and its GPU-versus-CPU error is at
    most twice the largest base-row GPU-versus-CPU error of the run (the base rows are existing
    code; the LoRA form adds one bf16 rounding per projection)."""
    cpu, gpu = models(name, SEEDS[(name, kv)], NORM_SEEDS[(name, kv)])
    ec = engine(name, cpu, "cpu", graphs=False, kv_cache_dtype=kv)
    eg = engine(name, gpu, kv_cache_dtype=kv)
    assert (eg.runner.kv_caches[0][0].dtype == FP8) == (kv == "fp8")
    loras = ["X", "Y", None]
    (tc, lc), (tg, lg) = run(ec, PROMPTS, loras), run(eg, PROMPTS, loras)
    (_, bc), (_, bg) = run(ec, PROMPTS, [None] * 3), run(eg, PROMPTS, [None] * 3)
    assert eg.runner.stats["lora_graph_steps"] > 0 and eg.runner.stats["lora_steps"] > 0
    for i, l in enumerate(loras):
        top2 = torch.topk(lc[i], 2).values
        assert float(top2[0] - top2[1]) >= 0.19 * rms(lc[i]), (i, "pick another seed: a near-tie on the CPU")
        assert tc[i][0] == tg[i][0], (i, l, tc[i], tg[i])
    if kv == "fp8":  # asked of this combination: it runs and agrees with its CPU twin on first tokens
        return
    err = lambda g, c: rms(g - c) / rms(c)
    base_err = [err(bg[i], bc[i]) for i in range(3)] + [err(lg[2], lc[2])]
    print(f"{name}: base rows' GPU-vs-CPU error / rms = {[f'{v:.2e}' for v in base_err]}")
    for i, l in enumerate(loras[:2]):
        dist = rms(lc[i] - bc[i])
        assert dist >= 0.5 * rms(lc[i]), (i, l, dist / rms(lc[i]), "draw the adapters larger")
        print(f"  adapter {l} prompt {i}: error / rms = {err(lg[i], lc[i]):.2e}, CPU adapter-vs-base distance / rms"
              f" = {dist / rms(lc[i]):.2f}")
        assert rms(lg[i] - lc[i]) < 0.5 * dist, (i, l)
        assert err(lg[i], lc[i]) <= 2.0 * max(base_err), (i, l, err(lg[i], lc[i]), base_err)


@pytest.mark.parametrize("name", NAMES)
def test_graphs_against_eager_and_continuations_against_the_synchronous_loop(name):
    _, gpu = models(name)
    prompts = [[1, 7, 8, 9], [1, 30, 31], [1] + list(range(50, 90)), [1, 60, 61, 62, 63]]
    loras = ["X", None, "Y", "Z"]
    res = {}
    for tag, kw in (("eager", dict(graphs=False)), ("graphs", dict(graphs=True)),
                    ("overlap", dict(graphs=True, overlap=True))):
        e = engine(name, gpu, **kw)
        res[tag], _ = run(e, prompts, loras, max_tokens=12)
        if tag != "eager":
            assert e.runner.stats["lora_graph_steps"] > 0
        if tag == "overlap":
            assert e.continuation_steps > 0
        assert e.bm.num_free == e.bm.num_blocks
    assert res["eager"] == res["graphs"] == res["overlap"]
    # and the adapters matter: the same prompts on the base model give other tokens somewhere
    e = engine(name, gpu)
    base, _ = run(e, prompts, [None] * 4, max_tokens=12)
    assert base != res["graphs"]
