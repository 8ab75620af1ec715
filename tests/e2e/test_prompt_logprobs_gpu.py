"""Prompt logprobs on the GPU: tiny-llama-gqa4, HIP graphs on, bf16 and FP8 KV caches, prompts of 33 and
70 tokens prefilled in one chunk and in chunks of 32, the engine stepped by hand.

Structure is checked exactly (lengths, the leading None, rank against the list, rank == 1 exactly where
the list's first id is the token).  Numerics use a twin, because the GPU engine has no all-row logits
to compare against: entry p + 1 of prompt X against the raw logprob of X[p + 1] after the prompt
X[:p + 1], which a request with ``logit_bias {X[p + 1]: 100}``, greedy, ``max_tokens = 1``,
``logprobs = 0`` reports (generated-token logprobs describe the raw logits).  Six positions per prompt.
Bound = max(3 x d_twin, two bf16 ulps at the row's largest |logit|); d_twin is measured on code this
feature does not touch: the twin's first-token logprob prefilled in one chunk against the same prompt
prefilled in chunks of 32 (the factor 3 covers the different launch geometry of a longer prefill, as in
the fork test).  The test prints d_twin, the measured difference and the bound per case.

Measured on an MI355X: see the README section "Prompt logprobs", paragraph "Numerics"."""
import copy
import math

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.parallel.state import ParallelState

pytestmark = pytest.mark.gpu

MODEL = "tiny-llama-gqa4"


@pytest.fixture(scope="module")
def engines():
    """(kv dtype, token budget) -> engine, built once per module.  Several engines are alive and
    stepped in turn here, so each gets its own copy of the (same) weights: an engine packs the
    decode weights of the model it is given anew, and the graphs of an engine built earlier on the
    same model object would keep pointing at the copies that packing released."""
    cpu = build_model(get_config(MODEL), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    cache = {}

    def get(kv, budget):
        if (kv, budget) not in cache:
            gpu_model = copy.deepcopy(cpu).to("cuda")
            gpu_model.device = torch.device("cuda")
            e = LLMEngine(EngineConfig(model=MODEL, max_num_seqs=8, max_num_batched_tokens=budget, max_model_len=256,
                                       hip_graphs=True, graph_batch_sizes=(1, 2, 4, 8), device="cuda", num_kv_blocks=24,
                                       kv_cache_dtype=kv, prefix_caching=False),
                          ParallelState(device=torch.device("cuda")), model=gpu_model)
            assert e.runner.graphs
            e.runner.keep_logits = True
            cache[(kv, budget)] = e
        return cache[(kv, budget)]
    return get


def prompt_of(P):
    return [1] + [(7 + 13 * i) % 200 + 3 for i in range(P - 1)]


def drain(e, limit=200):
    outs = []
    for _ in range(limit):
        if not e.has_unfinished():
            return outs
        outs += e.step()
    raise AssertionError("still unfinished")


def run(e, prompt, sp):
    s = e.add_request(prompt, sp)
    return s, [o for o in drain(e) if o.request_id == s.request_id]


def two_bf16_ulps(x: float) -> float:
    return 2.0 * 2.0 ** (math.floor(math.log2(x)) - 7)


def check_structure(entries, prompt, n):
    assert len(entries) == len(prompt) and entries[0] is None
    for tok, (lp, rank, top) in zip(prompt[1:], entries[1:]):
        assert lp <= 0.0 and rank >= 1 and len(top) == n and len({i for i, _ in top}) == n
        assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
        assert (rank == 1) == (top[0][0] == tok)
        if rank <= n:
            assert top[rank - 1] == (tok, lp)  # the same row, the same lse: bit-equal
        else:
            assert tok not in [i for i, _ in top] and lp <= top[-1][1]


def forced_first_token(e, prefix, tok):
    """-> (raw logprob of ``tok`` after ``prefix``, largest |logit| of that row).  ``prefix`` has at
    least two tokens, so it runs as an eager prefill step, which keeps its logits."""
    e.runner.last_logits = None
    s, _ = run(e, prefix, SamplingParams(max_tokens=1, logprobs=0, logit_bias={tok: 100.0}, ignore_eos=True))
    assert s.output_ids == [tok] and e.runner.last_logits is not None
    return s.logprobs[0][0], float(e.runner.last_logits[0].float().abs().max())


@pytest.mark.parametrize("budget", [256, 32], ids=["one-chunk", "chunks-of-32"])
@pytest.mark.parametrize("P", [33, 70])
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_entries_against_forced_twins(engines, kv, P, budget):
    e, one, chunked = engines(kv, budget), engines(kv, 256), engines(kv, 32)
    prompt = prompt_of(P)
    rows, steps = e.runner.stats["prompt_lp_rows"], e.runner.stats["prompt_lp_steps"]
    s, outs = run(e, prompt, SamplingParams(max_tokens=2, prompt_logprobs=5, logprobs=1, ignore_eos=True))
    got = [o for o in outs if o.prompt_logprobs is not None]
    assert len(got) == 1 and got[0] is outs[0] and len(s.logprobs) == 2
    entries = got[0].prompt_logprobs
    check_structure(entries, prompt, 5)
    assert e.runner.stats["prompt_lp_rows"] - rows == P - 1
    assert e.runner.stats["prompt_lp_steps"] - steps == (-(-(P - 1) // budget))
    worst = (0.0, 0.0, 0.0)
    for i in sorted({2, 3, P // 2, 32 if P > 33 else 17, P - 2, P - 1}):
        a, peak = forced_first_token(one, prompt[:i], prompt[i])
        b, _ = forced_first_token(chunked, prompt[:i], prompt[i])
        d_twin = abs(a - b)
        d = abs(entries[i][0] - a)
        bound = max(3.0 * d_twin, two_bf16_ulps(peak))
        print(f"kv {kv} P {P} budget {budget} entry {i}: d_twin {d_twin:.6g}  |entry - twin| {d:.6g}  "
              f"peak |logit| {peak:.4g}  bound {bound:.6g}")
        assert d <= bound, (i, d, bound)
        worst = max(worst, (d, d_twin, bound))
    print(f"kv {kv} P {P} budget {budget}: largest difference {worst[0]:.6g} (d_twin {worst[1]:.6g}, bound {worst[2]:.6g})")


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_decode_graphs_still_replay_next_to_penalties_and_a_grammar(engines, kv):
    e = engines(kv, 256)
    before = e.runner.stats["graph_steps"]
    ask = e.add_request(prompt_of(70), SamplingParams(max_tokens=6, prompt_logprobs=20, ignore_eos=True))
    other = e.add_request(prompt_of(33), SamplingParams(max_tokens=6, repetition_penalty=1.2, frequency_penalty=0.3,
                                                        logit_bias={5: 3.0}, guided_regex="[a-c]{8,12}"))
    outs = drain(e)
    assert e.runner.stats["graph_steps"] - before >= 5
    assert len(ask.output_ids) == 6 and len(other.output_ids) >= 1
    mine = [o for o in outs if o.request_id == ask.request_id]
    check_structure(mine[0].prompt_logprobs, prompt_of(70), 20)
    assert all(o.prompt_logprobs is None for o in outs if o is not mine[0])
