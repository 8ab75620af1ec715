"""Parallel sampling (SamplingParams.n) on the GPU: tiny-llama-gqa4, HIP graphs on, bf16 and FP8 KV
caches, the engine stepped by hand -- the checks of tests/parallel_sampling_cases.py with the fork's
block copy done by pk_kv_copy_blocks and the forked choices' one-row steps replayed from the decode
graphs.

Numerics of a forked choice's first token, measured on an MI355X (top-5 logprobs; d_twin: position P - 1
from the prefill against the same position from a one-row step, on code the fork does not change;
d_fork: choice i >= 1 with the fork against the same request with kv_fork=False; bound = max(3 x d_twin,
two bf16 ulps at the row's largest |logit|)):
    bf16 KV: d_twin = 0.03193, d_fork = 0.03287, bound = 3 x d_twin = 0.09580; 0 of 24 tokens differ fork on / off
    FP8 KV:  d_twin = 0.03313, d_fork = 0.03313, bound = 3 x d_twin = 0.09938; 0 of 24 tokens differ fork on / off"""
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.parallel.state import ParallelState
from tests import parallel_sampling_cases as C

pytestmark = pytest.mark.gpu

MODEL = "tiny-llama-gqa4"


@pytest.fixture(scope="module")
def gpu_model():
    cpu = build_model(get_config(MODEL), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return gpu


@pytest.fixture(params=["bf16", "fp8"])
def make(request, gpu_model):
    def _make(**kw):
        cfg = dict(model=MODEL, max_num_seqs=8, max_num_batched_tokens=256, max_model_len=256, hip_graphs=True,
                   graph_batch_sizes=(1, 2, 4, 8), device="cuda", num_kv_blocks=24, kv_cache_dtype=request.param)
        cfg.update(kw)
        e = LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cuda")), model=gpu_model)
        assert e.runner.graphs and e.kv_fork is cfg.get("kv_fork", True)
        return e
    return _make


def test_structure_of_the_fork(make):
    C.check_structure(make)


def test_choice0_identity_repeatability_and_seeds(make):
    C.check_identity_repeatability_seeds(make)


def test_forked_first_token_numerics(make, monkeypatch):
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")  # graphed steps keep their logits too
    C.check_numerics(make)


def test_no_free_block_at_fork_time_falls_back(make):
    C.check_no_block_at_fork_time(make)


def test_kv_fork_off(make):
    C.check_fork_off(make)


def test_abort_frees_everything(make):
    C.check_abort(make)


def test_preempted_forked_choice_recomputes_and_completes(make):
    C.check_preemption(make)


def test_one_token_prompts_and_one_token_chunk_tails_release_the_choices(make):
    C.check_short_and_chunk_tail_prompts(make)


def test_forked_steps_replay_the_decode_graphs(make):
    e = make()
    before = e.runner.stats["graph_steps"]
    choices = C.run(e, C.prompt_of(71), C.SamplingParams(max_tokens=4, temperature=1.0, seed=1, n=4, ignore_eos=True))
    # 1 prefill step, then 4 decode steps of 4 rows (the forked first tokens ride the first of them)
    assert e.runner.stats["graph_steps"] - before == 4 and e.step_count == 5
    assert all(len(c.output_ids) == 4 for c in choices)
