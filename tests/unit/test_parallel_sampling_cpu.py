"""Parallel sampling (SamplingParams.n) on the CPU engine (tiny-llama, reference ops, stepped by hand):
the structure of the fork, choice 0's identity with the n = 1 request, repeatability, seeds, the
numerics of a forked choice's first token, the fallbacks, abort and preemption
(tests/parallel_sampling_cases.py), validation, and a gloo tp = 2 engine serving n = 2 by the fallback.

Numerics measured here (CPU reference ops): d_twin = 0 and d_fork = 0 exactly, so the bound is the
two-bf16-ulp floor (0.0625 at a largest |logit| of 4); 0 of 24 tokens differ between fork on and off."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.parallel.state import ParallelState
from tests import parallel_sampling_cases as C


def make(**kw):
    cfg = dict(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=256, max_model_len=256, hip_graphs=False,
               device="cpu", num_kv_blocks=24)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState())


def test_structure_of_the_fork():
    C.check_structure(make)


def test_choice0_identity_repeatability_and_seeds():
    C.check_identity_repeatability_seeds(make)


def test_forked_first_token_numerics():
    C.check_numerics(make)


def test_no_free_block_at_fork_time_falls_back():
    C.check_no_block_at_fork_time(make)


def test_kv_fork_off():
    C.check_fork_off(make)


def test_kv_fork_env_switch(monkeypatch):
    monkeypatch.setenv("POLYKEY_KV_FORK", "0")
    assert EngineConfig().kv_fork is False
    monkeypatch.delenv("POLYKEY_KV_FORK")
    assert EngineConfig().kv_fork is True


def test_abort_frees_everything():
    C.check_abort(make)


def test_preempted_forked_choice_recomputes_and_completes():
    C.check_preemption(make)


def test_prompt_completed_over_two_chunks_forks_once():
    e = make(max_num_batched_tokens=48)  # 71 tokens: chunks of 48 and 23; the others stay parked after the first
    s0 = e.add_request(C.prompt_of(71), SamplingParams(max_tokens=3, n=2, ignore_eos=True))
    e.step()
    assert s0.seq_id in e.scheduler.parked and s0.num_computed == 48
    C.drain(e)
    assert e.kv_forks == 1 and s0.choices[1].forked_tokens == 70 and s0.choices[1].output_ids == s0.output_ids


def test_one_token_prompts_and_one_token_chunk_tails_release_the_choices():
    C.check_short_and_chunk_tail_prompts(make)


def test_a_forked_choice_that_loses_its_blocks_is_counted():
    e = make()
    s0 = e.add_request(C.prompt_of(71), SamplingParams(max_tokens=3, n=3, ignore_eos=True))
    C.step_until_forked(e, s0)
    e.scheduler._release_waiting()  # what a preemption of a running sequence does
    assert e.scheduler.num_unforked == 2 and e.scheduler.num_unforked_tokens == 140
    assert all(c.forked_tokens == 0 and c.num_computed == 0 and not e.bm.has(c.seq_id) for c in s0.choices[1:])
    C.step_at_most(e, 20)
    assert all(len(c.output_ids) == 3 for c in s0.choices) and e.bm.num_free == e.bm.num_blocks


def test_request_outputs_carry_the_index_and_metrics():
    e = make()
    e.add_request(C.prompt_of(40), SamplingParams(max_tokens=3, n=3, ignore_eos=True), request_id="r")
    outs = []
    while e.has_unfinished():
        outs += e.step()
    assert {o.request_id for o in outs} == {"r"} and {o.index for o in outs} == {0, 1, 2}
    fin = {o.index: o for o in outs if o.finished}
    assert sorted(fin) == [0, 1, 2] and all(o.finish_reason == "length" and o.num_output_tokens == 3 for o in fin.values())
    assert fin[0].metrics["forked_prompt_tokens"] == 0 and fin[1].metrics["forked_prompt_tokens"] == 39
    assert fin[1].metrics["cached_prompt_tokens"] == 0
    # n = 1: the output and its metrics are what they were
    one = e.add_request(C.prompt_of(40), SamplingParams(max_tokens=2, ignore_eos=True))
    outs = []
    while e.has_unfinished():
        outs += e.step()
    assert one.choices is None and all(o.index == 0 for o in outs) and "forked_prompt_tokens" not in outs[-1].metrics


def test_fork_counters_are_exported():
    from prometheus_client import CollectorRegistry

    from polykey_service_amd.utils.metrics import Metrics
    e = make()
    C.run(e, C.prompt_of(71), SamplingParams(max_tokens=2, n=3, ignore_eos=True))
    reg = CollectorRegistry()
    Metrics(reg).observe_step(e, 0.001, [])
    assert reg.get_sample_value("polykey_engine_kv_forks_total") == 1
    assert reg.get_sample_value("polykey_engine_kv_fork_fallbacks_total") == 0
    assert reg.get_sample_value("polykey_engine_kv_fork_shared_tokens_total") == 140


@pytest.mark.parametrize("bad", [True, "2", 2.5, 0, 17, -1])
def test_invalid_n_is_rejected_by_name(bad):
    with pytest.raises(ValueError, match=r"\bn must be"):
        SamplingParams.from_dict({"n": bad}).validate(256)
    e = make()
    with pytest.raises(ValueError, match=r"\bn must be"):
        e.add_request([1, 2, 3], SamplingParams(n=bad))
    assert not e.has_unfinished()


def test_n_is_capped_by_max_num_seqs_and_integral_floats_pass():
    e = make(max_num_seqs=4)
    with pytest.raises(ValueError, match="max_num_seqs"):
        e.add_request([1, 2, 3], SamplingParams(n=5))
    assert not e.has_unfinished() and not e.scheduler.by_request
    assert SamplingParams.from_dict({"n": 4.0}).n == 4 and SamplingParams.from_dict({}).n == 1
    assert len(C.run(e, [1, 2, 3], SamplingParams(n=4, max_tokens=2))) == 4


def test_guided_choices_share_the_table_and_release_it():
    e = make()
    choices = C.run(e, C.prompt_of(20), SamplingParams(max_tokens=8, temperature=1.0, seed=1, n=3,
                                                       guided_choice=("yes", "no")))
    assert all(e.tokenizer.decode(c.output_ids).strip() in ("yes", "no") or c.finish_reason.value == "length"
               for c in choices)
    assert sum(e.runner._gram_ref) == 0 and not e.runner._gram_seq


# ---------------------------------------------------------------------------- tp = 2 (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(max(1, 8 // world))
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=world, ep=1, device="cpu", backend="gloo")
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128,
                                 max_model_len=256, hip_graphs=False, device="cpu"), st)
    if st.tp_rank == 0:
        s0 = eng.add_request(C.prompt_of(71), SamplingParams(max_tokens=4, n=2, ignore_eos=True))
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [c.output_ids for c in s0.choices], "forks": eng.kv_forks,
                    "fallbacks": eng.kv_fork_fallbacks, "kv_fork": eng.kv_fork}, out_path)
    else:
        eng.runner.worker_loop()
    destroy_parallel()


def test_tp2_serves_n2_through_the_fallback(tmp_path):
    out = str(tmp_path / "n2.pt")
    mp.start_processes(_tp_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    assert got["kv_fork"] is False and got["forks"] == 0 and got["fallbacks"] == 1
    assert len(got["tokens"]) == 2 and all(len(t) == 4 for t in got["tokens"])
    assert got["tokens"][0] == got["tokens"][1]  # greedy
