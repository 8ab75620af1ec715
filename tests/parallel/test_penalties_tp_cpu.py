"""Sampling penalties under tensor parallelism on CPU (2 ranks, gloo): penalty slots are seeded by
messages of their own through the step channel, so the worker rank holds the same token history
and follows the same steps; the leader's first tokens equal a single-rank run's."""
import os
import socket

import torch
import torch.multiprocessing as mp

PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60)), [1, 2]]
FORCED = 77


def _params(i):
    from polykey_service_amd.engine import SamplingParams
    if i == 0:
        return SamplingParams(max_tokens=5, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5,
                              presence_penalty=0.5)
    if i == 2:
        return SamplingParams(max_tokens=5, ignore_eos=True, logit_bias=((FORCED, 100.0),))
    return SamplingParams(max_tokens=5, ignore_eos=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(max(1, 8 // world))
    from polykey_service_amd.engine import EngineConfig, LLMEngine
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=world, ep=1, device="cpu", backend="gloo")
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128,
                                 max_model_len=256, hip_graphs=False, device="cpu"), st)
    if st.tp_rank == 0:
        seqs = [eng.add_request(p, _params(i)) for i, p in enumerate(PROMPTS)]
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [s.output_ids for s in seqs], "seed_msgs": eng.runner.stats["seed_msgs"]}, out_path)
    else:
        eng.runner.worker_loop()
        from polykey_service_amd.ops import penalties
        torch.save({"seed_msgs": eng.runner.stats["seed_msgs"],
                    "counted": int((eng.runner.pen.counts & penalties.COUNT_MAX).sum())}, out_path + ".worker")
    destroy_parallel()


def test_tp2_penalised_request_next_to_a_neutral_one(tmp_path):
    out = str(tmp_path / "pen.pt")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    worker = torch.load(out + ".worker", weights_only=True)
    assert [len(t) for t in got["tokens"]] == [5, 5, 5]
    assert got["tokens"][2] == [FORCED] * 5
    assert got["seed_msgs"] >= 1 and worker["seed_msgs"] == got["seed_msgs"]
    assert worker["counted"] == 10  # the worker counted the 2 x 5 tokens its penalised rows sampled

    from polykey_service_amd.engine import EngineConfig, LLMEngine
    from polykey_service_amd.parallel.state import ParallelState
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128,
                                 max_model_len=256, hip_graphs=False, device="cpu"),
                    ParallelState(device=torch.device("cpu")))
    seqs = [eng.add_request(p, _params(i)) for i, p in enumerate(PROMPTS)]
    while eng.has_unfinished():
        eng.step()
    assert [s.output_ids[0] for s in seqs] == [t[0] for t in got["tokens"]]
