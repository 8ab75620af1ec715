"""Per-token logprobs under TP=2 on the GPU with decode graphs and pipelined continuations: the
worker rank replays graphs that hold the logprobs kernel (and copies nothing back); the leader
reports one finite entry per generated token."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60)), [1, 2]]
ASKS = [3, None, 0]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      LOCAL_RANK="0", POLYKEY_CUSTOM_AR="force")
    from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=2, device="cuda", backend="gloo")
    assert st.custom_ar is not None, "custom all-reduce did not come up"
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128,
                                 max_model_len=256, hip_graphs=True, device="cuda:0", overlap=True), st)
    assert eng.runner.graphs, "no decode graphs captured"
    if st.tp_rank == 0:
        seqs = [eng.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True, logprobs=lp))
                for p, lp in zip(PROMPTS, ASKS)]
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [s.output_ids for s in seqs], "logprobs": [s.logprobs for s in seqs],
                    "graph_steps": eng.runner.stats["graph_steps"], "cont": eng.continuation_steps,
                    "car_err": st.custom_ar.error()}, out_path)
    else:
        eng.runner.worker_loop()
        torch.save({"worker_steps": eng.runner.stats["steps"]}, out_path + ".w")
    destroy_parallel()


def test_tp2_graphs_logprobs_request_completes(tmp_path):
    out = str(tmp_path / "lp.pt")
    mp.start_processes(_worker, args=(_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    wk = torch.load(out + ".w", weights_only=True)
    assert got["car_err"] == 0 and got["graph_steps"] > 0 and got["cont"] > 0, got
    assert wk["worker_steps"] >= got["graph_steps"]
    for toks, lps, ask in zip(got["tokens"], got["logprobs"], ASKS):
        assert len(toks) == 8
        if ask is None:
            assert lps is None
            continue
        assert len(lps) == len(toks)
        for tok, (lp, top) in zip(toks, lps):
            assert lp == lp and float("-inf") < lp <= 0.0 and len(top) == ask
            assert all(float("-inf") < v <= 0.0 for _, v in top)
            if ask:  # greedy: the sampled token heads its top list
                assert top[0][0] == tok
