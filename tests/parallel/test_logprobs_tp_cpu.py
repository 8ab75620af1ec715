"""Per-token logprobs under tensor parallelism on CPU (2 ranks, gloo): the leader reports one
entry per generated token; the worker rank follows the same steps."""
import os
import socket

import torch
import torch.multiprocessing as mp

PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60)), [1, 2]]
ASKS = [3, None, 0]


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
    from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from polykey_service_amd.parallel.state import destroy_parallel, init_parallel
    st = init_parallel(tp=world, ep=1, device="cpu", backend="gloo")
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128,
                                 max_model_len=256, hip_graphs=False, device="cpu"), st)
    if st.tp_rank == 0:
        seqs = [eng.add_request(p, SamplingParams(max_tokens=5, ignore_eos=True, logprobs=lp))
                for p, lp in zip(PROMPTS, ASKS)]
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [s.output_ids for s in seqs], "logprobs": [s.logprobs for s in seqs]}, out_path)
    else:
        eng.runner.worker_loop()
    destroy_parallel()


def test_tp2_logprobs_request_completes(tmp_path):
    out = str(tmp_path / "lp.pt")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    for toks, lps, ask in zip(got["tokens"], got["logprobs"], ASKS):
        assert len(toks) == 5
        if ask is None:
            assert lps is None
            continue
        assert len(lps) == len(toks)
        for tok, (lp, top) in zip(toks, lps):
            assert lp == lp and float("-inf") < lp <= 0.0 and len(top) == ask
            assert all(float("-inf") < v <= 0.0 for _, v in top)
            if ask:  # greedy: the sampled token heads its top list
                assert top[0][0] == tok
