"""Guided decoding under tensor parallelism on CPU (2 ranks, gloo): tables and slot records travel
as messages of their own through the step channel, so the worker rank holds the same tables and
states and follows the same steps; the leader's tokens equal a single-rank run's."""
import os
import re
import socket

import torch
import torch.multiprocessing as mp

PROMPTS = [[1, 5, 6, 7, 8, 9], [1] + list(range(20, 60)), [1, 2]]
REGEX = r"(ab|cd){3}-[0-9]"
CHOICES = ("yes", "no")
CFG = dict(model="tiny-llama-gqa4", max_num_seqs=8, max_num_batched_tokens=128, max_model_len=256, hip_graphs=False,
           device="cpu")


def _params(i):
    from polykey_service_amd.engine import SamplingParams
    if i == 0:
        return SamplingParams(max_tokens=16, guided_regex=REGEX)
    if i == 2:
        return SamplingParams(max_tokens=16, guided_choice=CHOICES)
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
    eng = LLMEngine(EngineConfig(**CFG), st)
    if st.tp_rank == 0:
        seqs = [eng.add_request(p, _params(i)) for i, p in enumerate(PROMPTS)]
        while eng.has_unfinished():
            eng.step()
        eng.runner.stop_workers()
        torch.save({"tokens": [s.output_ids for s in seqs], "msgs": eng.runner.stats["grammar_msgs"],
                    "pool": eng.runner.gram.pool, "rec": eng.runner.gram.rec}, out_path)
    else:
        eng.runner.worker_loop()
        torch.save({"msgs": eng.runner.stats["grammar_msgs"], "pool": eng.runner.gram.pool,
                    "rec": eng.runner.gram.rec}, out_path + ".worker")
    destroy_parallel()


def test_tp2_guided_requests_next_to_a_free_one(tmp_path):
    out = str(tmp_path / "guided.pt")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    worker = torch.load(out + ".worker", weights_only=True)
    # 128 words per message: the two tables went over in several chunks, then the slot records
    assert got["msgs"] >= 4 and worker["msgs"] == got["msgs"]
    assert torch.equal(worker["pool"], got["pool"]) and int((got["pool"][:, 0] > 0).sum()) == 2
    assert torch.equal(worker["rec"], got["rec"]) and int((got["rec"][:, 0] >= 0).sum()) == 2

    from polykey_service_amd.engine import EngineConfig, LLMEngine
    from polykey_service_amd.parallel.state import ParallelState
    eng = LLMEngine(EngineConfig(**CFG), ParallelState(device=torch.device("cpu")))
    eng.runner.keep_logits = True
    seqs = [eng.add_request(p, _params(i)) for i, p in enumerate(PROMPTS)]
    eos, off = eng.mcfg.eos_token_id, eng.tokenizer.offset
    peak = 0.0
    margins = {s.seq_id: [] for s in seqs}  # per step: best minus second-best logit among the admitted ids
    while eng.has_unfinished():
        live = [s for s in seqs if not s.is_finished()]
        states = {s.seq_id: eng.runner.grammar_host_state(s) for s in live if s.grammar is not None}
        eng.step()
        logits = eng.runner.last_logits.float()
        for r, s in enumerate(live):
            ids = list(range(eng.mcfg.vocab_size))
            if s.grammar is not None:
                st = states[s.seq_id]
                ids = [off + b for b in range(256) if s.grammar.step(st, b) >= 0] + ([eos] if s.grammar.accept[st] else [])
            top = torch.topk(logits[r, ids], min(2, len(ids))).values
            margins[s.seq_id].append(float(top[0] - top[-1]) if len(ids) > 1 else float("inf"))
            peak = max(peak, float(top.abs().max()))
    # TP = 2 sums its partial products in another order: the tokens are those of TP = 1, except
    # that after a near-tie of the TP = 1 run's own admitted logits the two runs may part.  The
    # logits are bf16 (8 significant bits) and stay below 8 here, where one ulp is 2^-5: each of
    # the two logits may land one ulp away, so a margin under 2 ulps = 0.0625 is a near-tie
    compared = 0
    for s, theirs in zip(seqs, got["tokens"]):
        for j, (a, b) in enumerate(zip(s.output_ids, theirs)):
            if a != b:
                assert margins[s.seq_id][j] < 0.0625 and peak < 8, (s.request_id, j, a, b, margins[s.seq_id][j])
                break
            compared += 1
        else:
            assert len(theirs) == len(s.output_ids)
    assert compared >= 8
    assert got["tokens"][0][-1] == eos and re.fullmatch(REGEX, eng.tokenizer.decode(got["tokens"][0][:-1]))
    assert got["tokens"][2][-1] == eos and eng.tokenizer.decode(got["tokens"][2][:-1]) in CHOICES
    assert len(got["tokens"][1]) == 5
