"""Sampling penalties and logit_bias end to end on the GPU: the kernels inside the decode graphs
and the pipelined continuations, next to neutral requests; the device-resident token history is
audited against the host's after every step, through preemption and slot reuse."""
import collections
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import penalties, sampler
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.parallel.state import ParallelState

pytestmark = pytest.mark.gpu

MODEL = "tiny-llama"
PROMPTS = [[1] + list(range(5, 5 + n)) for n in (3, 17, 40, 9, 6, 12)]
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
# neutral greedy, penalised greedy, neutral seeded, penalised seeded, biased greedy, penalised + logprobs
KINDS = [dict(), dict(PEN), dict(temperature=0.8), dict(PEN, temperature=0.8, top_k=50, top_p=0.9),
         dict(logit_bias=((44, 4.0), (45, -100.0))), dict(PEN, logprobs=2)]
NEUTRAL = [0, 2]
ATOL = 1e-4


@pytest.fixture(scope="module")
def gpu_model():
    cpu = build_model(get_config(MODEL), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return gpu


def _engine(model, graphs=True, overlap=True, **kw):
    cfg = dict(model=MODEL, max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, hip_graphs=graphs,
               device="cuda", overlap=overlap)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cuda")), model=model)


def _params(kinds, max_tokens=12):
    return [SamplingParams(max_tokens=max_tokens + i, seed=7, ignore_eos=True, **k) for i, k in enumerate(kinds)]


def _audit(e, seqs):
    """Device history == host history for every live penalised sequence; a step in flight has
    counted exactly one token more per sequence it samples.  Returns how many were checked."""
    torch.cuda.synchronize()
    flying = {s.seq_id for s in e._inflight[1]} if e._inflight is not None else set()
    n = 0
    for s in seqs:
        if s.is_finished() or not s.params.has_penalties:
            continue
        state = e.runner.penalty_state(s)
        if state is None:  # not sampled yet, or preempted: holds no slot
            assert s.seq_id not in flying
            continue
        flags, counts = state
        assert flags == set(s.prompt_ids)
        extra = collections.Counter(counts)
        extra.subtract(collections.Counter(s.output_ids))
        assert all(v >= 0 for v in extra.values()), extra
        assert sum(extra.values()) == (1 if s.seq_id in flying else 0)
        n += 1
    return n


def test_mixed_batch_with_graphs_and_continuations(gpu_model):
    e = _engine(gpu_model)
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(KINDS))]
    audited = 0
    while e.has_unfinished():
        e.step()
        audited += _audit(e, seqs)
    assert e.continuation_steps > 0 and e.runner.stats["graph_steps"] > 0 and audited > 20
    assert not e.runner._pen_slot and len(e.runner._pen_free) == 8
    plain = _engine(gpu_model)
    kinds = [{k: v for k, v in kd.items() if k in ("temperature", "top_k", "top_p", "logprobs")} for kd in KINDS]
    base = [plain.add_request(p, sp) for p, sp in zip(PROMPTS, _params(kinds))]
    while plain.has_unfinished():
        plain.step()
    for i in NEUTRAL:
        assert seqs[i].output_ids == base[i].output_ids, i
    assert 45 not in seqs[4].output_ids  # what the penalised rows must emit is checked step by step below
    assert len(seqs[5].logprobs) == len(seqs[5].output_ids)


def test_replay_each_step_matches_the_reference(gpu_model, monkeypatch):
    """Graphs on, overlap off, every step's raw logits kept: each greedy token equals the argmax of
    the reference applied to that step's raw logits and the sequence's history, and logprobs asked
    alongside still describe the raw logits."""
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")
    e = _engine(gpu_model, overlap=False)
    assert e.runner.debug_logits
    V = e.mcfg.vocab_size
    kinds = [dict(PEN, logprobs=2), dict(), dict(PEN, logit_bias=((60, 3.0), (61, -2.5))), dict(logprobs=0)]
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(kinds, max_tokens=8))]
    by_id = {s.request_id: s for s in seqs}
    checked = 0
    while e.has_unfinished():
        hist = {s.request_id: list(s.output_ids) for s in seqs}
        outs = e.step()
        logits = e.runner.last_logits.float().cpu()
        for r, o in enumerate(outs):
            s = by_id[o.request_id]
            p = s.params
            if p.logprobs is not None:
                want = ref.logprobs(logits[r:r + 1], torch.tensor(o.new_token_ids, dtype=torch.int32),
                                    torch.tensor([p.logprobs], dtype=torch.int32))
                wlp, wtop = sampler.logprob_entry(want[0].numpy(), p.logprobs)
                (lp, top), = o.logprobs
                assert abs(lp - wlp) <= ATOL and [i for i, _ in top] == [i for i, _ in wtop]
            if not p.has_penalties:
                assert o.new_token_ids[0] == int(torch.argmax(logits[r]))
                continue
            st = penalties.PenaltyState(1, V, "cpu")
            bias = list(p.logit_bias)
            ids = s.prompt_ids + hist[o.request_id] + [t for t, _ in bias]
            ids += torch.tensor([b for _, b in bias], dtype=torch.float32).view(torch.int32).tolist()
            penalties.seed(st, torch.tensor([0, 0, len(s.prompt_ids), len(hist[o.request_id]), len(bias), 1],
                                            dtype=torch.int32), 1, torch.tensor(ids, dtype=torch.int32), len(ids))
            want = penalties.apply(st, logits[r:r + 1], torch.zeros(1, dtype=torch.int32),
                                   torch.tensor([p.repetition_penalty]), torch.tensor([p.frequency_penalty]),
                                   torch.tensor([p.presence_penalty]))
            assert o.new_token_ids[0] == int(torch.argmax(want[0, :V])), (o.request_id, len(s.output_ids))
            checked += 1
        _audit(e, seqs)
    assert e.runner.stats["graph_steps"] > 0 and checked >= 2 * 8


def test_preemption_reseeds_on_readmission(gpu_model):
    e = _engine(gpu_model, overlap=False, num_kv_blocks=6, block_size=32)
    prompts = [[1] + list(range(10 + i, 40 + i)) for i in range(4)]
    seqs = [e.add_request(p, SamplingParams(max_tokens=30, ignore_eos=True, **PEN)) for p in prompts]
    audited = 0
    while e.has_unfinished():
        e.step()
        audited += _audit(e, seqs)
    assert e.scheduler.num_preemptions > 0 and audited > 30
    assert all(len(s.output_ids) == 30 for s in seqs)
    assert not e.runner._pen_slot and len(e.runner._pen_free) == 8


def test_slot_reuse_across_waves(gpu_model):
    e = _engine(gpu_model, overlap=True, max_num_seqs=4)
    audited_last = 0
    for wave in range(3):  # 12 penalised requests over 4 slots
        seqs = [e.add_request([1, 7 + wave, 20 + i, 21 + i], SamplingParams(
            max_tokens=6 + i, ignore_eos=True, logit_bias=((30 + wave, 2.0),), **PEN)) for i in range(4)]
        while e.has_unfinished():
            e.step()
            n = _audit(e, seqs)
            audited_last = audited_last + n if wave == 2 else 0
    assert audited_last > 8 and len(e.runner._pen_free) == 4
