"""Guided decoding end to end on the GPU: the mask and advance kernels inside the decode graphs
and the pipelined continuations, next to unguided and penalised requests; the device's automaton
state is audited against the host's walk after every step, through preemption, slot and table
reuse, and with an FP8 KV cache."""
import copy
import json
import re

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import grammar as gram
from polykey_service_amd.ops import penalties
from polykey_service_amd.parallel.state import ParallelState
from tests import grammar_cases as gc

pytestmark = pytest.mark.gpu

MODEL = "tiny-llama"
PROMPTS = [[1] + list(range(5, 5 + n)) for n in (3, 17, 40, 9, 6, 12)]
CHOICES = ["yes", "no", "maybe so"]
REGEX = r"[a-c]{2,4}-[0-9]{2}(\.[0-9])?"
SCHEMA = {"type": "object", "properties": {"city": {"type": "string", "maxLength": 6}, "n": {"type": "integer"},
                                           "ok": {"type": "boolean"}}}
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
# guided greedy choice, unguided greedy, guided seeded regex, penalised unguided, guided + penalised json, unguided seeded
KINDS = [dict(guided_choice=CHOICES), dict(), dict(guided_regex=REGEX, temperature=0.9), dict(PEN),
         dict(guided_json=SCHEMA, presence_penalty=0.3, temperature=0.7), dict(temperature=0.8)]


@pytest.fixture(scope="module")
def gpu_model():
    cpu = build_model(get_config(MODEL), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return gpu


def _engine(model, graphs=True, overlap=True, **kw):
    # 256 words per staging message: every table travels in chunks
    cfg = dict(model=MODEL, max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, hip_graphs=graphs,
               device="cuda", overlap=overlap)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cuda")), model=model)


def _params(kinds, max_tokens=96):  # the longest text of SCHEMA is 87 bytes, and then eos
    return [SamplingParams.from_dict(dict(max_tokens=max_tokens, seed=7, **k)) for k in kinds]


def _ok(s, e):
    p = s.params
    assert s.finish_reason.value == "stop" and s.output_ids[-1] == e.mcfg.eos_token_id, (s.finish_reason, s.output_ids)
    text = e.tokenizer.decode(s.output_ids[:-1])
    if p.guided_choice:
        return text in p.guided_choice
    if p.guided_regex is not None:
        return re.fullmatch(p.guided_regex, text) is not None
    return gc.conforms(json.loads(p.guided_json), json.loads(text))


def _audit(e, seqs):
    """Device state == the host's walk of ``output_ids`` for every live guided sequence; a step in
    flight has advanced by exactly the one id the host has not seen yet, so those are checked
    when the step has landed.  Returns how many were checked."""
    torch.cuda.synchronize()
    flying = {s.seq_id for s in e._inflight[1]} if e._inflight is not None else set()
    n = 0
    for s in seqs:
        if s.is_finished() or s.grammar is None or s.seq_id in flying:
            continue
        st = e.runner.grammar_state(s)
        if st is None:  # not sampled yet, or preempted: holds no slot
            continue
        assert st == (e.runner._gram_seq[s.seq_id], e.runner.grammar_host_state(s)), (s.request_id, st)
        n += 1
    return n


def _drain(e, seqs):
    audited = 0
    while e.has_unfinished():
        e.step()
        audited += _audit(e, seqs)
    return audited


def test_mixed_batch_with_graphs_and_continuations(gpu_model):
    e = _engine(gpu_model)
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(KINDS))]
    _drain(e, seqs)
    assert e.continuation_steps > 0 and e.runner.stats["graph_steps"] > 0
    assert e.runner.stats["grammar_msgs"] > 3  # tables in chunks of 256 words, then slot records
    for i in (0, 2, 4):
        assert _ok(seqs[i], e), e.tokenizer.decode(seqs[i].output_ids)
    assert not e.runner._pen_slot and len(e.runner._pen_free) == 8 and sum(e.runner._gram_ref) == 0
    # (that unguided rows are sampled from their own logits is checked step by step below)


def test_state_equals_the_host_walk_at_every_step(gpu_model):
    e = _engine(gpu_model, overlap=False)
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(KINDS))]
    assert _drain(e, seqs) > 20 and e.runner.stats["graph_steps"] > 0
    assert all(_ok(seqs[i], e) for i in (0, 2, 4))


def test_replay_each_step_matches_the_reference(gpu_model, monkeypatch):
    """Graphs on, overlap off, every step's raw logits kept: each greedy token of a guided row equals
    the argmax of the reference (penalties, then the mask from the host's state) applied to that
    step's raw logits."""
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")
    e = _engine(gpu_model, overlap=False)
    assert e.runner.debug_logits
    V = e.mcfg.vocab_size
    kinds = [dict(guided_choice=CHOICES), dict(), dict(guided_json=SCHEMA, **PEN), dict(guided_regex=REGEX)]
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(kinds))]
    by_id = {s.request_id: s for s in seqs}
    off, data = e.runner.gram.off_np, e.runner.gram.data_np
    checked = 0
    refs = {}
    while e.has_unfinished():
        hist = {s.request_id: list(s.output_ids) for s in seqs}
        outs = e.step()
        logits = e.runner.last_logits.float().cpu()
        for r, o in enumerate(outs):
            s = by_id[o.request_id]
            p = s.params
            if s.grammar is None:
                assert o.new_token_ids[0] == int(torch.argmax(logits[r]))
                continue
            h = hist[o.request_id]
            pst = penalties.PenaltyState(1, V, "cpu")
            ids = s.prompt_ids + h
            penalties.seed(pst, torch.tensor([0, 0, len(s.prompt_ids), len(h), 0, 1], dtype=torch.int32), 1,
                           torch.tensor(ids, dtype=torch.int32), len(ids))
            zero = torch.zeros(1, dtype=torch.int32)
            row = penalties.apply(pst, logits[r:r + 1], zero, torch.tensor([p.repetition_penalty]),
                                  torch.tensor([p.frequency_penalty]), torch.tensor([p.presence_penalty]))
            gst = refs.get(s.seq_id)
            if gst is None:
                gst = refs[s.seq_id] = gram.GrammarState(1, off, data, "cpu", n_tables=1)
                words = torch.from_numpy(gram.pack(s.grammar.cmap, s.grammar.trans, s.grammar.accept))
                gram.load(gst, 0, 0, words, words.numel())
            state = s.grammar.walk(0, b"".join(bytes(data[off[t]:off[t + 1]]) for t in h))
            ends = e.runner.grammar_end_ids(s)
            gram.seed(gst, torch.tensor([0, 0, state, len(ends)] + ends + [-1] * (gram.MAX_END - len(ends)),
                                        dtype=torch.int32), 1)
            gram.mask(gst, row, zero, 1, V)
            assert o.new_token_ids[0] == int(torch.argmax(row[0, :V])), (o.request_id, len(h))
            checked += 1
        _audit(e, seqs)
    assert e.runner.stats["graph_steps"] > 0 and checked >= 20
    assert all(_ok(seqs[i], e) for i in (0, 2, 3))


def test_preemption_reseeds_on_readmission(gpu_model):
    e = _engine(gpu_model, overlap=False, num_kv_blocks=6, block_size=32)
    long_re = r"(ab|cd){40}"
    seqs = [e.add_request([1] + list(range(10 + i, 40 + i)),
                          SamplingParams(max_tokens=100, guided_regex=long_re, temperature=1.0, seed=i))
            for i in range(4)]
    audited = _drain(e, seqs)
    assert e.scheduler.num_preemptions > 0 and audited > 30
    for s in seqs:
        assert _ok(s, e), e.tokenizer.decode(s.output_ids)
    assert not e.runner._pen_slot and len(e.runner._pen_free) == 8 and sum(e.runner._gram_ref) == 0


def test_slot_and_table_reuse_across_waves(gpu_model):
    e = _engine(gpu_model, overlap=True, max_num_seqs=4)
    n_tables = e.runner.gram.n_tables
    for wave in range(3):  # 18 distinct grammars over 16 pool entries and 4 slots; unguided rows take guided slots over
        kinds = [dict(guided_regex=f"[ab]{{{1 + 6 * wave + i}}}", temperature=1.0) for i in range(6)]
        kinds += [dict(PEN, ignore_eos=True), dict(guided_choice=CHOICES)]
        seqs = [e.add_request([1, 7 + wave, 20 + i], sp) for i, sp in enumerate(_params(kinds, max_tokens=30))]
        _drain(e, seqs)
        for s in seqs:
            if s.grammar is not None:
                assert _ok(s, e), e.tokenizer.decode(s.output_ids)
        assert len(seqs[6].output_ids) == 30  # the penalised unguided row was not masked
    assert len(e.runner._pen_free) == 4 and sum(e.runner._gram_ref) == 0
    assert sum(k is not None for k in e.runner._gram_key) == n_tables  # entries were evicted and reused


def test_fp8_kv_engine_serves_a_guided_request(gpu_model):
    e = _engine(gpu_model, kv_cache_dtype="fp8")
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS[:3], _params(KINDS[:3]))]
    _drain(e, seqs)
    assert _ok(seqs[0], e) and _ok(seqs[2], e)
