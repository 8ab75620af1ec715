"""Guided decoding through the CPU engine (the reference functions of ops/reference.py): a tiny
random model with the byte tokenizer never writes well-formed text by itself, so every assertion
on the finished text below fails without the constraint."""
import json
import re

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.engine import grammar as G
from polykey_service_amd.ops import penalties
from polykey_service_amd.parallel.state import ParallelState
from tests import grammar_cases as gc

MODEL = "tiny-llama"
CHOICES = ["yes", "no", "maybe so"]
REGEX = r"[a-c]{2,4}-[0-9]{2}(\.[0-9])?"
SCHEMA = {"type": "object", "properties": {"city": {"type": "string", "maxLength": 6}, "n": {"type": "integer"},
                                           "ok": {"type": "boolean"}}}
PROMPT = [1, 5, 6, 7]


def _engine(**kw):
    cfg = dict(model=MODEL, max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, hip_graphs=False,
               device="cpu")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cpu")))


@pytest.fixture(scope="module")
def engine():
    return _engine()


def _text(e, s):
    assert s.finish_reason.value == "stop", (s.finish_reason, s.output_ids)
    assert s.output_ids[-1] == e.mcfg.eos_token_id
    return e.tokenizer.decode(s.output_ids[:-1])


def _run(e, seqs, audit=True):
    while e.has_unfinished():
        e.step()
        for s in seqs:
            if audit and s.grammar is not None and not s.is_finished():
                st = e.runner.grammar_state(s)
                assert st is None or st[1] == e.runner.grammar_host_state(s)


def _matches(kind, text):
    if kind == "choice":
        return text in CHOICES
    if kind == "regex":
        return re.fullmatch(REGEX, text) is not None
    return gc.conforms(json.loads(SamplingParams.from_dict({"guided_json": SCHEMA}).guided_json), json.loads(text))


def _guided(kind, **kw):
    d = {"choice": dict(guided_choice=CHOICES), "regex": dict(guided_regex=REGEX), "json": dict(guided_json=SCHEMA)}[kind]
    return SamplingParams.from_dict(dict(max_tokens=96, **d, **kw))  # SCHEMA's longest text: 87 bytes


# ------------------------------------------------------------------------------ parameters
def test_sampling_params_validation():
    sp = SamplingParams.from_dict({"guided_json": {"type": "object", "properties": {"b": {"type": "null"},
                                                                                   "a": {"type": "null"}}}})
    assert sp.guided_json == json.dumps(json.loads(sp.guided_json), sort_keys=True) and sp.guided
    assert SamplingParams.from_dict({"guided_json": sp.guided_json}).guided_json == sp.guided_json
    assert SamplingParams.from_dict({"guided_choice": ["a", "b"]}).guided_choice == ("a", "b")
    assert not SamplingParams().guided
    SamplingParams(guided_regex="a+").validate(512)
    for bad, word in ((dict(guided_regex="a", guided_choice=("b",)), "at most one"),
                      (dict(guided_regex="a", guided_json='{"type": "null"}'), "at most one"),
                      (dict(guided_regex="a", ignore_eos=True), "ignore_eos"),
                      (dict(guided_regex=5), "guided_regex"), (dict(guided_choice="ab"), "guided_choice"),
                      (dict(guided_choice=("a", "")), "guided_choice"), (dict(guided_json=7), "guided_json"),
                      (dict(guided_regex="a", stop_token_ids=tuple(range(10, 27))), "stop_token_ids"),
                      (dict(guided_regex="(?=a)"), "lookahead"), (dict(guided_json='{"$ref": "#"}'), "$ref")):
        with pytest.raises(ValueError, match=re.escape(word)):
            SamplingParams(**bad).validate(512)
    assert not SamplingParams.from_dict({"guided_choice": []}).guided  # the unset field, as the wire carries it
    for bad in ({"guided_json": "{"}, {"guided_json": [1]}, {"guided_choice": [""]}, {"guided_regex": 1}):
        with pytest.raises(ValueError):
            SamplingParams.from_dict(bad)


def test_params_cross_the_remote_boundary_unchanged():
    from polykey_service_amd.engine.remote import _params_dict
    sp = _guided("json", temperature=0.5)
    back = SamplingParams(**json.loads(json.dumps(_params_dict(sp))))
    back.validate(512)
    assert (back.guided_json, back.guided_choice, back.guided_regex) == (sp.guided_json, (), None)
    sp = _guided("choice")
    back = SamplingParams(**json.loads(json.dumps(_params_dict(sp))))
    back.validate(512)
    assert back.guided_choice == tuple(CHOICES)


# ---------------------------------------------------------------------------------- engine
def test_neutral_penalty_apply_is_the_float_of_the_logit():
    V = 1024
    st = penalties.PenaltyState(2, V, "cpu")
    ids = torch.arange(0, 600, dtype=torch.int32)  # prompt 0..299 seen, 300..599 generated
    penalties.seed(st, torch.tensor([1, 0, 300, 300, 0, 1], dtype=torch.int32), 1, ids, 600)
    logits = (torch.randn(1, V, generator=torch.Generator().manual_seed(0)) * 20).to(torch.bfloat16)
    logits[0, :4] = torch.tensor([0.0, -0.0, float("inf"), float("-inf")])
    out = penalties.apply(st, logits, torch.tensor([1], dtype=torch.int32), torch.tensor([1.0]), torch.tensor([0.0]),
                          torch.tensor([0.0]))
    assert torch.equal(out[1, :V].view(torch.int32), logits[0].float().view(torch.int32))


@pytest.mark.parametrize("kind", ["choice", "regex", "json"])
def test_greedy_and_seeded_sampling_stay_inside_the_grammar(engine, kind):
    e = engine
    free = e.add_request(PROMPT, SamplingParams(max_tokens=24))
    seqs = [e.add_request(PROMPT, _guided(kind))]
    seqs += [e.add_request(PROMPT, _guided(kind, temperature=1.0, seed=s)) for s in range(20)]
    _run(e, seqs)
    texts = [_text(e, s) for s in seqs]
    assert all(_matches(kind, t) for t in texts), texts
    assert len(set(texts)) > 1  # temperature 1 explores the language
    # what the model writes by itself is nowhere near it
    own = e.tokenizer.decode(free.output_ids)
    with pytest.raises(Exception):
        assert _matches(kind, own)
    assert not e.runner._pen_slot and not e.runner._gram_seq and sum(e.runner._gram_ref) == 0


def test_mixed_batch_leaves_unguided_sequences_alone(engine):
    e = engine
    plain = [dict(max_tokens=20), dict(max_tokens=20, temperature=0.9, seed=5, top_k=40),
             dict(max_tokens=20, repetition_penalty=1.3, frequency_penalty=0.5, logit_bias=((70, 5.0),))]
    prompts = [[1, 9, 8], [1] + list(range(30, 50)), [1, 4]]
    base = [e.add_request(p, SamplingParams(**kw)) for p, kw in zip(prompts, plain)]
    _run(e, base)
    mixed, guided = [], []
    for i, (p, kw) in enumerate(zip(prompts, plain)):
        guided.append(e.add_request(PROMPT, _guided(("choice", "regex", "json")[i], temperature=0.7, seed=i,
                                                    presence_penalty=0.4 * (i == 1))))
        mixed.append(e.add_request(p, SamplingParams(**kw)))
    _run(e, guided)
    assert [s.output_ids for s in mixed] == [s.output_ids for s in base]
    for kind, s in zip(("choice", "regex", "json"), guided):
        assert _matches(kind, _text(e, s))


def test_stop_token_ids_are_end_ids_and_max_tokens_may_cut(engine):
    e = engine
    bang = e.tokenizer.encode("!", add_bos=False)[0]
    s = e.add_request(PROMPT, SamplingParams(max_tokens=32, guided_choice=("yes",), stop_token_ids=(bang,),
                                             logit_bias=((e.mcfg.eos_token_id, -100.0),)))
    cut = e.add_request(PROMPT, SamplingParams(max_tokens=3, guided_regex="a{8}"))
    _run(e, [s, cut])
    assert e.tokenizer.decode(s.output_ids) == "yes!" and s.finish_reason.value == "stop"
    assert e.tokenizer.decode(cut.output_ids) == "aaa" and cut.finish_reason.value == "length"


def test_preemption_keeps_the_constraint():
    e = _engine(num_kv_blocks=6, block_size=32)
    long_re = r"(ab|cd){40}"
    seqs = [e.add_request([1] + list(range(10 + i, 40 + i)), SamplingParams(max_tokens=100, guided_regex=long_re,
                                                                            temperature=1.0, seed=i))
            for i in range(4)]
    _run(e, seqs)
    assert e.scheduler.num_preemptions > 0
    for s in seqs:
        assert re.fullmatch(long_re, _text(e, s))
    assert not e.runner._gram_seq and sum(e.runner._gram_ref) == 0 and len(e.runner._pen_free) == 8


def test_a_17th_distinct_live_grammar_is_refused():
    e = _engine(max_num_seqs=4)
    n = e.runner.gram.n_tables
    assert n == 16
    live = [e.add_request(PROMPT, SamplingParams(max_tokens=4, guided_regex=f"x{{{i + 1}}}")) for i in range(n)]
    twin = e.add_request(PROMPT, SamplingParams(max_tokens=4, guided_regex="x{3}"))  # a shared table is no new one
    with pytest.raises(ValueError, match=f"all {n} grammar tables are held by live sequences"):
        e.add_request(PROMPT, SamplingParams(max_tokens=4, guided_regex="y"))
    assert e.scheduler.num_unfinished() == n + 1
    e.abort(live[0].request_id)  # lets go of its table: the next distinct grammar takes that entry
    late = e.add_request(PROMPT, SamplingParams(max_tokens=4, guided_regex="y"))
    _run(e, live[1:] + [twin, late])
    assert e.tokenizer.decode(late.output_ids[:-1]) == "y" and e.tokenizer.decode(twin.output_ids[:-1]) == "xxx"
    assert sum(e.runner._gram_ref) == 0
    # unreferenced tables stay cached: the same grammar again needs no reload
    msgs = e.runner.stats["grammar_msgs"]
    again = e.add_request(PROMPT, SamplingParams(max_tokens=4, guided_regex="y"))
    _run(e, [again])
    assert e.runner.stats["grammar_msgs"] == msgs + 1  # its slot record only


def test_an_engine_is_freed_by_reference_counting():
    """No reference cycle through the scheduler's on_free hook: an engine that only the cyclic
    collector can free may be torn down in the middle of a later engine's graph capture."""
    import gc
    import weakref
    gc.collect()
    gc.disable()
    try:
        e = _engine()
        s = e.add_request(PROMPT, _guided("choice"))
        _run(e, [s])
        alive = weakref.ref(e)
        del e
        assert alive() is None
    finally:
        gc.enable()


def test_requests_the_engine_cannot_serve_are_value_errors(engine):
    with pytest.raises(ValueError, match="lookbehind"):
        engine.add_request(PROMPT, SamplingParams(guided_regex="(?<=a)b"))
    with pytest.raises(ValueError, match="stop_token_ids"):
        engine.add_request(PROMPT, SamplingParams(guided_regex="a", stop_token_ids=(5000,)))
    small = _engine(model=MODEL)
    small._single_bytes = frozenset(range(0x30, 0x3A))  # a vocabulary with digit bytes only
    with pytest.raises(ValueError, match="single-byte token"):
        small.add_request(PROMPT, SamplingParams(guided_regex="[a-z]+"))
    small.add_request(PROMPT, SamplingParams(guided_regex="[0-9]+"))
