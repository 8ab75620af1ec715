"""Prompt logprobs (SamplingParams.prompt_logprobs) on the CPU engine (tiny-llama, tiny-qwen3, reference
ops, stepped by hand): the entries against an independent forward over the whole prompt, chunked
prefill, preemption, the prefix-cache rule, n > 1, the combinations that must not change an entry, the
untouched path of requests that do not ask, every refusal, and the remote-engine wire.

Measured here (CPU reference ops): a one-chunk prefill's entries equal the independent computation
exactly (float64 log-softmax of the fp32 logits, rounded to fp32), and are within 1e-5 of
torch.log_softmax in fp32; chunked prefill (chunks of 32, prompts of 5 / 33 / 70 tokens) equals
one-chunk prefill exactly, so no bound is needed there."""
import asyncio
import threading

import msgpack
import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.engine import remote as remote_mod
from polykey_service_amd.engine.async_llm import AsyncLLM
from polykey_service_amd.engine.model_runner import PROMPT_LP_CHUNK_ROWS, _Layout
from polykey_service_amd.engine.remote import EngineServer, RemoteEngine, _params_dict
from polykey_service_amd.engine.sequence import RequestOutput
from polykey_service_amd.parallel.state import ParallelState


def make(**kw):
    cfg = dict(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=256, max_model_len=256, hip_graphs=False,
               device="cpu", num_kv_blocks=24)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState())


def prompt_of(P, base=7):
    return [1] + [(base + 13 * i) % 200 + 3 for i in range(P - 1)]


def drain(e, limit=400):
    outs = []
    for _ in range(limit):
        if not e.has_unfinished():
            return outs
        outs += e.step()
    raise AssertionError("still unfinished")


def run(e, prompt, sp):
    s = e.add_request(prompt, sp)
    outs = [o for o in drain(e) if o.request_id == s.request_id]
    return s, outs


def delivered(outs):
    got = [o.prompt_logprobs for o in outs if o.prompt_logprobs is not None]
    assert len(got) == 1 and outs[0].prompt_logprobs is not None and outs[0].index == 0
    return got[0]


def check_shape(entries, prompt, n):
    assert len(entries) == len(prompt) and entries[0] is None
    for tok, (lp, rank, top) in zip(prompt[1:], entries[1:]):
        assert lp <= 0.0 and rank >= 1 and len(top) == n
        assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
        assert (rank == 1) == (n > 0 and top[0][0] == tok) or n == 0
        if rank <= n:
            assert top[rank - 1] == (tok, lp)
        else:
            assert tok not in [i for i, _ in top]


# ------------------------------------------------------------------ against one eager forward
@pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen3"])
def test_entries_equal_an_independent_forward_over_the_prompt(model):
    e = make(model=model)
    prompt = prompt_of(70)
    hidden = []
    fwd = e.model.forward

    def spy(*a, **k):
        h = fwd(*a, **k)
        hidden.append(h.clone())
        return h
    e.model.forward = spy
    try:
        s, outs = run(e, prompt, SamplingParams(max_tokens=1, prompt_logprobs=5, ignore_eos=True))
    finally:
        del e.model.forward
    entries = delivered(outs)
    check_shape(entries, prompt, 5)
    assert len(hidden) == 1 and hidden[0].shape[0] == 70  # one chunk
    logits = e.model.compute_logits(hidden[0]).float()    # every row at once
    want = torch.log_softmax(logits.double(), -1)
    lsm32 = torch.log_softmax(logits, -1)
    for i in range(1, 70):
        lp, rank, top = entries[i]
        row, t = want[i - 1], prompt[i]
        assert lp == float(row[t].float()), (i, lp, float(row[t]))
        assert abs(lp - float(lsm32[i - 1, t])) <= 1e-5
        x = logits[i - 1]
        assert rank == 1 + int((x > x[t]).sum()) + int((x[:t] == x[t]).sum())
        vals, idx = torch.sort(x, descending=True, stable=True)
        assert [j for j, _ in top] == idx[:5].tolist()
        assert [v for _, v in top] == [float(v) for v in row[idx[:5]].float()]
    assert e.runner.stats["prompt_lp_rows"] == 69 and e.runner.stats["prompt_lp_steps"] == 1
    assert e.prompt_logprob_tokens == 69


# ------------------------------------------------------------------ chunked prefill
_one_chunk = {}


def one_chunk_entries(P, n=3):
    if (P, n) not in _one_chunk:
        _, outs = run(make(), prompt_of(P), SamplingParams(max_tokens=2, prompt_logprobs=n, ignore_eos=True))
        _one_chunk[(P, n)] = delivered(outs)
    return _one_chunk[(P, n)]


@pytest.mark.parametrize("P", [5, 33, 70])
def test_chunked_prefill_equals_one_chunk(P):
    e = make(max_num_batched_tokens=32)
    s, outs = run(e, prompt_of(P), SamplingParams(max_tokens=2, prompt_logprobs=3, ignore_eos=True))
    entries = delivered(outs)
    check_shape(entries, prompt_of(P), 3)
    assert entries == one_chunk_entries(P)  # exact on the CPU reference ops
    assert e.runner.stats["prompt_lp_steps"] == (P - 1 + 31) // 32 and e.runner.stats["prompt_lp_rows"] == P - 1
    assert s.prompt_lp_missing == 0


def test_lm_head_chunks_are_bounded(monkeypatch):
    """More asked rows than PROMPT_LP_CHUNK_ROWS in one step: the LM head never sees more."""
    e = make(max_num_batched_tokens=PROMPT_LP_CHUNK_ROWS + 64, max_model_len=512, num_kv_blocks=32)
    P = PROMPT_LP_CHUNK_ROWS + 40
    seen = []
    real = e.model.compute_logits
    monkeypatch.setattr(e.model, "compute_logits", lambda h: (seen.append(h.shape[0]), real(h))[1])
    _, outs = run(e, prompt_of(P), SamplingParams(max_tokens=1, prompt_logprobs=0, ignore_eos=True))
    entries = delivered(outs)
    check_shape(entries, prompt_of(P), 0)
    assert seen == [PROMPT_LP_CHUNK_ROWS, P - 1 - PROMPT_LP_CHUNK_ROWS, 1]  # two chunks, then the sampling row
    ref = run(make(max_num_batched_tokens=64, max_model_len=512, num_kv_blocks=32), prompt_of(P),
              SamplingParams(max_tokens=1, prompt_logprobs=0, ignore_eos=True))[1]
    assert delivered(ref) == entries


# ------------------------------------------------------------------ preemption
def test_forced_preemption_keeps_entries_and_computes_each_once():
    e = make(num_kv_blocks=8, watermark=0.0, max_num_batched_tokens=32, prefix_caching=False)
    prompts = [prompt_of(70, base=b) for b in (7, 8, 9)]
    seqs = [e.add_request(p, SamplingParams(max_tokens=40, prompt_logprobs=2, ignore_eos=True)) for p in prompts]
    outs = drain(e)
    assert e.scheduler.num_preemptions > 0 and any(s.num_preemptions for s in seqs)
    for s, p in zip(seqs, prompts):
        mine = [o for o in outs if o.request_id == s.request_id]
        entries = delivered(mine)
        check_shape(entries, p, 2)
        assert len(s.output_ids) == 40 and s.prompt_lp_missing == 0
        want = delivered(run(make(), p, SamplingParams(max_tokens=1, prompt_logprobs=2, ignore_eos=True))[1])
        assert entries == want
    # none duplicated, none lost: every entry was computed exactly once across all recomputes
    assert e.prompt_logprob_tokens == e.runner.stats["prompt_lp_rows"] == 3 * 69
    assert e.bm.num_free == 8


def preempt(e, s):
    """What Scheduler._preempt_youngest does to ``s``."""
    sch = e.scheduler
    sch.running.remove(s)
    sch._free(s)
    s.num_computed, s.status = 0, type(s.status).WAITING
    s.num_preemptions += 1
    sch.waiting.appendleft(s)


def test_preemption_in_the_middle_of_a_prefill_recomputes_only_the_missing_entries():
    e = make(max_num_batched_tokens=32, prefix_caching=False)
    s = e.add_request(prompt_of(70), SamplingParams(max_tokens=2, prompt_logprobs=3, ignore_eos=True))
    e.step()
    assert s.num_computed == 32 and s.prompt_lp_missing == 69 - 32
    kept = list(s.prompt_logprobs[1:33])
    preempt(e, s)
    outs = drain(e)
    assert all(a is b for a, b in zip(kept, s.prompt_logprobs[1:33]))  # the recorded entries were kept
    assert delivered(outs) == one_chunk_entries(70)
    assert e.runner.stats["prompt_lp_rows"] == e.prompt_logprob_tokens == 69  # the first 32 rows ran twice, scored once


# ------------------------------------------------------------------ prefix cache
def test_prefix_cache_rule():
    e = make(prefix_caching=True, num_kv_blocks=8, watermark=0.0)
    p = prompt_of(70)
    ask = SamplingParams(max_tokens=2, prompt_logprobs=1, ignore_eos=True)
    first, outs1 = run(e, p, ask)
    second, outs2 = run(e, p, ask)  # the blocks are cached now: an asking request still computes every row
    assert second.num_cached_tokens == 0 and delivered(outs2) == delivered(outs1)
    assert e.scheduler.num_cached_tokens == 0
    third, outs3 = run(e, p, SamplingParams(max_tokens=2, ignore_eos=True))  # does not ask: hits, as ever
    assert third.num_cached_tokens == 64 and all(o.prompt_logprobs is None for o in outs3)
    assert third.output_ids == first.output_ids
    # an asking sequence whose entries are complete matches like any other when it is re-admitted
    a = e.add_request(p, SamplingParams(max_tokens=60, prompt_logprobs=1, ignore_eos=True))
    while len(a.output_ids) < 3:
        e.step()
    assert a.prompt_lp_missing == 0 and a.num_cached_tokens == 0
    rows = e.runner.stats["prompt_lp_rows"]
    sch = e.scheduler                      # preempt it by hand, the way _preempt_youngest does
    sch.running.remove(a)
    sch._free(a)
    a.num_computed, a.status, a.num_preemptions = 0, type(a.status).WAITING, 1
    sch.waiting.appendleft(a)
    e.step()
    assert a.num_computed >= 64 and e.bm.prefix_hits >= 2  # it took its committed blocks back
    drain(e)
    assert len(a.output_ids) == 60 and e.runner.stats["prompt_lp_rows"] == rows


# ------------------------------------------------------------------ n > 1
@pytest.mark.parametrize("fork", [True, False])
def test_only_choice_zero_computes(fork):
    p = prompt_of(70)
    sp = dict(max_tokens=5, temperature=1.0, seed=4, n=3, ignore_eos=True)
    e = make(kv_fork=fork)
    s0 = e.add_request(p, SamplingParams(prompt_logprobs=2, **sp))
    outs = drain(e)
    plain = make(kv_fork=fork)
    q0 = plain.add_request(p, SamplingParams(**sp))
    drain(plain)
    assert [c.output_ids for c in s0.choices] == [c.output_ids for c in q0.choices]
    assert e.runner.stats["prompt_lp_rows"] == 69 and e.kv_forks == plain.kv_forks == int(fork)
    assert [c.prompt_logprobs is not None for c in s0.choices] == [True, False, False]
    got = [o for o in outs if o.prompt_logprobs is not None]
    assert len(got) == 1 and got[0].index == 0 and got[0].new_token_ids == s0.output_ids[:1]
    assert got[0].prompt_logprobs == one_chunk_entries(70, 2)
    if not fork:  # choices >= 1 prefill as plain sequences, with the prefix cache
        assert all(c.num_cached_tokens == 64 for c in s0.choices[1:]) and s0.num_cached_tokens == 0


# ------------------------------------------------------------------ combinations
def test_penalties_bias_grammar_and_logprobs_change_no_entry():
    p = prompt_of(33)
    want = one_chunk_entries(33)
    sp = SamplingParams(max_tokens=4, prompt_logprobs=3, logprobs=2, repetition_penalty=1.3, frequency_penalty=0.5,
                        presence_penalty=-0.5, logit_bias={5: 50.0, 9: -100.0}, guided_regex="[a-c]{2,6}",
                        temperature=0.7, seed=3)
    s, outs = run(make(), p, sp)
    assert delivered(outs) == want
    assert s.logprobs is not None and len(s.logprobs) == len(s.output_ids)
    plain, _ = run(make(), p, SamplingParams(**{**_params_dict(sp), "logit_bias": sp.logit_bias, "prompt_logprobs": None}))
    assert plain.output_ids == s.output_ids and plain.logprobs == s.logprobs  # and asking changes no token


# ------------------------------------------------------------------ the untouched path
PARENT_SECTIONS = ["header", "input_ids", "positions", "slots", "context_lens", "cu_q", "cu_rel", "sample_idx",
                   "temperature", "top_k", "top_p", "min_p", "seeds", "offsets", "pen_slot", "rep", "freq", "pres",
                   "logprobs", "block_tables"]


def test_steps_without_an_asking_row_do_nothing_extra(monkeypatch):
    lay = _Layout(64, 8, 4)
    assert list(lay.sections) == PARENT_SECTIONS  # the staging layout (= the step-channel frame) of the parent
    off = 0
    for name, n in zip(PARENT_SECTIONS, (16, 64, 64, 64, 8, 9, 9) + (8,) * 12 + (32,)):
        assert lay.sections[name] == (off, n)
        off += (n + 15) // 16 * 16
    assert lay.size == off
    e = make(max_num_batched_tokens=32)
    calls = []
    monkeypatch.setattr(e.runner, "_stage_prompt_lp", lambda b: calls.append(b))
    s, outs = run(e, prompt_of(70), SamplingParams(max_tokens=4, logprobs=1, ignore_eos=True))
    assert not calls and e.runner.stats["prompt_lp_steps"] == 0 and e.runner.stats["prompt_lp_rows"] == 0
    assert e.runner._plp_events == [None, None] and e.runner._plp_i == 0
    assert e.runner.plp_dev is None and e.runner._plp_hosts is None  # not even the buffers: made on first use
    assert sum(e.runner.prompt_lp_bytes) > 0  # (their bytes are reserved all the same)
    assert all(o.prompt_logprobs is None for o in outs) and s.prompt_logprobs is None
    # a decode step of an asking request has no asking row either
    monkeypatch.undo()
    a = e.add_request(prompt_of(33), SamplingParams(max_tokens=6, prompt_logprobs=0, ignore_eos=True))
    while not a.output_ids:
        e.step()
    steps = e.runner.stats["prompt_lp_steps"]
    handles = []
    real = e.runner.launch
    monkeypatch.setattr(e.runner, "launch", lambda b: (handles.append(real(b)), handles[-1])[1])
    drain(e)
    assert handles and all(len(h) == 5 for h in handles) and e.runner.stats["prompt_lp_steps"] == steps


def test_request_output_field_is_keyword_only():
    o = RequestOutput("r", [5], True, "length", 3, 4, {"x": 1}, [(-0.5, [])])
    assert o.logprobs == [(-0.5, [])] and o.prompt_logprobs is None and o.index == 0
    with pytest.raises(TypeError):
        RequestOutput("r", [5], True, "length", 3, 4, None, None, [None])
    assert RequestOutput("r", [5], False, prompt_logprobs=[None]).prompt_logprobs == [None]


def test_abort_drops_the_entries():
    e = make(max_num_batched_tokens=32)
    s = e.add_request(prompt_of(70), SamplingParams(max_tokens=4, prompt_logprobs=1), request_id="x")
    e.step()
    assert s.prompt_lp_missing == 69 - 32
    assert e.abort("x") is s and s.prompt_logprobs is None and s.prompt_lp_missing == 0
    assert not e.has_unfinished() and e.bm.num_free == e.bm.num_blocks


def test_one_token_prompt():
    _, outs = run(make(), [1], SamplingParams(max_tokens=2, prompt_logprobs=4, ignore_eos=True))
    assert delivered(outs) == [None]


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [True, False, "3", 1.5, -1, 21])
def test_invalid_values_are_refused_by_name(bad):
    with pytest.raises(ValueError, match="prompt_logprobs must be an integer in \\[0, 20\\]"):
        make_params = SamplingParams(prompt_logprobs=bad)
        make_params.validate(128)
    if not isinstance(bad, int) or isinstance(bad, bool):
        with pytest.raises(ValueError, match="prompt_logprobs must be"):
            SamplingParams.from_dict({"prompt_logprobs": bad})


@pytest.mark.parametrize("v", [0, 1, 20])
def test_valid_values(v):
    SamplingParams(prompt_logprobs=v).validate(128)
    assert SamplingParams.from_dict({"prompt_logprobs": float(v)}).prompt_logprobs == v
    assert SamplingParams().prompt_logprobs is None and SamplingParams.from_dict({"prompt_logprobs": None}).prompt_logprobs is None


def test_parallel_engines_refuse_by_name():
    e = make()
    real = e.st.tp_size
    try:
        e.st.tp_size = 2
        with pytest.raises(ValueError, match="prompt_logprobs does not support tp=2"):
            e.add_request([1, 2, 3], SamplingParams(prompt_logprobs=0))
    finally:
        e.st.tp_size = real
    e.lockstep = True
    with pytest.raises(ValueError, match="prompt_logprobs does not support ep=.* / DP attention"):
        e.add_request([1, 2, 3], SamplingParams(prompt_logprobs=0))
    e.lockstep = False
    e.add_request([1, 2, 3], SamplingParams())  # and nothing else is refused
    assert not e.scheduler.by_request.keys() - {s.key for s in e.scheduler.waiting}


# ------------------------------------------------------------------ remote engine
def test_remote_engine_round_trip_and_frames_of_other_requests(monkeypatch):
    sent = []
    real_send = remote_mod._send

    def spy_send(sock, lock, obj):
        sent.append(msgpack.packb(obj, use_bin_type=True))
        return real_send(sock, lock, obj)
    monkeypatch.setattr(remote_mod, "_send", spy_send)
    llm = AsyncLLM(make(max_num_batched_tokens=32))
    srv = EngineServer(llm)
    th = threading.Thread(target=srv.serve, daemon=True)
    th.start()
    remote = RemoteEngine(("127.0.0.1", srv.port), llm.tokenizer, name="t")
    prompt = prompt_of(40)
    ask = SamplingParams(max_tokens=4, ignore_eos=True, prompt_logprobs=2, logprobs=1)
    plain = SamplingParams(max_tokens=4, ignore_eos=True, logprobs=1)

    async def go():
        local = await llm.generate_all(prompt, ask)
        far = await remote.generate_all(prompt, ask)                      # final-only on the wire
        steps = [o async for o in remote.generate(prompt, ask)]           # per step
        choices = await remote.generate_choices(prompt, SamplingParams(max_tokens=3, ignore_eos=True, n=2,
                                                                       prompt_logprobs=0, temperature=1.0, seed=1))
        mark = len(sent)
        one = await remote.generate_all(prompt, plain, request_id="one")
        return local, far, steps, choices, sent[mark:], one
    try:
        (ltoks, llast), (rtoks, rlast), steps, (ctoks, clast), frames, (otoks, olast) = asyncio.run(go())
    finally:
        remote.shutdown()
        th.join(10)
        llm.shutdown()
    assert rtoks == ltoks and rlast.prompt_logprobs == llast.prompt_logprobs and rlast.logprobs == llast.logprobs
    check_shape(rlast.prompt_logprobs, prompt, 2)
    assert [o.prompt_logprobs is not None for o in steps] == [True] + [False] * (len(steps) - 1)
    assert steps[0].prompt_logprobs == llast.prompt_logprobs
    assert clast[0].prompt_logprobs is not None and clast[1].prompt_logprobs is None and len(clast[0].prompt_logprobs) == 40
    assert not srv._final and not srv._final_lp and not srv._final_plp and not srv._owner
    # the frames of the request that does not ask, byte for byte: built as without the field
    assert "prompt_logprobs" not in _params_dict(plain) and _params_dict(ask)["prompt_logprobs"] == 2
    msgs = [msgpack.unpackb(f, raw=False) for f in frames]
    add = [m for m in msgs if m.get("op") == "add"]
    want_add = {"op": "add", "rid": "one", "prompt": prompt, "params": {
        "max_tokens": 4, "temperature": 0.0, "top_p": 1.0, "top_k": 0, "min_p": 0.0, "seed": None, "stop_token_ids": [],
        "ignore_eos": True, "stop": [], "cache_salt": None, "logprobs": 1, "repetition_penalty": 1.0,
        "frequency_penalty": 0.0, "presence_penalty": 0.0, "logit_bias": [], "guided_regex": None, "guided_choice": [],
        "guided_json": None, "guided_suffix": "", "lora": None, "speculative": None}, "final": True}
    assert len(add) == 1 and msgpack.packb(add[0], use_bin_type=True) == msgpack.packb(want_add, use_bin_type=True)
    items = [it for m in msgs if m.get("op") == "out" for it in m["items"] if it[0] == "one"]
    assert len(items) == 1 and len(items[0]) == 9
    lps = [[lp, [list(t) for t in top]] for lp, top in olast.logprobs]
    assert items[0] == ["one", otoks, True, "length", len(prompt), 4, olast.metrics, None, lps]
