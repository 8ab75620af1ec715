"""Sampling penalties and logit_bias, CPU side: the packed-table reference against a brute-force
loop over Python lists, SamplingParams validation / parsing / wire round trip, the staging-buffer
sections, and the CPU engine (forced tokens, step-by-step replay, device-state audit)."""
import collections
import dataclasses
import math

import numpy as np
import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.engine.model_runner import _Layout
from polykey_service_amd.engine.sequence import SamplingParams
from polykey_service_amd.ops import penalties, sampler
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.parallel.state import ParallelState

f32 = np.float32


def brute(x, prompt, out, r, f, p, bias):
    """The semantics, one token at a time, rounding to fp32 after every operation."""
    y = [f32(v) for v in x]
    for t in range(len(y)):
        if t in prompt or t in out:
            y[t] = f32(y[t] / f32(r)) if y[t] > 0 else f32(y[t] * f32(r))
        c = min(out.count(t), 0x7FFF)
        if c:
            y[t] = f32(f32(y[t] - f32(f32(f) * f32(c))) - f32(p))
    for t, b in bias:
        y[t] = f32(y[t] + f32(b))
    return y


def seed_slot(st, slot, prompt, out, bias=(), clear=1):
    ids = list(prompt) + list(out) + [t for t, _ in bias]
    ids += np.asarray([b for _, b in bias], dtype=np.float32).view(np.int32).tolist()
    entries = torch.tensor([slot, 0, len(prompt), len(out), len(bias), clear], dtype=torch.int32)
    penalties.seed(st, entries, 1, torch.tensor(ids + [0], dtype=torch.int32), len(ids))


def test_reference_matches_brute_force():
    V = 21
    st = penalties.PenaltyState(4, V, "cpu")       # row stride 24: differs from V
    assert st.stride == 24 and st.vocab == V
    prompt = [0, 3, 3, 7, 20]                      # 3: prompt only; 7: both; 0 / V-1: the edges
    out = [7, 9, 9, 9, 20, 5]                      # 9, 5: output only
    bias = [(0, 2.5), (11, -100.0), (20, 0.25)]
    seed_slot(st, 2, prompt, out, bias)
    flags, counts = penalties.read_slot(st, 2)
    assert flags == set(prompt) and counts == dict(collections.Counter(out))
    x = torch.tensor([[1.5, -2.0, 0.0, 3.0, float("-inf"), -1.25, 2.0, -0.5, 1.0, 4.0, 0.5] + [0.75] * 9 + [-3.0],
                      [0.0] * V])
    x[0, 9] = -4.0                                 # negative logit under repetition
    x[0, 5] = float("-inf")                        # -inf stays -inf through every step
    slots = torch.tensor([2, -1], dtype=torch.int32)
    for r, f, p in ((1.3, 0.5, 0.25), (0.5, -1.5, -2.0), (1.0, 0.0, 0.0)):
        rep, fr, pr = (torch.tensor([v, 9.0]) for v in (r, f, p))
        st.out.fill_(float("nan"))
        before = x.clone()
        got = penalties.apply(st, x, slots, rep, fr, pr)
        want = brute(x[0].tolist(), prompt, out, r, f, p, bias)
        assert got[2, :V].numpy().view(np.uint32).tolist() == np.asarray(want, f32).view(np.uint32).tolist()
        assert math.isinf(float(got[2, 5])) and float(got[2, 5]) < 0
        assert torch.isnan(got[[0, 1, 3]]).all() and torch.equal(x, before)
        # the float64 form of the same computation stays within four fp32 roundings
        r64 = ref.penalty_apply(x, st.counts, slots, rep, fr, pr, st.bias_ids, st.bias_vals, st.bias_n,
                                dtype=np.float64)
        fin = np.isfinite(r64[2])
        assert np.all(np.abs(r64[2][fin] - got[2, :V].double().numpy()[fin]) <= 4 * 2.0 ** -24 * 200)


def test_reference_update_saturates_and_keeps_the_prompt_flag():
    st = penalties.PenaltyState(2, 16, "cpu")
    seed_slot(st, 1, [4], [4] * 5)
    st.counts.numpy().view(np.uint16)[1, 4] = 0x8000 | 0x7FFE
    toks = torch.tensor([4, 4], dtype=torch.int32)
    penalties.update(st, torch.tensor([1, -1], dtype=torch.int32), toks, 2)
    assert st.counts.numpy().view(np.uint16)[1, 4] == 0xFFFF
    penalties.update(st, torch.tensor([1, -1], dtype=torch.int32), toks, 2)
    assert st.counts.numpy().view(np.uint16)[1, 4] == 0xFFFF      # saturated, bit 15 kept
    flags, counts = penalties.read_slot(st, 1)
    assert flags == {4} and counts == {4: 0x7FFF}
    x = torch.zeros(1, 16)
    x[0, 4] = 8.0
    got = penalties.apply(st, x, torch.tensor([1], dtype=torch.int32), torch.tensor([2.0]), torch.tensor([2.0 ** -10]),
                          torch.tensor([0.5]))
    assert float(got[1, 4]) == 8.0 / 2 - 2.0 ** -10 * 0x7FFF - 0.5
    before = st.counts.clone()
    penalties.update(st, torch.tensor([5, 1, 0], dtype=torch.int32), torch.tensor([3, 16, -1], dtype=torch.int32), 3)
    assert torch.equal(st.counts, before)                          # bad slot / bad ids write nothing


def test_reference_seed_appends_and_clears():
    st = penalties.PenaltyState(2, 16, "cpu")
    seed_slot(st, 0, [1, 2], [3], [(5, 1.0)])
    seed_slot(st, 0, [], [3, 3, 6], [(7, -2.0)], clear=0)
    flags, counts = penalties.read_slot(st, 0)
    assert flags == {1, 2} and counts == {3: 3, 6: 1}
    assert int(st.bias_n[0]) == 2 and st.bias_ids[0, :2].tolist() == [5, 7] and st.bias_vals[0, :2].tolist() == [1, -2]
    seed_slot(st, 0, [9], [])
    assert penalties.read_slot(st, 0) == ({9}, {}) and int(st.bias_n[0]) == 0


# ---------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("kw", [
    {"frequency_penalty": 2.01}, {"frequency_penalty": -2.5}, {"frequency_penalty": float("nan")},
    {"presence_penalty": 3}, {"presence_penalty": float("inf")}, {"presence_penalty": -2.0001},
    {"repetition_penalty": 0.0}, {"repetition_penalty": -1.0}, {"repetition_penalty": float("inf")},
    {"repetition_penalty": float("nan")},
    {"logit_bias": tuple((i, 0.0) for i in range(301))}, {"logit_bias": ((3, 1.0), (3, 2.0))},
    {"logit_bias": ((3, 100.5),)}, {"logit_bias": ((3, float("nan")),)}, {"logit_bias": ((-1, 1.0),)},
])
def test_sampling_params_rejects(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).validate(128)


def test_sampling_params_accepts_the_edges_and_reports_neutral():
    sp = SamplingParams(frequency_penalty=-2, presence_penalty=2, repetition_penalty=0.01,
                        logit_bias=tuple((i, 100.0 if i % 2 else -100.0) for i in range(300)))
    sp.validate(128)
    assert sp.has_penalties
    assert not SamplingParams().has_penalties and not SamplingParams.from_dict({"max_tokens": 3}).has_penalties
    for kw in ({"repetition_penalty": 1.1}, {"frequency_penalty": 0.1}, {"presence_penalty": -0.1},
               {"logit_bias": ((1, 0.0),)}):
        assert SamplingParams(**kw).has_penalties


def test_from_dict_normalises_logit_bias():
    want = ((3, -1.5), (7, 2.0), (40, 0.0))
    for form in ({"7": 2, "3": -1.5, "40": 0}, {7: 2.0, 3: -1.5, 40: 0}, [[7, 2], [3, -1.5], [40, 0]],
                 {7.0: 2.0, 3.0: -1.5, 40.0: 0.0}):
        sp = SamplingParams.from_dict({"logit_bias": form, "frequency_penalty": 1, "repetition_penalty": 2})
        assert sp.logit_bias == want and all(type(t) is int and type(b) is float for t, b in sp.logit_bias)
        assert sp.frequency_penalty == 1.0 and sp.repetition_penalty == 2.0
        sp.validate(128)
    for bad in ({"a": 1}, {"3": "x"}, [[1]], {"1.5": 1}, {1.5: 1.0}, 7):
        with pytest.raises(ValueError):
            SamplingParams.from_dict({"logit_bias": bad})
    with pytest.raises(ValueError):
        SamplingParams.from_dict({"logit_bias": {"3": 1, 3: 2}}).validate(128)
    with pytest.raises(ValueError):
        SamplingParams.from_dict({"presence_penalty": "1"})


def test_wire_round_trip_keeps_logit_bias():
    import msgpack

    from polykey_service_amd.engine.remote import _params_dict
    sp = SamplingParams.from_dict({"logit_bias": {"9": -3.25, "2": 100}, "presence_penalty": 0.5,
                                   "repetition_penalty": 1.2, "frequency_penalty": -0.5})
    wire = msgpack.unpackb(msgpack.packb(dataclasses.asdict(sp), use_bin_type=True), raw=False)
    back = SamplingParams.from_dict(wire)
    back.validate(128)
    assert SamplingParams.from_dict(msgpack.unpackb(msgpack.packb(_params_dict(sp), use_bin_type=True), raw=False)) == sp
    assert back == sp and back.logit_bias == ((2, 100.0), (9, -3.25))


def test_layout_has_penalty_sections_before_logprobs():
    lay = _Layout(64, 8, 4)
    names = list(lay.sections)
    assert names[-1] == "block_tables" and names[-2] == "logprobs"
    assert names[-6:-2] == ["pen_slot", "rep", "freq", "pres"]
    buf = torch.zeros(lay.size, dtype=torch.int32)
    assert lay.view(buf, "pen_slot").dtype == torch.int32 and lay.view(buf, "pen_slot").shape == (8,)
    for k in ("rep", "freq", "pres"):
        assert lay.view(buf, k).dtype == torch.float32 and lay.view(buf, k).shape == (8,)
        assert lay.sections[k][0] % 16 == 0


# ---------------------------------------------------------------------------- CPU engine
def make_engine(**kw):
    cfg = dict(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=64, max_model_len=256, hip_graphs=False,
               device="cpu")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cpu")))


@pytest.fixture(scope="module")
def engine():
    return make_engine()


def run(e, reqs):
    seqs = [e.add_request(p, sp) for p, sp in reqs]
    while e.has_unfinished():
        e.step()
    return seqs


def test_engine_logit_bias_forces_and_forbids(engine):
    e = engine
    V = e.mcfg.vocab_size
    prompt = [1, 17, 9, 4]
    plain = run(e, [(prompt, SamplingParams(max_tokens=5, ignore_eos=True))])[0].output_ids
    t = (plain[0] + 11) % V
    forced, banned, sampled = run(e, [
        (prompt, SamplingParams(max_tokens=5, ignore_eos=True, logit_bias=((t, 100.0),))),
        (prompt, SamplingParams(max_tokens=5, ignore_eos=True, logit_bias=((plain[0], -100.0),))),
        (prompt, SamplingParams(max_tokens=5, ignore_eos=True, temperature=0.9, seed=4, logit_bias=((t, 100.0),)))])
    assert forced.output_ids == [t] * 5 and sampled.output_ids == [t] * 5
    assert banned.output_ids[0] != plain[0]
    assert run(e, [(prompt, SamplingParams(max_tokens=5, ignore_eos=True))])[0].output_ids == plain
    assert not e.runner._pen_slot and len(e.runner._pen_free) == 8   # every slot came back
    with pytest.raises(ValueError):
        e.add_request(prompt, SamplingParams(logit_bias=((V, 1.0),)))


def test_engine_replay_and_audit(engine):
    e = engine
    e.runner.keep_logits = True
    sp = SamplingParams(max_tokens=12, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5,
                        presence_penalty=0.5)
    prompt = [1, 40, 41, 40, 7]
    s = e.add_request(prompt, sp)
    V = e.mcfg.vocab_size
    try:
        while e.has_unfinished():
            hist = list(s.output_ids)
            e.step()
            raw = e.runner.last_logits[:1].clone()
            st = penalties.PenaltyState(1, V, "cpu")
            seed_slot(st, 0, prompt, hist)
            want = penalties.apply(st, raw, torch.zeros(1, dtype=torch.int32), torch.tensor([1.3]),
                                   torch.tensor([0.5]), torch.tensor([0.5]))
            assert s.output_ids[-1] == int(torch.argmax(want[0, :V]))
            if not s.is_finished():
                flags, counts = e.runner.penalty_state(s)
                assert flags == set(prompt) and counts == dict(collections.Counter(s.output_ids))
    finally:
        e.runner.keep_logits = False
    assert len(s.output_ids) == 12 and e.runner.penalty_state(s) is None
    plain = run(e, [(prompt, SamplingParams(max_tokens=12, ignore_eos=True))])[0]
    assert plain.output_ids != s.output_ids   # the penalties changed what a random tiny model repeats


def test_engine_history_longer_than_one_seed_message():
    e = make_engine(max_num_batched_tokens=32, max_num_seqs=4)
    prompt = [(7 * i + 3) % 50 + 1 for i in range(75)]        # three 32-token chunks; seeds span messages
    bias = tuple((100 + i, 0.5) for i in range(40))           # 80 words: more than one message too
    s = e.add_request(prompt, SamplingParams(max_tokens=3, ignore_eos=True, repetition_penalty=1.2, logit_bias=bias))
    n0 = e.runner.stats["seed_msgs"]
    while e.has_unfinished():
        e.step()
        if not s.is_finished() and s.output_ids:
            flags, counts = e.runner.penalty_state(s)
            assert flags == set(prompt) and counts == dict(collections.Counter(s.output_ids))
            slot = e.runner._pen_slot[s.seq_id]
            assert int(e.runner.pen.bias_n[slot]) == 40
            assert e.runner.pen.bias_ids[slot, :40].tolist() == [t for t, _ in bias]
    assert e.runner.stats["seed_msgs"] - n0 >= 4 and len(s.output_ids) == 3
