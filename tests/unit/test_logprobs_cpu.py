"""Per-token logprobs, CPU side: the float64 reference against torch.log_softmax + stable sort,
SamplingParams validation / parsing, the staging-buffer section, RequestOutput compatibility and
the CPU engine recording one entry per generated token."""
import dataclasses

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.engine.model_runner import _Layout
from polykey_service_amd.engine.sequence import RequestOutput, SamplingParams, Sequence
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.ops import sampler
from polykey_service_amd.parallel.state import ParallelState


def test_reference_matches_log_softmax_and_stable_sort():
    B, V = 10, 4096 + 8
    x = (torch.randn(B, V) * 3).to(torch.bfloat16)  # few distinct values: natural ties
    x[7, :] = 0.5                                   # all equal → ids 0..n-1
    n_top = torch.tensor([-1, 0, 1, 5, 20, 20, 3, 20, 2, 7], dtype=torch.int32)
    tokens = torch.randint(0, V, (B,), dtype=torch.int32)
    tokens[2] = V - 1
    sentinel = 0x5A5A5A5A
    out = ref.logprobs(x, tokens, n_top, torch.full((B, sampler.LOGPROB_WORDS), sentinel, dtype=torch.int32))
    lp, ids, top = sampler.unpack_logprobs(out)
    lsm = torch.log_softmax(x.double(), -1)
    assert torch.equal(out[0], torch.full_like(out[0], sentinel))  # n = -1: untouched
    for b in range(1, B):
        n = int(n_top[b])
        assert abs(float(lp[b]) - float(lsm[b, int(tokens[b])])) < 1e-5
        vals, idx = torch.sort(lsm[b], descending=True, stable=True)
        assert ids[b, :n].tolist() == idx[:n].tolist()
        assert torch.allclose(top[b, :n].double(), vals[:n], atol=1e-5, rtol=0)
        assert ids[b, n:].eq(-1).all() and torch.isneginf(top[b, n:]).all()
    assert ids[7].tolist() == list(range(20))


def test_reference_all_minus_inf_row_has_no_nan():
    x = torch.full((2, 16), float("-inf"))
    x[1, 3] = 1.0
    out = ref.logprobs(x, torch.tensor([5, 3], dtype=torch.int32), torch.tensor([4, 2], dtype=torch.int32))
    lp, ids, top = sampler.unpack_logprobs(out)
    assert torch.isneginf(lp[0]) and torch.isneginf(top[0]).all() and ids[0, :4].tolist() == [0, 1, 2, 3]
    assert float(lp[1]) == 0.0 and ids[1, :2].tolist() == [3, 0] and torch.isneginf(top[1, 1])
    assert not torch.isnan(top).any()


def test_cpu_op_dispatches_to_reference():
    x = torch.randn(3, 64)
    t = torch.tensor([1, 2, 3], dtype=torch.int32)
    n = torch.tensor([2, -1, 0], dtype=torch.int32)
    assert torch.equal(sampler.logprobs(x, t, n), ref.logprobs(x, t, n))
    row = sampler.logprobs(x, t, n)[0].numpy()
    lp, top = sampler.logprob_entry(row, 2)
    assert len(top) == 2 and top[0][1] >= top[1][1] and lp <= 0.0


@pytest.mark.parametrize("v", [0, 1, 20])
def test_sampling_params_accepts(v):
    sp = SamplingParams(logprobs=v)
    sp.validate(128)
    assert SamplingParams.from_dict({"logprobs": v}).logprobs == v
    assert SamplingParams.from_dict({"logprobs": float(v)}).logprobs == v  # gRPC Struct numbers are doubles


@pytest.mark.parametrize("v", [-1, 21, 1.5, "3", True])
def test_sampling_params_rejects(v):
    with pytest.raises(ValueError):
        SamplingParams(logprobs=v).validate(128)


def test_sampling_params_default_is_off():
    assert SamplingParams().logprobs is None and SamplingParams.from_dict({"max_tokens": 3}).logprobs is None
    assert SamplingParams.from_dict({"logprobs": None}).logprobs is None
    SamplingParams().validate(128)
    with pytest.raises(ValueError):
        SamplingParams.from_dict({"logprobs": 2.5})
    assert "logprobs" in dataclasses.asdict(SamplingParams(logprobs=2))


def test_layout_has_logprobs_section_and_block_tables_stay_last():
    lay = _Layout(64, 8, 4)
    names = list(lay.sections)
    assert names[-1] == "block_tables" and names[-2] == "logprobs"
    off, n = lay.sections["logprobs"]
    assert n == 8 and off % 16 == 0
    bt_off, bt_n = lay.sections["block_tables"]
    assert bt_off >= off + n and all(o < bt_off for k, (o, _) in lay.sections.items() if k != "block_tables")
    buf = torch.zeros(lay.size, dtype=torch.int32)
    assert lay.view(buf, "logprobs").dtype == torch.int32 and lay.view(buf, "logprobs").shape == (8,)


def test_request_output_positional_compatibility():
    o = RequestOutput("r", [5], True, "length", 3, 4, {"x": 1})
    assert o.metrics == {"x": 1} and o.logprobs is None
    o = RequestOutput("r", [5], False)
    assert o.logprobs is None
    assert RequestOutput("r", [5], False, logprobs=[(-0.5, [])]).logprobs == [(-0.5, [])]
    assert dataclasses.fields(RequestOutput)[-1].name == "logprobs"


def test_sequence_keeps_a_list_only_when_asked():
    assert Sequence("a", [1, 2], SamplingParams()).logprobs is None
    assert Sequence("b", [1, 2], SamplingParams(logprobs=0)).logprobs == []


def test_cpu_engine_records_one_entry_per_token_and_leaves_tokens_unchanged():
    def run(lps):
        e = LLMEngine(EngineConfig(model="tiny-llama", max_num_seqs=8, max_num_batched_tokens=64, max_model_len=256,
                                   hip_graphs=False, device="cpu"), ParallelState(device=torch.device("cpu")))
        seqs = [e.add_request([1, 5 + i, 9], SamplingParams(max_tokens=4 + i, ignore_eos=True, logprobs=lp,
                                                            temperature=0.8 * (i == 2), seed=3))
                for i, lp in enumerate(lps)]
        outs = []
        while e.has_unfinished():
            outs += e.step()
        return seqs, outs
    seqs, outs = run([None, 0, 3])
    plain, _ = run([None, None, None])
    assert [s.output_ids for s in seqs] == [s.output_ids for s in plain]
    assert seqs[0].logprobs is None and all(o.logprobs is None for o in outs if o.request_id == seqs[0].request_id)
    for s, n in ((seqs[1], 0), (seqs[2], 3)):
        assert len(s.logprobs) == len(s.output_ids)
        for lp, top in s.logprobs:
            assert lp <= 0.0 and len(top) == n and all(v <= 0.0 for _, v in top)
            assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
        mine = [o for o in outs if o.request_id == s.request_id]
        assert sum((o.logprobs for o in mine), []) == s.logprobs
    # greedy row: had it asked for a top list, its head would be the sampled token; here the
    # sampled row (temperature 0.8) only needs its token's logprob to be <= the top one
    for (lp, top) in seqs[2].logprobs:
        assert lp <= top[0][1] + 1e-6
