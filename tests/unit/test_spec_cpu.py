"""Speculative decoding on the CPU engine: the n-gram proposer against a brute-force search, draft
reservation, the acceptance rule under scripted proposers, and every refusal.

A scripted proposer drafts from the recorded output of a run without speculation (right, wrong, or
right for ``a`` tokens and then wrong), so what a verify step must emit is known exactly.  Verify and
decode steps feed the model different row counts, so their float32 logits differ in the last bits:
the baseline run first checks that the top-2 margin of every sampled row exceeds 1e-3 of the row's
rms -- four orders above that noise -- which makes equality of greedy tokens a sound demand.
"""
import dataclasses
import random

import pytest
import torch

from polykey_service_amd.config.server_config import load_server_config
from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.engine import spec
from polykey_service_amd.engine.sequence import FinishReason, Sequence
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import attention as attn_ops
from polykey_service_amd.parallel.state import ParallelState

K = 3
V = 1024


# ----------------------------------------------------------------------------- the proposer
def _seq(prompt, out=()):
    s = Sequence("r", list(prompt), SamplingParams())
    s.output_ids = list(out)
    return s


def test_ngram_lookup_definition():
    f = spec.ngram_lookup
    assert f([1, 2, 3, 9, 1, 2, 3], 3, 4, 2) == [9, 1, 2]              # n = 3 wins over n = 2
    assert f([1, 2, 7, 5, 1, 2, 8, 6, 1, 2], 2, 4, 2) == [8, 6]         # the most recent occurrence
    assert f([5, 5, 5, 5], 3, 2, 2) == [5]                              # overlap with the suffix; clipped at L
    assert f([5, 5, 5], 3, 4, 2) == [5]                                 # L < n + 1 for n = 4, 3: n = 2 at i = 0
    assert f([1, 2], 3, 4, 2) == [] and f([7], 3, 4, 2) == [] and f([], 3, 4, 2) == []
    assert f([1, 2, 3, 4, 5, 6], 3, 4, 2) == []                         # no match
    assert f([1, 2, 3, 1, 2], 5, 2, 2) == [3, 1, 2]                     # continuation clipped at L
    assert f([3, 4, 9, 9, 2, 3, 4, 8, 1, 2, 3, 4], 4, 4, 2) == [8, 1, 2, 3]   # n = 4 absent: n = 3 ("2 3 4")
    assert f([1, 2, 3, 1, 2], 0, 4, 2) == []


@pytest.mark.parametrize("kind", ["random", "periodic", "small_alphabet"])
def test_ngram_proposer_matches_the_search(kind):
    """The incremental index, queried as the sequence grows token by token and in jumps (a verify
    step appends several), gives what the search over the whole sequence gives."""
    rng = random.Random(11)
    for trial in range(30):
        n_min = rng.choice([1, 2, 3])
        n_max = n_min + rng.choice([0, 1, 2])
        L = rng.choice([1, 2, 3, 5, 17, 60, 150])
        if kind == "random":
            t = [rng.randrange(50) for _ in range(L)]
        elif kind == "periodic":
            period = [rng.randrange(1000) for _ in range(rng.choice([1, 2, 3, 7]))]
            t = [period[i % len(period)] for i in range(L)]
            for _ in range(L // 20):
                t[rng.randrange(L)] = rng.randrange(1000)
        else:
            t = [rng.randrange(3) for _ in range(L)]
        n_prompt = rng.randrange(1, L + 1)
        p = spec.NgramProposer(n_max, n_min)
        s = _seq(t[:n_prompt])
        n = n_prompt
        while True:
            k = rng.choice([0, 1, 3, 5])
            want = spec.ngram_lookup(t[:n], k, n_max, n_min)
            assert p.propose(s, k) == want, (kind, trial, n, k, n_min, n_max)
            assert p.propose(s, k) == want   # asking twice changes nothing
            if n == L:
                break
            step = min(rng.choice([1, 1, 2, 4]), L - n)
            s.output_ids.extend(t[n:n + step])
            n += step


def test_ngram_proposer_rejects_bad_lengths():
    for lo, hi in ((0, 2), (3, 2)):
        with pytest.raises(ValueError, match="ngram"):
            spec.NgramProposer(hi, lo)
    assert spec.max_draft_tokens(4) == 3 and spec.max_draft_tokens(8) == 1 and spec.max_draft_tokens(1) == 15


# ----------------------------------------------------------------------------- engines
@pytest.fixture(scope="module")
def model_of():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build_model(get_config(name), ParallelState(), torch.float32, torch.device("cpu")).init_random(5)
        return cache[name]
    return get


def make(model_of, name="tiny-llama", speculative=None, **kw):
    cfg = dict(model=name, dtype="float32", max_num_seqs=8, max_num_batched_tokens=256, max_model_len=256,
               num_kv_blocks=96, hip_graphs=False, device="cpu", speculative=speculative, num_speculative_tokens=K)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), ParallelState(device=torch.device("cpu")), model=model_of(name))


PROMPTS = [[1, 40, 41, 42, 43, 44], [1, 7, 8, 9, 7, 8, 9, 7, 8], [1] + list(range(100, 135)), [1, 3]]
GREEDY = dict(max_tokens=14, ignore_eos=True)


@dataclasses.dataclass
class Run:
    tokens: list
    reasons: list
    logprobs: list
    steps: int
    log: list          # per step: (is verify step, [(request index, drafts, tokens emitted)])


def drive(e, prompts, params, check_margin=False, before_step=None) -> Run:
    """Add the requests, step until done; per step the drafts and the tokens every request emitted."""
    if isinstance(params, (dict, SamplingParams)):
        params = [params] * len(prompts)
    seqs = [e.add_request(p, dataclasses.replace(sp) if isinstance(sp, SamplingParams) else SamplingParams(**sp))
            for p, sp in zip(prompts, params)]
    idx = {s.seq_id: i for i, s in enumerate(seqs)}
    e.runner.keep_logits = check_margin
    real, last = e.runner.launch, {}

    def launch(batch):
        last["batch"] = batch
        return real(batch)
    e.runner.launch = launch
    log, emitted_by_outputs = [], {i: [] for i in range(len(seqs))}
    lp_by_outputs = {i: [] for i in range(len(seqs))}
    rid = {s.request_id: i for i, s in enumerate(seqs)}
    try:
        while e.has_unfinished():
            if before_step is not None:
                before_step(e, seqs)
            before = [len(s.output_ids) for s in seqs]
            last.clear()
            outs = e.step()
            for o in outs:
                emitted_by_outputs[rid[o.request_id]].extend(o.new_token_ids)
                if o.logprobs is not None:
                    assert len(o.logprobs) == len(o.new_token_ids)
                    lp_by_outputs[rid[o.request_id]].extend(o.logprobs)
            b = last.get("batch")
            if b is None:
                continue
            drafts = b.drafts if b.drafts is not None else [[] for _ in b.decodes]
            rows = [(idx[s.seq_id], list(d), len(s.output_ids) - before[idx[s.seq_id]])
                    for s, d in zip(b.decodes, drafts) if s.seq_id in idx]
            log.append((b.drafts is not None, rows))
            if check_margin and e.runner.last_logits is not None:
                lg = e.runner.last_logits.double()
                top = lg.topk(2, dim=-1).values
                margin = (top[:, 0] - top[:, 1]) / lg.pow(2).mean(-1).sqrt()
                assert float(margin.min()) > 1e-3, f"near tie in the baseline: margin {float(margin.min()):.2e} of the rms"
    finally:
        del e.runner.launch
    for i, s in enumerate(seqs):   # the outputs carry every token, in order, exactly once
        if s.finish_reason is not FinishReason.ABORT:
            assert emitted_by_outputs[i] == s.output_ids
            if s.logprobs is not None:
                assert lp_by_outputs[i] == s.logprobs and len(s.logprobs) == len(s.output_ids)
    return Run([list(s.output_ids) for s in seqs], [s.finish_reason for s in seqs],
               [s.logprobs for s in seqs], e.step_count, log)


class Script:
    """Drafts from a recorded continuation per prompt: ``right`` leading drafts are the recording's,
    the rest are wrong (the recorded token + 1); None: all right."""

    def __init__(self, prompts, recorded, right=None):
        self.rec = {tuple(p): r for p, r in zip(prompts, recorded)}
        self.right = right
        self.calls = 0

    def propose(self, seq, k):
        self.calls += 1
        full = self.rec[tuple(seq.prompt_ids)]
        n = len(seq.output_ids)
        assert seq.output_ids == full[:n], "the engine left the recorded path"
        d = full[n:n + k]
        if self.right is not None:
            d = [t if j < self.right else (t + 1) % V for j, t in enumerate(d)]
        return d


class Nothing:
    def propose(self, seq, k):
        return []


@pytest.fixture(scope="module")
def baseline(model_of):
    return drive(make(model_of), PROMPTS, GREEDY, check_margin=True)


def spec_engine(model_of, proposer, name="tiny-llama", **kw):
    e = make(model_of, name, speculative="ngram", **kw)
    assert isinstance(e.proposer, spec.NgramProposer) and e.spec_k == K
    e.proposer = proposer
    return e


def test_all_drafts_right(model_of, baseline):
    e = spec_engine(model_of, Script(PROMPTS, baseline.tokens))
    got = drive(e, PROMPTS, GREEDY)
    assert got.tokens == baseline.tokens and got.reasons == baseline.reasons
    assert got.steps < baseline.steps and got.steps <= 2 + (GREEDY["max_tokens"] + K) // (K + 1)
    verify = [rows for is_v, rows in got.log if is_v]
    assert verify
    for rows in verify:
        for _, d, emitted in rows:
            assert emitted == len(d) + 1
    assert e.spec_steps == len(verify)
    assert e.spec_draft_tokens == e.spec_accepted_tokens == sum(len(d) for rows in verify for _, d, _ in rows) > 0
    assert e.total_output_tokens == sum(len(t) for t in baseline.tokens)
    assert all(s.num_pending == 1 or s.is_finished() for s in e.scheduler.running)


def test_all_drafts_wrong(model_of, baseline):
    e = spec_engine(model_of, Script(PROMPTS, baseline.tokens, right=0))
    got = drive(e, PROMPTS, GREEDY)
    assert got.tokens == baseline.tokens and got.steps == baseline.steps
    assert e.spec_accepted_tokens == 0 and e.spec_draft_tokens > 0
    # (the step that samples the last token has no room for a draft: today's decode step)
    assert [is_v for is_v, _ in got.log] == [False] + [True] * (baseline.steps - 2) + [False]
    assert all(emitted == 1 for _, rows in got.log[1:] for _, _, emitted in rows)


@pytest.mark.parametrize("a", range(K + 1))
def test_right_for_a_then_wrong(model_of, baseline, a):
    e = spec_engine(model_of, Script(PROMPTS, baseline.tokens, right=a))
    got = drive(e, PROMPTS, GREEDY)
    assert got.tokens == baseline.tokens
    full = [(d, emitted) for is_v, rows in got.log if is_v for _, d, emitted in rows if len(d) == K]
    assert len(full) >= 4
    for d, emitted in full:
        assert emitted == a + 1          # n_acc == a exactly


def _first_repeat_free(tokens, lo=2):
    """An index >= lo whose token does not occur earlier in the recording."""
    return next(i for i in range(lo, len(tokens)) if tokens[i] not in tokens[:i])


@pytest.mark.parametrize("how", ["stop_token_id", "eos", "max_tokens"])
def test_right_drafts_run_through_the_end(model_of, baseline, how):
    """The script drafts the ignore_eos recording, which runs on past the point where this request
    must end: same tokens, same finish_reason, nothing after the end."""
    cut = [_first_repeat_free(t) for t in baseline.tokens]
    if how == "max_tokens":
        params = [dict(max_tokens=c + 1, ignore_eos=True) for c in cut]
    elif how == "stop_token_id":
        params = [dict(max_tokens=14, ignore_eos=False, stop_token_ids=(t[c],)) for t, c in zip(baseline.tokens, cut)]
    else:
        params = [dict(max_tokens=14) for _ in cut]
    engines = [make(model_of), spec_engine(model_of, Script(PROMPTS, baseline.tokens))]
    runs = []
    for e in engines:
        if how == "eos":   # every request's own end token cannot be eos at once: one request per engine run
            out = []
            for i, (p, c) in enumerate(zip(PROMPTS, cut)):
                e.mcfg = dataclasses.replace(e.mcfg, eos_token_id=baseline.tokens[i][c])
                out.append(drive(e, [p], [params[i]]))
            runs.append(Run([r.tokens[0] for r in out], [r.reasons[0] for r in out], [], 0, []))
        else:
            runs.append(drive(e, PROMPTS, params))
    base, got = runs
    want_reason = FinishReason.LENGTH if how == "max_tokens" else FinishReason.STOP
    for i, c in enumerate(cut):
        assert base.tokens[i] == baseline.tokens[i][:c + 1]
        assert got.tokens[i] == base.tokens[i] and got.reasons[i] == base.reasons[i] == want_reason
    assert engines[1].spec_accepted_tokens > 0


def test_seeded_sampling_uses_row_offsets(model_of):
    params = dict(max_tokens=12, temperature=0.8, top_p=0.9, seed=7, ignore_eos=True)
    base = drive(make(model_of), PROMPTS, params)
    for right in (None, 1):
        got = drive(spec_engine(model_of, Script(PROMPTS, base.tokens, right=right)), PROMPTS, params)
        assert got.tokens == base.tokens and got.steps < base.steps
    other = drive(make(model_of), PROMPTS, dict(params, seed=8))
    assert other.tokens != base.tokens   # the seed matters: equality above is not greedy in disguise


def test_logprobs_one_entry_per_token(model_of):
    params = dict(max_tokens=10, ignore_eos=True, logprobs=3)
    base = drive(make(model_of), PROMPTS, params)
    got = drive(spec_engine(model_of, Script(PROMPTS, base.tokens, right=2)), PROMPTS, params)
    assert got.tokens == base.tokens
    for lg, lb, toks in zip(got.logprobs, base.logprobs, base.tokens):
        assert len(lg) == len(lb) == len(toks)
        for (g, gtop), (b, btop) in zip(lg, lb):
            assert abs(g - b) <= 1e-5
            assert [t for t, _ in gtop] == [t for t, _ in btop] and len(gtop) == 3
            assert all(abs(x - y) <= 1e-5 for (_, x), (_, y) in zip(gtop, btop))


def test_penalised_and_guided_requests_do_not_draft(model_of):
    params = [dict(max_tokens=10, ignore_eos=True),
              dict(max_tokens=10, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.4),
              dict(max_tokens=10, guided_regex="[a-c]{4,12}"),
              dict(max_tokens=10, ignore_eos=True)]
    base = drive(make(model_of), PROMPTS, params)
    rec = {tuple(p): t for p, t in zip(PROMPTS, base.tokens)}
    script = Script(PROMPTS, base.tokens)
    asked = []
    real = script.propose

    def propose(seq, k):
        asked.append(tuple(seq.prompt_ids))
        return real(seq, k)
    script.propose = propose
    e = spec_engine(model_of, script)
    got = drive(e, PROMPTS, params)
    assert got.tokens == base.tokens and got.reasons == base.reasons
    assert set(asked) == {tuple(PROMPTS[0]), tuple(PROMPTS[3])}
    drafted = {i: 0 for i in range(4)}
    for is_v, rows in got.log:
        for i, d, emitted in rows:
            drafted[i] += len(d)
            if i in (1, 2):
                assert d == [] and emitted <= 1
    assert drafted[0] > 0 and drafted[3] > 0 and drafted[1] == drafted[2] == 0
    assert any(is_v for is_v, _ in got.log)


def test_speculative_false_never_drafts(model_of, baseline):
    params = [dict(GREEDY, speculative=False), dict(GREEDY, speculative=True), dict(GREEDY), dict(GREEDY, speculative=False)]
    got = drive(spec_engine(model_of, Script(PROMPTS, baseline.tokens)), PROMPTS, params)
    assert got.tokens == baseline.tokens
    per = {i: sum(len(d) for _, rows in got.log for j, d, _ in rows if j == i) for i in range(4)}
    assert per[0] == per[3] == 0 and per[1] > 0 and per[2] > 0
    # True on an engine without speculation is ignored
    plain = drive(make(model_of), PROMPTS[:2], dict(GREEDY, speculative=True))
    assert plain.tokens == baseline.tokens[:2] and not any(is_v for is_v, _ in plain.log)


def test_abort_while_the_verify_step_is_in_flight(model_of, baseline):
    e = spec_engine(model_of, Script(PROMPTS, baseline.tokens), overlap=True)
    state = {}

    def before_step(e, seqs):
        inflight = e._inflight
        if "done" not in state and inflight is not None and inflight[0].drafts is not None:
            state["done"] = True
            state["len"] = len(seqs[1].output_ids)
            assert e.abort(seqs[1].request_id) is seqs[1]
    got = drive(e, PROMPTS, GREEDY, before_step=before_step)
    assert state.get("done")
    assert got.reasons[1] is FinishReason.ABORT and len(got.tokens[1]) == state["len"]
    for i in (0, 2, 3):
        assert got.tokens[i] == baseline.tokens[i] and got.reasons[i] is FinishReason.LENGTH
    assert e.bm.num_free == e.bm.num_blocks


def test_sixteen_sequences_of_four_rows(model_of):
    prompts = [[1, 20 + i, 21 + 2 * i, 5 + i] for i in range(16)]
    kw = dict(max_num_seqs=16)
    base = drive(make(model_of, **kw), prompts, dict(max_tokens=9, ignore_eos=True), check_margin=True)
    e = spec_engine(model_of, Script(prompts, base.tokens, right=2), **kw)
    rows = []
    real = attn_ops.paged_verify

    def spy(q, *a, **k):
        rows.append(q.shape[0])
        return real(q, *a, **k)
    attn_ops.paged_verify = spy
    try:
        got = drive(e, prompts, dict(max_tokens=9, ignore_eos=True))
    finally:
        attn_ops.paged_verify = real
    assert got.tokens == base.tokens and got.steps < base.steps
    assert max(rows) == 64 and set(rows) <= {4 * n for n in range(1, 17)}


def test_qwen3_all_drafts_right(model_of):
    prompts = PROMPTS[:3]
    base = drive(make(model_of, "tiny-qwen3"), prompts, GREEDY, check_margin=True)
    e = spec_engine(model_of, Script(prompts, base.tokens), "tiny-qwen3")
    got = drive(e, prompts, GREEDY)
    assert got.tokens == base.tokens and got.steps < base.steps and e.spec_accepted_tokens > 0


def test_a_proposer_with_nothing_to_say_changes_nothing(model_of, baseline, monkeypatch):
    calls = []
    real = attn_ops.paged_verify
    monkeypatch.setattr(attn_ops, "paged_verify", lambda *a, **k: calls.append(1) or real(*a, **k))
    e = spec_engine(model_of, Nothing())
    got = drive(e, PROMPTS, GREEDY)
    assert got.tokens == baseline.tokens and got.steps == baseline.steps
    assert not calls and e.runner.stats["verify_steps"] == 0 and e.spec_steps == 0
    assert not any(is_v for is_v, _ in got.log)


def test_the_ngram_proposer_end_to_end(model_of):
    """The real proposer on prompts that repeat: whatever it drafts, the tokens are the baseline's."""
    prompts = [[1] + [50, 51, 52, 53] * 6, [1, 9, 8, 7, 9, 8, 7, 9, 8]]
    base = drive(make(model_of), prompts, dict(max_tokens=24, ignore_eos=True), check_margin=True)
    e = make(model_of, speculative="ngram")
    got = drive(e, prompts, dict(max_tokens=24, ignore_eos=True))
    assert got.tokens == base.tokens and e.spec_draft_tokens > 0
    assert all(len(d) <= K for _, rows in got.log for _, d, _ in rows)


# ----------------------------------------------------------------------------- reservation
def test_drafts_shrink_before_anyone_is_preempted(model_of):
    """A pool one block short: the second sequence's drafts shrink to what its last block holds."""
    prompts = [[1] + list(range(200, 229)), [1] + list(range(300, 329))]      # 30 tokens each
    params = dict(max_tokens=2, ignore_eos=True)
    rec = drive(make(model_of), prompts, dict(max_tokens=8, ignore_eos=True))
    e = spec_engine(model_of, Script(prompts, rec.tokens), num_kv_blocks=3, block_size=32, prefix_caching=False)
    seqs = [e.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True)) for p in prompts]
    seen = []
    real = e.runner.launch

    def launch(batch):
        seen.append(None if batch.drafts is None else [len(d) for d in batch.drafts])
        return real(batch)
    e.runner.launch = launch
    e.step()   # prefill: 31 tokens each, one block each, one block free
    e.step()   # the first verify step
    assert seen == [None, [3, 1]]
    assert e.scheduler.num_preemptions == 0 and all(s.num_preemptions == 0 for s in seqs)
    assert [s.output_ids for s in seqs] == [rec.tokens[0][:5], rec.tokens[1][:3]]


def test_drafts_respect_max_tokens_and_max_model_len(model_of):
    prompt = [1] + list(range(400, 429))            # 30 tokens, max_model_len 40: 11 tokens fit
    kw = dict(max_model_len=40)
    rec = drive(make(model_of, **kw), [prompt], dict(max_tokens=11, ignore_eos=True))
    assert len(rec.tokens[0]) == 11
    longer = rec.tokens[0] + [5, 6, 7, 8]            # the script would go on past the end
    for max_tokens, room in ((11, lambda n: 40 - (30 + n) - 1), (5, lambda n: 5 - n - 1)):
        e = spec_engine(model_of, Script([prompt], [longer]), **kw)
        got = drive(e, [prompt], dict(max_tokens=max_tokens, ignore_eos=True))
        assert got.tokens[0] == rec.tokens[0][:max_tokens] and got.reasons[0] is FinishReason.LENGTH
        n = 1
        for is_v, rows in got.log[1:]:
            (_, d, emitted), = rows
            assert len(d) == max(0, min(K, room(n))), (max_tokens, n, d)
            n += emitted


# ----------------------------------------------------------------------------- refusals, parsing
def _cfg(**kw):
    base = dict(model="tiny-llama", device="cpu", hip_graphs=False, max_num_seqs=4, max_num_batched_tokens=64,
                max_model_len=64, num_kv_blocks=8, speculative="ngram")
    base.update(kw)
    return EngineConfig(**base)


@pytest.mark.parametrize("kw,st,words", [
    (dict(model="tiny-mixtral"), {}, ("speculative=ngram", "MoE")),
    ({}, dict(tp_size=2), ("speculative=ngram", "tp=2")),
    (dict(model="tiny-mixtral"), dict(ep_size=2), ("speculative=ngram",)),
    (dict(kv_cache_dtype="fp8"), {}, ("speculative=ngram", "kv_cache_dtype=fp8")),
    (dict(lora_modules=(("a", "/nowhere"),)), {}, ("speculative=ngram", "LoRA")),
    (dict(num_speculative_tokens=4), {}, ("num_speculative_tokens=4", "largest k for this model is 3")),
    (dict(model="tiny-llama-g8", num_speculative_tokens=2), {}, ("num_speculative_tokens=2", "largest k for this model is 1")),
    (dict(num_speculative_tokens=0), {}, ("num_speculative_tokens",)),
    (dict(speculative="eagle"), {}, ("speculative must be one of ngram",)),
    (dict(ngram_min=3, ngram_max=2), {}, ("ngram_min",)),
])
def test_refusals(kw, st, words):
    with pytest.raises(ValueError) as ei:
        LLMEngine(_cfg(**kw), ParallelState(device=torch.device("cpu"), **st))
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_ep_refusal_names_the_option():
    with pytest.raises(ValueError, match="speculative=ngram does not support ep=2"):
        LLMEngine(_cfg(), ParallelState(device=torch.device("cpu"), ep_size=2))


def test_flags_env_and_engine_config():
    sc = load_server_config([], {})
    assert sc.speculative == "" and sc.num_speculative_tokens == 3 and (sc.ngram_max, sc.ngram_min) == (4, 2)
    ec = EngineConfig.from_server_config(sc)
    assert ec.speculative is None
    sc = load_server_config(["--speculative", "ngram", "--num-speculative-tokens", "2", "--ngram-max", "5", "--ngram-min", "3"], {})
    ec = EngineConfig.from_server_config(sc)
    assert (ec.speculative, ec.num_speculative_tokens, ec.ngram_max, ec.ngram_min) == ("ngram", 2, 5, 3)
    sc = load_server_config(["--speculative", "ngram"], {"POLYKEY_SPECULATIVE": "NGRAM", "POLYKEY_NUM_SPECULATIVE_TOKENS": "1",
                                                         "POLYKEY_NGRAM_MAX": "3", "POLYKEY_NGRAM_MIN": "1"})
    assert (sc.speculative, sc.num_speculative_tokens, sc.ngram_max, sc.ngram_min) == ("ngram", 1, 3, 1)
    for argv, env in ((["--speculative", "medusa"], {}), ([], {"POLYKEY_SPECULATIVE": "draft"}),
                      (["--speculative", "ngram", "--num-speculative-tokens", "0"], {}),
                      (["--speculative", "ngram", "--ngram-min", "5"], {})):
        with pytest.raises(ValueError):
            load_server_config(argv, env)


def test_sampling_params_field():
    assert SamplingParams.from_dict({"speculative": False}).speculative is False
    assert SamplingParams.from_dict({"speculative": True}).speculative is True
    assert SamplingParams.from_dict({}).speculative is None
    for bad in (1, 0, "false", 1.0, [True]):
        with pytest.raises(ValueError, match="speculative must be a boolean"):
            SamplingParams.from_dict({"speculative": bad})
        with pytest.raises(ValueError, match="speculative must be a boolean"):
            SamplingParams(speculative=bad).validate(64)


def test_layout_keeps_its_size_without_speculation():
    from polykey_service_amd.engine.model_runner import _Layout
    a, b = _Layout(256, 8, 8), _Layout(256, 8, 8, max_samples=0)
    assert a.sections == b.sections and a.size == b.size and "verify_rows" not in a.sections
    c = _Layout(256, 8, 8, max_samples=32)
    assert c.sections["sample_idx"][1] == 32 and c.sections["verify_rows"][1] == 8 and c.size > a.size
    assert list(c.sections)[-1] == "block_tables"
