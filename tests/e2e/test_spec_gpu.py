"""Speculative decoding end to end on the GPU, HIP graphs on, against the CPU engine with the same
scripted proposer: ``tiny-llama`` (G = 4, k = 3), ``tiny-llama-g8`` (G = 8, k = 1) and ``tiny-qwen3``
(QK-norm, k = 3).

``tiny-llama-g8`` is the 70B TP = 8 per-rank shape and its vocabulary of 1003 rows is deliberately no
multiple of 8: it has only ever run sharded (padded shards), and on one GPU the sampling-penalty
kernel refuses its logits (``pk_penalty_apply``: V % 8) with or without speculation.  The G = 8 case
here is therefore that preset with 1008 vocabulary rows, registered below as ``tiny-llama-g8-v1008``;
nothing else of the shape changes.

Compared on logits as tests/e2e/test_qwen3_gpu.py compares them, ``d = max|gpu - cpu| / rms(cpu)``,
over the rows of verify steps whose token prefix (prompt, emitted tokens and the drafts before the
row) is the same on both engines.  A verify row passes through the same chain as a decode row with
one different kernel, so the bound is that file's for its decode step: 2^-3 (2^-2 with FP8 weights).

The exact part needs no second engine: from the logits a step kept, every accepted draft is the
greedy choice of the row before it, the extra token is the greedy choice of row ``n_acc``, and the
first rejected draft is not.
"""
import copy
import dataclasses

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.models.config import PRESETS
from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm
from polykey_service_amd.parallel.state import ParallelState
from tests.model_cases import NORM_SEED, randomize_norms

pytestmark = pytest.mark.gpu
BOUND, BOUND_FP8 = 2.0 ** -3, 2.0 ** -2
PROMPTS = [[1] + list(range(5, 5 + n)) for n in (3, 40, 77)]
MAX_TOKENS = 16
G8 = "tiny-llama-g8-v1008"
PRESETS.setdefault(G8, dataclasses.replace(PRESETS["tiny-llama-g8"], name=G8, vocab_size=1008))
K_OF = {"tiny-llama": 3, G8: 1, "tiny-qwen3": 3}
# norm-weight draws (tests/model_cases.py randomize_norms): for G8 one with which the CPU engine's first-token top-2
# margins are at least 0.15 of the logits' rms on every prompt, so that both engines share token prefixes on all three
NORM_SEEDS = {G8: 1}


@pytest.fixture(autouse=True)
def graph_logits(monkeypatch):
    """Graph-replayed steps keep their logits too (a copy captured into each graph, model_runner.py)."""
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")


_MODELS = {}


def models(name):
    if name not in _MODELS:
        _MODELS[name] = randomize_norms(
            build_model(get_config(name), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3),
            NORM_SEEDS.get(name, NORM_SEED))
    cpu = _MODELS[name]
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return copy.deepcopy(cpu), gpu


def engine(name, model, dev="cuda", graphs=True, speculative="ngram", **kw):
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512, speculative=speculative,
                num_speculative_tokens=K_OF[name])
    base.update(kw)
    return LLMEngine(EngineConfig(model=name, hip_graphs=graphs, device=dev, **base),
                     ParallelState(device=torch.device(dev)), model=model)


class Script:
    """Drafts from a recorded continuation: with m = output length + prompt length it proposes
    ``m % (k + 1)`` tokens (0 .. k drafts occur, out of step between the requests), of which the first
    ``m % 3`` are the recording's and the rest are wrong.  A function of (prompt, output length) only:
    both engines get the same drafts wherever their tokens agree."""

    def __init__(self, prompts, recorded, vocab):
        self.rec = {tuple(p): r for p, r in zip(prompts, recorded)}
        self.vocab = vocab

    def propose(self, seq, k):
        n = len(seq.output_ids)
        m = n + len(seq.prompt_ids)
        d = self.rec[tuple(seq.prompt_ids)][n:n + min(k, m % (k + 1))]
        return [t if j < m % 3 else (t + 1) % self.vocab for j, t in enumerate(d)]


class Nothing:
    def propose(self, seq, k):
        return []


def run(e, prompts=PROMPTS, max_tokens=MAX_TOKENS):
    """-> (tokens per request, {(request, prefix tokens): logits row} over verify rows,
    [(drafts, emitted tokens, logits rows)] per (verify step, sequence))."""
    e.runner.keep_logits = True
    real, last = e.runner.launch, {}

    def launch(batch):
        last["batch"] = batch
        return real(batch)
    e.runner.launch = launch
    rows, steps = {}, []
    try:
        seqs = [e.add_request(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True)) for p in prompts]
        idx = {s.seq_id: i for i, s in enumerate(seqs)}
        qr = e.spec_k + 1
        while e.has_unfinished():
            e.runner.last_logits = None
            last.clear()
            before = {s.seq_id: list(s.output_ids) for s in seqs}
            e.step()
            b = last.get("batch")
            if b is None or b.drafts is None:
                continue
            lg = e.runner.last_logits.float().cpu()
            for i, (s, d) in enumerate(zip(b.decodes, b.drafts)):
                out0 = before[s.seq_id]
                mine = lg[i * qr:i * qr + 1 + len(d)].clone()
                for j in range(1 + len(d)):
                    rows[(idx[s.seq_id], tuple(out0 + d[:j]))] = mine[j]
                steps.append((list(d), s.output_ids[len(out0):], mine))
    finally:
        del e.runner.launch
    return [list(s.output_ids) for s in seqs], rows, steps


def dist(a, b):
    return float((a - b).abs().max() / b.double().pow(2).mean().sqrt())


def check_invariant(steps, max_tokens=MAX_TOKENS):
    """Greedy acceptance, exactly, from the step's own logits."""
    n_draft = n_acc_all = 0
    for d, emitted, lg in steps:
        greedy = lg.argmax(dim=-1).tolist()
        n_acc = len(emitted) - 1
        assert 0 <= n_acc <= len(d)
        assert d[:n_acc] == greedy[:n_acc] == emitted[:n_acc], (d, emitted, greedy)
        assert emitted[n_acc] == greedy[n_acc], (d, emitted, greedy)
        if n_acc < len(d):
            assert d[n_acc] != greedy[n_acc], (d, emitted, greedy)
        n_draft += len(d)
        n_acc_all += n_acc
    return n_draft, n_acc_all


def compare(gpu_rows, cpu_rows, bound, what):
    common = sorted(set(gpu_rows) & set(cpu_rows))
    worst = max(dist(gpu_rows[k], cpu_rows[k]) for k in common)
    print(f"\n{what}: {len(common)} verify rows with equal prefixes ({len(gpu_rows)} on the GPU), worst d = {worst:.4f}")
    assert len(common) >= 8 and len({k[0] for k in common}) == len(PROMPTS)
    assert worst <= bound, (what, worst)
    return worst


@pytest.fixture(scope="module")
def cpu_side():
    """Per (model, weight dtype): the CPU recording without speculation and the CPU engine's verify rows."""
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cpu, _ = models(name)
            rec = run(engine(name, cpu, "cpu", False, speculative=None, **kw))[0]
            e = engine(name, cpu, "cpu", False, **kw)
            e.proposer = Script(PROMPTS, rec, e.mcfg.vocab_size)
            cache[key] = (rec, run(e))
        return cache[key]
    return get


class Spy:
    """Which attention launches steps issue, split by whether the step is a verify step."""

    def __init__(self, monkeypatch):
        self.n = dict(verify=0, slab_v=0, rope_v=0, slab=0, rope=0, fused=0, decode_qkv=0, fused_v=0, decode_qkv_v=0,
                      decode=0)
        real = dict(verify=A.paged_verify, slab=gemm.qkv_reduce_rope_cache, fused=gemm.qkv_attn_fused,
                    decode_qkv=A.paged_decode_from_qkv, rope=A.rope_and_cache, attn=A.paged_attention)
        self.in_verify = False
        spy = self

        def verify(q, kc, vc, md, scale, **k):
            spy.n["verify"] += 1
            return real["verify"](q, kc, vc, md, scale, **k)

        def with_md(key, fn, md_at):
            def f(*a, **k):
                md = a[md_at]
                spy.n[key + ("_v" if md.verify_qr > 0 else "")] += 1
                return fn(*a, **k)
            return f

        def by_flag(key, fn):
            def f(*a, **k):
                spy.n[key + ("_v" if spy.in_verify else "")] += 1
                return fn(*a, **k)
            return f

        def attn(*a, **k):
            spy.n["decode"] += 1
            return real["attn"](*a, **k)
        monkeypatch.setattr(A, "paged_verify", verify)
        monkeypatch.setattr(A, "paged_attention", attn)
        monkeypatch.setattr(gemm, "qkv_attn_fused", with_md("fused", real["fused"], 8))
        monkeypatch.setattr(A, "paged_decode_from_qkv", with_md("decode_qkv", real["decode_qkv"], 5))
        monkeypatch.setattr(gemm, "qkv_reduce_rope_cache", by_flag("slab", real["slab"]))
        monkeypatch.setattr(A, "rope_and_cache", by_flag("rope", real["rope"]))

    def watch(self, e):
        """Mark the launches of verify steps (the slab writer and rope_and_cache take no metadata)."""
        real = e.runner._run
        spy = self

        def _run(*a, **k):
            spy.in_verify = bool(a[8] if len(a) > 8 else k.get("qr", 0))
            try:
                return real(*a, **k)
            finally:
                spy.in_verify = False
        e.runner._run = _run


@pytest.mark.parametrize("name,kw,bound", [("tiny-llama", {}, BOUND), (G8, {}, BOUND),
                                           ("tiny-qwen3", {}, BOUND), ("tiny-qwen3", dict(weight_dtype="fp8"), BOUND_FP8)])
def test_verify_steps_match_the_cpu_engine(name, kw, bound, cpu_side, monkeypatch):
    rec, (cpu_toks, cpu_rows, cpu_steps) = cpu_side(name, **kw)
    _, gpu = models(name)
    e = engine(name, gpu, **kw)
    assert sorted(e.runner.verify_graphs) == [1, 2, 4, 8]
    e.proposer = Script(PROMPTS, rec, e.mcfg.vocab_size)
    toks, rows, steps = run(e)
    assert e.runner.stats["verify_graph_steps"] == e.runner.stats["verify_steps"] > 0
    compare(rows, cpu_rows, bound, f"{name} {kw}")
    n_draft, n_acc = check_invariant(steps)
    check_invariant(cpu_steps)
    assert n_draft > 0 and 0 < n_acc < n_draft, (n_draft, n_acc)
    # every draft count 0..k occurred, sequences without a draft inside verify steps among them
    assert {len(d) for d, _, _ in cpu_steps} >= set(range(K_OF[name] + 1))
    assert {len(d) for d, _, _ in steps} >= {0, K_OF[name]}
    assert e.spec_draft_tokens == n_draft and e.spec_accepted_tokens == n_acc
    assert all(len(t) == MAX_TOKENS for t in toks)
    # eager verify steps run the same launches at the same partition plan: bit-identical tokens
    spy = Spy(monkeypatch)
    e2 = engine(name, gpu, graphs=False, **kw)
    spy.watch(e2)
    e2.proposer = Script(PROMPTS, rec, e2.mcfg.vocab_size)
    toks2, _, steps2 = run(e2)
    assert toks2 == toks and e2.runner.stats["verify_steps"] == e.runner.stats["verify_steps"]
    assert [s[:2] for s in steps2] == [s[:2] for s in steps]
    n = spy.n
    assert n["verify"] > 0 and n["fused_v"] == 0 and n["decode_qkv_v"] == 0, n
    if e2.model.layers[0].attn.qkv_pf is not None:   # the folded chain: the slab writer feeds the verify attention
        assert n["slab_v"] == n["verify"] and n["rope_v"] == 0, n
    else:
        assert n["slab_v"] + n["rope_v"] == n["verify"], n


def test_a_proposer_with_nothing_to_say_leaves_todays_steps(monkeypatch):
    name = "tiny-qwen3"
    _, gpu = models(name)
    spy = Spy(monkeypatch)
    counts = []
    for speculative in (None, "ngram"):
        e = engine(name, gpu, speculative=speculative)
        if speculative:
            e.proposer = Nothing()
        before = dict(spy.n)
        toks, rows, _ = run(e)
        counts.append((toks, e.runner.stats["graph_steps"], e.runner.stats["short_graph_steps"], e.step_count,
                       {k: spy.n[k] - before[k] for k in spy.n}))
        assert not rows and e.runner.stats.get("verify_steps", 0) == 0
    assert counts[0] == counts[1], counts
    assert counts[0][1] > 0


def test_mutant_every_row_taken_as_real_misses(cpu_side):
    """verify_rows forced to QR: a sequence with fewer drafts attends as if it had k, every real row
    loses its newest keys -- the logits leave the bound.  (The greedy invariant is decided from the
    step's own logits and cannot see this; the comparison with the CPU engine does.)"""
    name = "tiny-llama"
    rec, (_, cpu_rows, _) = cpu_side(name)
    _, gpu = models(name)
    e = engine(name, gpu)
    e.proposer = Script(PROMPTS, rec, e.mcfg.vocab_size)
    real = e.runner._pack_verify

    def pack(batch):
        out = real(batch)
        e.runner.h["verify_rows"][:len(batch.decodes)] = e.runner.spec_qr
        return out
    e.runner._pack_verify = pack
    toks, rows, steps = run(e)
    assert any(len(d) < K_OF[name] for d, _, _ in steps)
    common = sorted(set(rows) & set(cpu_rows))
    worst = max(dist(rows[k], cpu_rows[k]) for k in common)
    print(f"\nmutant: worst d = {worst:.3f} over {len(common)} rows")
    assert worst > BOUND
