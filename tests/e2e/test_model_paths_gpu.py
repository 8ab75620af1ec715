"""Every serving path of the model forward on the GPU against the float64 model of
tests/model_cases.py, with norm weights that are not ones.

``models/llama.py`` routes one norm weight through many forms: folded into ``qkv_pf`` / ``gate_up_pf``
with the row scale from the parts, applied by ``norm_apply`` with ``ln2`` before the unfolded
``gate_up``, applied with unit weights before the folded packed weight, applied by the add + norm
kernels, and again in the LoRA, quantised and verify variants.  Each test below drives the engine
down one of these, asserts with a spy or the runner's counters that the path was really taken, and
holds every sampled row to

    ||gpu logits - ref64||_2 / ||ref64||_2  <=  T

where ref64 is teacher-forced with the GPU's own tokens (no row is lost to a flipped greedy token)
and T = ``model_cases.threshold(model)`` is set on the CPU alone (tests/unit/test_model_cases.py): at
least twice the CPU engine's worst row, at most half of the best-hidden norm-wiring mutant's.  The
GPU paths round where the CPU path rounds, plus one rounding of W diag(ln) in the folded weights and
another summation order.  The last test wires a GPU model wrongly and must miss T on every row.
"""
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine
from polykey_service_amd.models import build_model, get_config, llama
from polykey_service_amd.models.llama import LlamaForCausalLM
from polykey_service_amd.models.lora import LoraAdapter
from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm, gemm_prefill
from polykey_service_amd.parallel.state import ParallelState
from tests import model_cases as mc

pytestmark = pytest.mark.gpu
LLAMA, QWEN = "tiny-llama-gqa4", "tiny-qwen3"


@pytest.fixture(autouse=True)
def graph_logits(monkeypatch):
    """Graph-replayed steps keep their logits too (a copy captured into each graph, model_runner.py)."""
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")


_CPU = {}


def models(name):
    """-> (float64 weights of the CPU model, a fresh GPU copy of it), norm weights redrawn."""
    if name not in _CPU:
        cpu = build_model(get_config(name), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(mc.MODEL_SEED)
        mc.randomize_norms(cpu)
        _CPU[name] = (cpu, mc.weights64(cpu))
    cpu, sd = _CPU[name]
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return sd, gpu


def engine(name, model, graphs=False, **kw):
    base = dict(max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512)
    base.update(kw)
    return LLMEngine(EngineConfig(model=name, hip_graphs=graphs, device="cuda", **base),
                     ParallelState(device=torch.device("cuda")), model=model)


class Trace:
    """Which forward served each step, and the launches that tell the forms of a path apart."""

    def __init__(self, monkeypatch):
        self.steps = []   # (T, decode rows, prefill sequences, verify rows per sequence) of every forward
        self.chain, self.chain_lora, self.general_lora = [], [], []   # row counts
        self.n = dict(fused=0, decode_qkv=0, slab=0, slab_norm=0, rope=0, rope_norm=0, verify=0, wide_silu=0,
                      wide_head=0, norm_ln2=0, norm_ones=0, gate_up_rowscale=0)
        t = self
        real = dict(forward=LlamaForCausalLM.forward, chain=LlamaForCausalLM._forward_rowscale,
                    chain_lora=LlamaForCausalLM._forward_rowscale_lora, lora=LlamaForCausalLM._forward_lora,
                    fused=gemm.qkv_attn_fused, decode_qkv=A.paged_decode_from_qkv, slab=gemm.qkv_reduce_rope_cache,
                    rope=A.rope_and_cache, verify=A.paged_verify, wide=gemm_prefill.linear, norm_apply=gemm.norm_apply,
                    linear_silu=gemm.linear_silu)

        def forward(self, ids, pos, md, kv):
            t.steps.append((ids.shape[0], md.num_decode, md.num_prefill, md.verify_qr))
            return real["forward"](self, ids, pos, md, kv)

        def rows(into, fn):
            def f(self, x, *a, **k):
                into.append(x.shape[0])
                return fn(self, x, *a, **k)
            return f

        def lora(self, ids, pos, md, kv):
            before = len(t.chain_lora)
            out = real["lora"](self, ids, pos, md, kv)
            if len(t.chain_lora) == before:
                t.general_lora.append(ids.shape[0])
            return out

        def count(key, fn):
            def f(*a, **k):
                t.n[key] += 1
                return fn(*a, **k)
            return f

        def normed(key, fn):
            def f(*a, **k):
                t.n[key + ("_norm" if k.get("q_norm") is not None else "")] += 1
                return fn(*a, **k)
            return f

        def wide(x, w, *a, **k):
            t.n["wide_silu" if k.get("silu") else "wide_head"] += 1
            return real["wide"](x, w, *a, **k)

        def norm_apply(residual, parts, weight, eps):
            if any(weight is layer.ln2 for layer in t.model.layers):
                t.n["norm_ln2"] += 1
            elif weight is getattr(t.model, "_ones_h", None):
                t.n["norm_ones"] += 1
            return real["norm_apply"](residual, parts, weight, eps)

        def linear_silu(*a, **k):
            t.n["gate_up_rowscale"] += int(k.get("rowscale") is not None)
            return real["linear_silu"](*a, **k)
        self.model = None
        monkeypatch.setattr(LlamaForCausalLM, "forward", forward)
        monkeypatch.setattr(LlamaForCausalLM, "_forward_rowscale", rows(self.chain, real["chain"]))
        monkeypatch.setattr(LlamaForCausalLM, "_forward_rowscale_lora", rows(self.chain_lora, real["chain_lora"]))
        monkeypatch.setattr(LlamaForCausalLM, "_forward_lora", lora)
        monkeypatch.setattr(gemm, "qkv_attn_fused", count("fused", real["fused"]))
        monkeypatch.setattr(A, "paged_decode_from_qkv", count("decode_qkv", real["decode_qkv"]))
        monkeypatch.setattr(gemm, "qkv_reduce_rope_cache", normed("slab", real["slab"]))
        monkeypatch.setattr(A, "rope_and_cache", normed("rope", real["rope"]))
        monkeypatch.setattr(A, "paged_verify", count("verify", real["verify"]))
        monkeypatch.setattr(gemm_prefill, "linear", wide)
        monkeypatch.setattr(gemm, "norm_apply", norm_apply)
        monkeypatch.setattr(gemm, "linear_silu", linear_silu)

    def reset(self, model):
        """Forget what set-up (graph capture, warm-up) launched; watch ``model`` from here."""
        self.model = model
        del self.steps[:], self.chain[:], self.chain_lora[:], self.general_lora[:]
        for k in self.n:
            self.n[k] = 0


def check(what, name, sd, prompts, tokens, logits, loras=None):
    """Every row within T of the float64 model; prints and returns the worst error / T."""
    T = mc.threshold(name)
    errs = mc.row_errors(sd, get_config(name), prompts, tokens, logits, loras=loras)
    worst = max(max(e) for e in errs)
    print(f"\n[model paths] {what}: {sum(len(e) for e in errs)} rows, worst error / T = {worst / T:.3f}")
    assert worst <= T, (what, worst, T, errs)
    return worst / T


# ----------------------------------------------------------------------------- prefill
def test_prefill_general_path(monkeypatch):
    """One step of 4 + 32 + 34 + 78 rows: above 64, so the library GEMMs, ``rope_and_cache`` and the
    add + norm kernels with ``ln1`` / ``ln2`` / ``norm``; never the folded chain."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    e = engine(LLAMA, gpu)
    tr.reset(e.model)
    toks, lg = mc.collect(e, mc.PROMPTS, max_tokens=1)
    check("prefill, general path", LLAMA, sd, mc.PROMPTS, toks, lg)
    assert tr.steps == [(sum(mc.PROMPT_LENS), 0, 4, 0)] and not tr.chain and tr.n["rope"] > 0, (tr.steps, tr.n)


def test_prefill_in_chunks_and_mixed_steps(monkeypatch):
    """A 64-token budget: the 78-token prompt is prefilled in chunks, chunks of at most 64 rows run
    inside the folded chain through the slab writer, and some steps carry decode rows next to
    prefill rows."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    e = engine(LLAMA, gpu, max_num_batched_tokens=64)
    tr.reset(e.model)
    toks, lg = mc.collect(e, mc.PROMPTS, max_tokens=4)
    check("prefill in chunks, mixed steps", LLAMA, sd, mc.PROMPTS, toks, lg)
    with_prefill = [s for s in tr.steps if s[2] > 0]
    assert len(with_prefill) >= 3 and all(s[0] <= 64 for s in tr.steps), tr.steps
    assert any(nd > 0 and npf > 0 for _, nd, npf, _ in tr.steps), tr.steps
    assert tr.chain == [s[0] for s in tr.steps] and tr.n["slab"] > 0 and tr.n["rope"] == 0, (tr.steps, tr.chain, tr.n)


def test_prefix_cache_hit(monkeypatch):
    """The second request shares 64 tokens (two blocks) with a finished one: it prefills only its
    tail, attending over cached keys another request wrote."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    e = engine(LLAMA, gpu)
    first = mc.prompt(70, 5)
    second = first[:64] + mc.prompt(11, 6)[1:]
    t1, l1 = mc.collect(e, [first])
    tr.reset(e.model)
    cached = e.scheduler.num_cached_tokens
    t2, l2 = mc.collect(e, [second])
    check("prefix-cache hit", LLAMA, sd, [first, second], t1 + t2, l1 + l2)
    assert e.scheduler.num_cached_tokens - cached == 64
    assert tr.steps[0] == (len(second) - 64, 0, 1, 0), tr.steps


def test_prefill_on_packed_only_weights(monkeypatch):
    """Only the block-packed copies: prefill above 64 rows reads the folded ``qkv_pf`` / ``gate_up_pf``
    through the MFMA prefill GEMM after a norm with unit weights (``ln1`` / ``ln2`` become ones, the
    originals live in the packed weights)."""
    monkeypatch.setenv("POLYKEY_PACKED_WEIGHTS", "packed")
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    e = engine(LLAMA, gpu)
    m = e.model
    assert m.packed_only and m.layers[0].attn.qkv.is_meta and m.layers[0].mlp.gate_up.is_meta
    assert float(m.layers[1].ln1.min()) == float(m.layers[1].ln2.max()) == 1.0
    tr.reset(m)
    prompts = [mc.prompt(70, 1), mc.prompt(130, 2)]
    toks, lg = mc.collect(e, prompts)
    check("prefill + decode on packed-only weights", LLAMA, sd, prompts, toks, lg)
    assert tr.steps[0] == (200, 0, 2, 0) and 200 not in tr.chain, (tr.steps, tr.chain)
    assert tr.n["wide_silu"] > 0 and tr.n["wide_head"] > 0 and tr.n["rope"] > 0, tr.n


# ----------------------------------------------------------------------------- decode, up to 64 rows
def _small_decode(tr, sd, gpu, what):
    e = engine(LLAMA, gpu)
    tr.reset(e.model)
    toks, lg = mc.collect(e, mc.PROMPTS, max_tokens=4)
    check(what, LLAMA, sd, mc.PROMPTS, toks, lg)
    assert tr.steps[1:] == [(4, 4, 0, 0)] * 3, tr.steps


def test_decode_folded_chain_fused_launch(monkeypatch):
    """QKV slabs handed in-launch to the decode attention (enabled for this model's 2 kv heads)."""
    monkeypatch.setattr(gemm, "QKV_ATTN_MIN_KV", 1)
    assert gemm.QKV_ATTN_FUSED
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    _small_decode(tr, sd, gpu, "decode <= 64 rows, folded chain, fused launch")
    assert tr.chain == [4] * 3 and tr.n["fused"] > 0 and tr.n["decode_qkv"] == 0, (tr.chain, tr.n)


def test_decode_folded_chain_two_launch_forms(monkeypatch):
    saved = (gemm.MLP_FUSED, gemm.QKV_ATTN_FUSED)
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    try:
        gemm.disable_fused()
        _small_decode(tr, sd, gpu, "decode <= 64 rows, folded chain, two-launch forms")
    finally:
        gemm.MLP_FUSED, gemm.QKV_ATTN_FUSED = saved
    assert tr.chain == [4] * 3 and tr.n["fused"] == 0 and tr.n["decode_qkv"] > 0, (tr.chain, tr.n)
    assert tr.n["gate_up_rowscale"] > 0, tr.n


def test_decode_unfolded_chain(monkeypatch):
    """The normalised chain: add + norm kernels with ``ln1`` / ``ln2`` on the split-K slabs."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    monkeypatch.setattr(LlamaForCausalLM, "_rowscale_ok", lambda self, x: False)
    _small_decode(tr, sd, gpu, "decode <= 64 rows, unfolded chain")
    assert not tr.chain and tr.n["decode_qkv"] > 0 and tr.n["gate_up_rowscale"] == 0, (tr.chain, tr.n)


# ----------------------------------------------------------------------------- decode, wide batches
def _wide_decode(tr, sd, gpu, batch, what):
    """``batch`` six-token prompts: one prefill step, one decode step of ``batch`` rows."""
    e = engine(LLAMA, gpu, max_num_seqs=512, max_num_batched_tokens=4096, max_model_len=256, num_kv_blocks=1024,
               prefix_caching=False)
    tr.reset(e.model)
    prompts = [[1] + [(7 * i + 3 * j) % 1000 + 3 for j in range(5)] for i in range(batch)]
    toks, lg = mc.collect(e, prompts, max_tokens=2)
    check(what, LLAMA, sd, prompts, toks, lg)
    assert tr.steps == [(6 * batch, 0, batch, 0), (batch, batch, 0, 0)] and tr.chain == [batch], (tr.steps, tr.chain)


@pytest.mark.parametrize("batch", [100, 150, 200, 450])
def test_decode_wide_batches(batch, monkeypatch):
    """Above 64 rows the folded chain on 128-row tiles (row-tiled above 128); above 192 rows gate_up
    leaves the folded weight: ``norm_apply`` with ``ln2``, then the library GEMM on the plain one."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    _wide_decode(tr, sd, gpu, batch, f"decode at {batch} rows")
    if batch > llama.GATE_UP_SKINNY_MAX_M:
        assert tr.n["norm_ln2"] > 0 and tr.n["gate_up_rowscale"] == 0 and tr.n["wide_silu"] == 0, tr.n
    else:
        assert tr.n["norm_ln2"] == 0 and tr.n["gate_up_rowscale"] > 0, tr.n


def test_decode_wide_batch_on_the_mfma_gemm(monkeypatch):
    """200 rows with the tile threshold lowered: ``norm_apply`` with unit weights, then the folded
    packed gate_up (``ln2`` inside the weight) and the packed LM head on the prefill MFMA GEMM."""
    monkeypatch.setattr(llama, "WIDE_MFMA_MIN_TILES", 1)
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    _wide_decode(tr, sd, gpu, 200, "decode at 200 rows, wide MFMA gate_up + LM head")
    assert tr.n["norm_ones"] > 0 and tr.n["norm_ln2"] == 0 and tr.n["wide_silu"] > 0 and tr.n["wide_head"] > 0, tr.n


# ----------------------------------------------------------------------------- graphs
def test_decode_graph_replay_short_and_long_context():
    """Decode steps replayed from the short-context graph, then, once a context passes the 512-token
    partition, from the long-context one."""
    sd, gpu = models(LLAMA)
    e = engine(LLAMA, gpu, graphs=True, max_num_batched_tokens=1024, max_model_len=1024)
    prompts = [mc.prompt(500, 3), mc.prompt(60, 4)]
    toks, lg = mc.collect(e, prompts, max_tokens=24)
    check("decode graph replay, contexts crossing 512", LLAMA, sd, prompts, toks, lg)
    st = e.runner.stats
    assert st["graph_steps"] == 23 and 0 < st["short_graph_steps"] < st["graph_steps"], st


# ----------------------------------------------------------------------------- QK-norm
def test_qwen3_prefill_and_folded_chain(monkeypatch):
    """``tiny-qwen3``: prefill on the general path (``rope_and_cache`` with the QK-norm), decode in
    the folded chain through the slab writer with the QK-norm."""
    tr = Trace(monkeypatch)
    sd, gpu = models(QWEN)
    e = engine(QWEN, gpu)
    tr.reset(e.model)
    toks, lg = mc.collect(e, mc.PROMPTS)
    check("tiny-qwen3 prefill + folded chain", QWEN, sd, mc.PROMPTS, toks, lg)
    assert tr.steps == [(sum(mc.PROMPT_LENS), 0, 4, 0)] + [(4, 4, 0, 0)] * 2 and tr.chain == [4, 4], (tr.steps, tr.chain)
    n = tr.n
    assert n["rope_norm"] > 0 and n["slab_norm"] > 0 and n["rope"] == n["slab"] == n["fused"] == n["decode_qkv"] == 0, n


def test_qwen3_chunked_mixed_steps(monkeypatch):
    tr = Trace(monkeypatch)
    sd, gpu = models(QWEN)
    e = engine(QWEN, gpu, max_num_batched_tokens=64)
    tr.reset(e.model)
    toks, lg = mc.collect(e, mc.PROMPTS, max_tokens=4)
    check("tiny-qwen3 chunked prefill, mixed steps", QWEN, sd, mc.PROMPTS, toks, lg)
    assert any(nd > 0 and npf > 0 for _, nd, npf, _ in tr.steps), tr.steps
    n = tr.n
    assert tr.chain == [s[0] for s in tr.steps] and n["slab_norm"] > 0, (tr.steps, tr.chain, n)
    assert n["rope"] == n["rope_norm"] == n["slab"] == n["fused"] == n["decode_qkv"] == 0, n


# ----------------------------------------------------------------------------- speculative decoding
class Script:
    """Drafts from a recorded continuation: with m = prompt + output length, ``m % (k + 1)`` drafts of
    which the first ``m % 3`` are the recording's and the rest are wrong."""

    def __init__(self, prompts, recorded, vocab):
        self.rec = {tuple(p): r for p, r in zip(prompts, recorded)}
        self.vocab = vocab

    def propose(self, seq, k):
        n = len(seq.output_ids)
        m = n + len(seq.prompt_ids)
        d = self.rec[tuple(seq.prompt_ids)][n:n + min(k, m % (k + 1))]
        return [t if j < m % 3 else (t + 1) % self.vocab for j, t in enumerate(d)]


def test_verify_steps_of_speculative_decoding(monkeypatch):
    """Verify steps (k + 1 rows per sequence, the slab writer, the verify attention): real row j of
    a sequence is the float64 model's row after prompt + outputs + the first j drafts, accepted or
    not; padding rows are not looked at."""
    from polykey_service_amd.engine import SamplingParams
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    cfg = get_config(LLAMA)
    prompts = mc.PROMPTS[:3]
    rec = engine(LLAMA, gpu).generate(prompts, SamplingParams(max_tokens=12, ignore_eos=True))
    e = engine(LLAMA, gpu, speculative="ngram", num_speculative_tokens=3)
    e.proposer = Script(prompts, rec, cfg.vocab_size)
    tr.reset(e.model)
    e.runner.keep_logits = True
    real, last = e.runner.launch, {}

    def launch(batch):
        last["batch"] = batch
        return real(batch)
    e.runner.launch = launch
    rows = []   # (full token sequence, index of the row's position in it, logits row)
    try:
        seqs = [e.add_request(p, SamplingParams(max_tokens=12, ignore_eos=True)) for p in prompts]
        qr = e.spec_k + 1
        while e.has_unfinished():
            last.clear()
            before = {s.seq_id: list(s.output_ids) for s in seqs}
            e.step()
            b = last.get("batch")
            if b is None or b.drafts is None:
                continue
            lg = e.runner.last_logits.float().cpu()
            for i, (s, d) in enumerate(zip(b.decodes, b.drafts)):
                ids = list(s.prompt_ids) + before[s.seq_id] + list(d)
                for j in range(1 + len(d)):
                    rows.append((ids, len(ids) - len(d) - 1 + j, lg[i * qr + j].clone()))
    finally:
        del e.runner.launch
    T = mc.threshold(LLAMA)
    refs = {}
    worst = 0.0
    for ids, at, row in rows:
        if tuple(ids) not in refs:
            refs[tuple(ids)] = mc.ref64(sd, cfg, ids)
        worst = max(worst, mc.row_error(row, refs[tuple(ids)][at]))
    print(f"\n[model paths] verify steps: {len(rows)} rows, worst error / T = {worst / T:.3f}")
    assert len(rows) > 3 * len(prompts) and worst <= T, (len(rows), worst, T)
    assert e.runner.stats["verify_steps"] > 0 and tr.n["verify"] == 2 * e.runner.stats["verify_steps"], tr.n
    assert tr.n["slab"] >= tr.n["verify"] and tr.n["fused"] == 0, tr.n
    assert any(v == qr for _, _, _, v in tr.steps), tr.steps
    assert e.spec_draft_tokens > e.spec_accepted_tokens > 0   # accepted and rejected drafts both occurred


# ----------------------------------------------------------------------------- LoRA
def test_lora_general_path_and_folded_chain(monkeypatch):
    """One rank-16 adapter on q / k / v / o / gate / up / down, adapter rows next to base rows: the
    148-row prefill step on the general path (bf16 add form), the decode steps in
    ``_forward_rowscale_lora`` (slab add form; the shrink reads ``norm_apply`` of ``ln1`` / ``ln2``)."""
    tr = Trace(monkeypatch)
    sd, gpu = models(LLAMA)
    ad = LoraAdapter.random(get_config(LLAMA), rank=16, alpha=16, seed=1, b_std=0.08)
    e = engine(LLAMA, gpu, lora_modules=(("X", ad),))
    tr.reset(e.model)
    loras = ["X", None, "X", None]
    toks, lg = mc.collect(e, mc.PROMPTS, loras=loras)
    check("LoRA, general path + folded chain", LLAMA, sd, mc.PROMPTS, toks, lg,
          loras=[mc.lora_of(ad) if l else None for l in loras])
    assert tr.general_lora == [sum(mc.PROMPT_LENS)] and tr.chain_lora == [4, 4] and not tr.chain, \
        (tr.general_lora, tr.chain_lora, tr.chain)
    assert e.runner.stats["lora_steps"] == 3


# ----------------------------------------------------------------------------- the check bites
def test_mutant_ln1_and_ln2_of_layer_1_exchanged_misses_on_every_row():
    sd, gpu = models(LLAMA)
    layer = gpu.layers[1]
    layer.ln1, layer.ln2 = layer.ln2, layer.ln1   # before the engine packs (and folds) the weights
    e = engine(LLAMA, gpu)
    toks, lg = mc.collect(e, mc.PROMPTS)
    T = mc.threshold(LLAMA)
    errs = [x for r in mc.row_errors(sd, get_config(LLAMA), mc.PROMPTS, toks, lg) for x in r]
    print(f"\n[model paths] GPU mutant: smallest error / T = {min(errs) / T:.2f} over {len(errs)} rows")
    assert len(errs) == 12 and min(errs) > T, errs
