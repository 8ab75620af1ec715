"""The whole model forward against a float64 model (library of tests/unit/test_model_cases.py, which
derives the thresholds on the CPU, and tests/e2e/test_model_paths_gpu.py, which holds every serving
path of the GPU engine to them).

``init_random`` draws ``norm``, ``ln1`` and ``ln2`` as ones, and a model whose norm weights are ones
cannot tell a norm weight that is ignored, applied twice, swapped or taken from another layer from
one applied correctly.  :func:`randomize_norms` redraws them; :func:`ref64` is a plain dense causal
transformer in float64 written from the model definition, on the weights ``hf_state_dict`` exports
(unfused q / k / v, de-interleaved gate / up): it knows nothing of the packed, folded or interleaved
layouts, of paging or of any kernel.  The measure is the per-row relative L2 error of the logits,
:func:`row_error`.

The threshold of a model, :func:`threshold`, is the geometric mean of the largest row error of the
CPU engine (the project's bf16-rounding reference path) and the smallest row error of any mutant of
:data:`MUTANTS` on the fixed case below; tests/unit/test_model_cases.py recomputes both and asserts
2 cpu_max <= T <= mut_min / 2.  No GPU run enters it.
"""
import math

import torch

NORM_SEED = 11
NORM_RANGE = (0.5, 2.0)
MUTANTS = ("swap_ln", "ln2_twice", "ln1_ones_layer1", "final_ones", "ln_from_next_layer")

# the fixed case of the thresholds: init_random(MODEL_SEED), randomize_norms(NORM_SEED), these
# prompts (lengths on both sides of 32 and of 64), the prefill step and two decode steps
MODEL_SEED = 3
PROMPT_LENS = (4, 32, 34, 78)
STEPS = 3


def prompt(n, salt=0):
    """``n`` tokens: BOS, then ids that differ between positions and between salts."""
    return [1] + [(7 * i + 13 * salt) % 1000 + 3 for i in range(n - 1)]


PROMPTS = [prompt(n, j) for j, n in enumerate(PROMPT_LENS)]

# sqrt(cpu_max * mut_min) of the fixed case, per model (tests/unit/test_model_cases.py prints both)
_THRESHOLDS = {
    "tiny-llama-gqa4": 0.0755,
    "tiny-qwen3": 0.0429,
}


def threshold(name):
    return _THRESHOLDS[name]


def randomize_norms(model, seed=NORM_SEED, lo=NORM_RANGE[0], hi=NORM_RANGE[1]):
    """Overwrite ``model.norm`` and every layer's ``ln1`` / ``ln2`` with distinct log-uniform draws in
    [lo, hi], rounded to the model dtype.  Before the GPU copy and before ``pack_decode_weights``
    folds them into the projections."""
    g = torch.Generator().manual_seed(1 << 20 | seed)

    def draw(w):
        u = torch.rand(w.shape, generator=g, dtype=torch.float64)
        v = torch.exp(math.log(lo) + u * (math.log(hi) - math.log(lo)))
        with torch.no_grad():
            w.copy_(v.to(device=w.device, dtype=w.dtype))
    draw(model.norm)
    for layer in model.layers:
        draw(layer.ln1)
        draw(layer.ln2)
    return model


def weights64(model):
    """``model.hf_state_dict()`` in float64 (a model whose norm weights and row-major projections
    are intact: the CPU model, not one packed on the GPU)."""
    return {k: v.double() for k, v in model.hf_state_dict().items()}


def lora_of(adapter):
    """{(layer, projection): (A, B, scale)} of a ``LoraAdapter``, for :func:`ref64`."""
    return {key: (a, b, adapter.scale) for key, (a, b) in adapter.tensors.items()}


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _rope(x, pos, theta):
    """Neox (rotate-half) rotation of heads x [T, heads, D] at positions pos [T]."""
    D = x.shape[-1]
    inv = theta ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    f = pos.double()[:, None, None] * inv
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    return torch.cat([x1 * f.cos() - x2 * f.sin(), x2 * f.cos() + x1 * f.sin()], dim=-1)


def ref64(model, cfg, ids, mutant=None, lora=None):
    """Logits [T, vocab] in float64 of the token sequence ``ids`` (one sequence, positions 0 .. T-1,
    causal attention over the whole of it).  ``model``: the model, or its :func:`weights64`.
    ``lora``: {(layer, projection): (A [r, K], B [N, r], scale)}, added to that projection's weight
    as scale * B A.  ``mutant``: one of :data:`MUTANTS`, a model that wires a norm weight wrongly."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert not cfg.rope_scaling, "ref64 has no scaled RoPE"
    sd = model if isinstance(model, dict) else weights64(model)
    L, hd, nq, nkv, eps = cfg.num_layers, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.rms_eps
    ids = torch.as_tensor(ids, dtype=torch.long)
    T = ids.shape[0]
    pos = torch.arange(T)
    causal = torch.ones(T, T, dtype=torch.bool).tril()

    def w(i, name, p):
        t = sd[f"model.layers.{i}.{name}.weight"]
        if lora is not None and (i, p) in lora:
            a, b, s = lora[(i, p)]
            t = t + s * (b.double() @ a.double())
        return t

    def ln(i, which):
        if mutant == "swap_ln":
            which = {"input_layernorm": "post_attention_layernorm", "post_attention_layernorm": "input_layernorm"}[which]
        if mutant == "ln_from_next_layer":
            i = (i + 1) % L
        t = sd[f"model.layers.{i}.{which}.weight"]
        if mutant == "ln1_ones_layer1" and i == 1 and which == "input_layernorm":
            t = torch.ones_like(t)
        return t

    h = sd["model.embed_tokens.weight"][ids]
    for i in range(L):
        x = _rms(h, ln(i, "input_layernorm"), eps)
        q = (x @ w(i, "self_attn.q_proj", "q").T).view(T, nq, hd)
        k = (x @ w(i, "self_attn.k_proj", "k").T).view(T, nkv, hd)
        v = (x @ w(i, "self_attn.v_proj", "v").T).view(T, nkv, hd)
        if cfg.qk_norm:
            q = _rms(q, sd[f"model.layers.{i}.self_attn.q_norm.weight"], eps)
            k = _rms(k, sd[f"model.layers.{i}.self_attn.k_norm.weight"], eps)
        q, k = _rope(q, pos, cfg.rope_theta), _rope(k, pos, cfg.rope_theta)
        k = k.repeat_interleave(nq // nkv, dim=1)  # query head j reads kv head j // (nq / nkv)
        v = v.repeat_interleave(nq // nkv, dim=1)
        s = torch.einsum("thd,shd->hts", q, k) / math.sqrt(hd)
        p = s.masked_fill(~causal, float("-inf")).softmax(-1)
        a = torch.einsum("hts,shd->thd", p, v).reshape(T, nq * hd)
        h = h + a @ w(i, "self_attn.o_proj", "o").T
        x = _rms(h, ln(i, "post_attention_layernorm"), eps)
        if mutant == "ln2_twice":
            x = _rms(x, ln(i, "post_attention_layernorm"), eps)
        g = x @ w(i, "mlp.gate_proj", "gate").T
        u = x @ w(i, "mlp.up_proj", "up").T
        h = h + (g * torch.sigmoid(g) * u) @ w(i, "mlp.down_proj", "down").T
    fw = sd["model.norm.weight"]
    x = _rms(h, torch.ones_like(fw) if mutant == "final_ones" else fw, eps)
    head = sd["model.embed_tokens.weight"] if cfg.tie_embeddings else sd["lm_head.weight"]
    return x @ head.T


def row_error(got, want):
    """||got - ref||_2 / ||ref||_2 of one logits row."""
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / want.norm())


def collect(e, prompts, max_tokens=STEPS, loras=None):
    """Run ``prompts`` through engine ``e`` to ``max_tokens`` each -> (output ids per request,
    per request the logits row of every sampled token, in order, fp32 on the CPU).  Rows are mapped
    to requests as the step's batch orders its sampling sequences; a step whose logits the runner
    did not keep (a graph replay without POLYKEY_DEBUG_LOGITS) leaves a gap the caller sees in the
    row counts."""
    from polykey_service_amd.engine import SamplingParams
    e.runner.keep_logits = True
    real, last = e.runner.launch, {}

    def launch(batch):
        last["sampling"] = batch.sampling_seqs()
        return real(batch)
    e.runner.launch = launch
    try:
        seqs = [e.add_request(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True,
                                                **({"lora": loras[i]} if loras else {})))
                for i, p in enumerate(prompts)]
        idx = {s.seq_id: i for i, s in enumerate(seqs)}
        got = [[] for _ in seqs]
        while e.has_unfinished():
            e.runner.last_logits = None
            last.clear()
            before = {s.seq_id: len(s.output_ids) for s in seqs}
            e.step()
            if e.runner.last_logits is None or "sampling" not in last:
                continue
            lg = e.runner.last_logits.float().cpu()
            for r, s in enumerate(last["sampling"]):
                if s.seq_id in idx and len(got[idx[s.seq_id]]) == before[s.seq_id]:
                    got[idx[s.seq_id]].append(lg[r].clone())
    finally:
        del e.runner.launch
    return [list(s.output_ids) for s in seqs], got


def row_errors(model, cfg, prompts, tokens, logits, mutant=None, loras=None):
    """Row errors of :func:`collect`'s logits against :func:`ref64` teacher-forced with the tokens
    the engine produced: the row that sampled output token j of a request sits at position
    len(prompt) + j - 1 of prompt + outputs.  ``loras``: per request a :func:`lora_of` dict or None.
    -> one list of errors per request."""
    sd = model if isinstance(model, dict) else weights64(model)
    out = []
    for i, (p, toks, rows) in enumerate(zip(prompts, tokens, logits)):
        assert len(rows) == len(toks) > 0, (i, len(rows), len(toks))
        ref = ref64(sd, cfg, list(p) + list(toks[:-1]), mutant, loras[i] if loras else None)
        out.append([row_error(r, ref[len(p) - 1 + j]) for j, r in enumerate(rows)])
    return out
