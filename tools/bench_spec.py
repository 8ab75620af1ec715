"""Speculative decoding, whole steps and end to end, on one GPU (Llama-3-8B, random init by default).

Three measurements per batch size, written as JSON lines:

* ``step``: device time of the graph-replayed decode step and of the graph-replayed verify step
  (QR = k + 1 rows per sequence) on the inputs of a real step of that batch -- the graph the engine
  just replayed, replayed again back to back between device events.  ``break_even`` is
  ``t_verify / t_decode - 1``: the accepted drafts per verify step above which speculation wins on
  device time.
* ``e2e``: output tokens per second of whole generations with a *replay proposer*: it drafts a
  recorded continuation and corrupts a chosen fraction of the draft positions, so the acceptance
  rate is scripted (the achieved one is reported from the engine's counters).  The recording is the
  output of the acceptance-0 run (every draft wrong, every step a verify step): a random-init 8B
  model has near-ties at almost every token, so the continuation of the run *without* speculation,
  whose decode steps round differently, is left after a token or two -- while a verify row's result
  does not depend on what the other rows hold, so the verify path reproduces its own recording
  whatever is accepted (``reproduced`` counts the requests that did).  Random-weight models do not
  copy their prompts: no natural-text acceptance rate can be measured this way, only the cost and
  gain at a given rate.
* ``idle``: speculation configured with a proposer that never drafts (every step is today's decode
  step, but no continuation launches) against the same build with speculation off; and the host
  time of the n-gram proposer per call on the sequences of the run.

    python tools/bench_spec.py [--model llama3-8b] [--weight-dtype bf16] [--seqs 1,8,64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams  # noqa: E402
from polykey_service_amd.engine import spec  # noqa: E402
from polykey_service_amd.parallel.state import ParallelState  # noqa: E402


class Replay:
    """Drafts the recorded continuation; draft position p of a prompt is corrupted when a hash of
    (prompt, p) falls below ``wrong`` (a fraction in [0, 1])."""

    def __init__(self, prompts, recorded, wrong: float, vocab: int):
        self.rec = {tuple(p): r for p, r in zip(prompts, recorded)}
        self.key = {tuple(p): zlib.crc32(repr(p).encode()) for p in prompts}
        self.wrong, self.vocab = wrong, vocab

    def propose(self, seq, k):
        p = tuple(seq.prompt_ids)
        n = len(seq.output_ids)
        out = []
        for j, t in enumerate(self.rec[p][n:n + k]):
            h = zlib.crc32(f"{self.key[p]}:{n + j}".encode()) / 2 ** 32
            out.append((t + 1) % self.vocab if h < self.wrong else t)
        return out


class Nothing:
    def propose(self, seq, k):
        return []


class Junk:
    """k drafts that are wrong (the last token + 1, + 2, ..: not what a model samples next)."""

    def __init__(self, vocab: int):
        self.vocab = vocab

    def propose(self, seq, k):
        last = seq.output_ids[-1] if seq.output_ids else seq.prompt_ids[-1]
        return [(last + 1 + j) % self.vocab for j in range(k)]


def prompts_for(n: int, length: int, vocab: int):
    g = torch.Generator().manual_seed(1234)
    return [[1] + torch.randint(3, vocab, (length - 1,), generator=g).tolist() for _ in range(n)]


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def generate(e, prompts, max_tokens):
    """-> (tokens per request, wall seconds, engine steps)."""
    seqs = [e.add_request(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True)) for p in prompts]
    sync()
    s0, t0 = e.step_count, time.perf_counter()
    while e.any_unfinished():
        e.step()
    sync()
    return [list(s.output_ids) for s in seqs], time.perf_counter() - t0, e.step_count - s0


def replay_last_step_us(e, replays=40):
    """Device time of the graph the engine's last step replayed, on that step's inputs."""
    r = e.runner
    mode, T, n, nd, ns, max_q, g, short, cont, lora, qr = (int(v) for v in r.h["header"][:11])
    if not g:
        return None, qr
    graph = r.verify_graphs[g] if qr else (r.short_graphs[g] if short else r.graphs[g])
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / replays * 1000
        best = us if best is None else min(best, us)
    return best, qr


def step_times(e, prompts, vocab):
    """Decode and verify step device times on the inputs of real steps of this batch."""
    out = {}
    for what, proposer in (("decode", Nothing()), ("verify", Replay(prompts, [[5] * 64 for _ in prompts], 1.0, vocab))):
        e.proposer = proposer
        seqs = [e.add_request(p, SamplingParams(max_tokens=24, ignore_eos=True)) for p in prompts]
        for _ in range(8):   # prefill, then a few steps of the kind
            e.step()
        sync()
        us, qr = replay_last_step_us(e)
        assert (qr > 0) == (what == "verify"), (what, qr)
        out[what + "_us"] = us
        for s in seqs:
            e.abort(s.request_id)
        while e.any_unfinished():
            e.step()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--weight-dtype", default="bf16")
    ap.add_argument("--seqs", default="1,8,64")
    ap.add_argument("--prompt-len", type=int, default=384)
    ap.add_argument("--max-tokens", type=int, default=96)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--num-layers", type=int, default=0)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--device", default="cuda", help="cpu: a rehearsal of the host logic (no times are meaningful)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.device != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_spec needs the GPU")
    sizes = [int(x) for x in a.seqs.split(",")]
    st = ParallelState(device=torch.device(a.device))
    blocks = max(sizes) * ((a.prompt_len + a.max_tokens + 64) // 32 + 1) + 64

    def engine(speculative, model=None):
        cfg = EngineConfig(model=a.model, weight_dtype=a.weight_dtype, max_num_seqs=max(sizes),
                           max_num_batched_tokens=8192, max_model_len=2048, num_kv_blocks=blocks,
                           graph_batch_sizes=tuple(sizes), overlap=True, speculative=speculative,
                           num_speculative_tokens=a.k, num_layers=a.num_layers, prefix_caching=False,
                           device=a.device, hip_graphs=a.device != "cpu")
        return LLMEngine(cfg, st, model=model)

    rows = []

    def emit(**rec):
        rec = {"model": a.model, "weight_dtype": a.weight_dtype, "k": a.k, **rec}
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    off = engine(None)
    on = engine("ngram", model=off.model)
    vocab = off.mcfg.vocab_size
    for n in sizes:
        prompts = prompts_for(n, a.prompt_len, vocab)
        t = step_times(on, prompts, vocab)
        if t["decode_us"] and t["verify_us"]:   # (None: no graphs, a CPU rehearsal)
            emit(kind="step", seqs=n, qr=a.k + 1, prompt_len=a.prompt_len, decode_us=round(t["decode_us"], 1),
                 verify_us=round(t["verify_us"], 1), break_even=round(t["verify_us"] / t["decode_us"] - 1, 3))
        if a.skip_e2e:
            continue
        generate(off, prompts, 8)   # warm-up of every shape
        rec, wall, steps = generate(off, prompts, a.max_tokens)
        total = sum(len(r) for r in rec)
        base = total / wall
        emit(kind="e2e", seqs=n, mode="off", tok_s=round(base, 1), steps=steps, wall_s=round(wall, 3))
        rec_on = None
        for wrong in (1.0, 0.5, 0.25, 0.0):
            on.proposer = Junk(vocab) if rec_on is None else Replay(prompts, rec_on, wrong, vocab)
            d0, a0, v0 = on.spec_draft_tokens, on.spec_accepted_tokens, on.spec_steps
            toks, wall, steps = generate(on, prompts, a.max_tokens)
            drafted, acc, vsteps = on.spec_draft_tokens - d0, on.spec_accepted_tokens - a0, on.spec_steps - v0
            if rec_on is None:
                rec_on = toks
            emit(kind="e2e", seqs=n, mode="replay", corrupt=wrong, tok_s=round(sum(len(x) for x in toks) / wall, 1),
                 vs_off=round(sum(len(x) for x in toks) / wall / base, 3), steps=steps, wall_s=round(wall, 3),
                 accept_rate=round(acc / max(drafted, 1), 3),
                 accepted_per_seq_step=round(acc / max(vsteps * n, 1), 3),
                 reproduced=sum(x == y for x, y in zip(toks, rec_on)),
                 same_as_off=sum(x == y for x, y in zip(toks, rec)))
        on.proposer = Nothing()
        toks, wall, steps = generate(on, prompts, a.max_tokens)
        emit(kind="idle", seqs=n, tok_s=round(sum(len(x) for x in toks) / wall, 1),
             vs_off=round(sum(len(x) for x in toks) / wall / base, 3), steps=steps,
             continuation_steps_off=off.continuation_steps, continuation_steps_on=on.continuation_steps)
        # host time of the n-gram proposer: one call per sequence and step, as the engine makes them
        ng = spec.NgramProposer()
        from polykey_service_amd.engine.sequence import Sequence
        seqs = [Sequence(str(i), p, SamplingParams()) for i, p in enumerate(prompts)]
        t0 = time.perf_counter()
        for s in seqs:
            ng.propose(s, a.k)   # first call: indexes the prompt
        first = (time.perf_counter() - t0) / n
        calls, t0 = 0, time.perf_counter()
        for j in range(len(rec[0])):
            for s, r in zip(seqs, rec):
                s.output_ids.append(r[j])
                ng.propose(s, a.k)
                calls += 1
        emit(kind="proposer", seqs=n, first_call_us=round(first * 1e6, 1),
             per_call_us=round((time.perf_counter() - t0) / calls * 1e6, 2),
             per_step_us=round((time.perf_counter() - t0) / len(rec[0]) * 1e6, 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
