"""The guided decoding kernels next to pk_penalty_apply at the 8B decode shape (B = 64 rows,
V = 128,256), and the compiler's state counts and compile times.

GPU part: device-event times per call (graph replays of 20 back-to-back calls) of pk_grammar_mask
and pk_grammar_advance with 0, 1, 8 and 64 of the 64 rows constrained by a JSON-schema grammar
(rows inside a string value, where most ids survive their walk), and pk_penalty_apply at the
same row counts as the yardstick.  The vocabulary is synthetic: 256 single-byte ids, the rest
2..12 ASCII-heavy bytes.  CPU part (``--compile``, needs no GPU): the test grammars of
tests/grammar_cases.py.  Prints markdown (profiles/grammar_kernel.md).

Usage: ``python tools/bench_grammar.py [--rows 64] [--vocab 128256] [--iters 400]`` or ``--compile``
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from polykey_service_amd.engine import grammar as G  # noqa: E402

CALLS_PER_GRAPH = 20
SCHEMA = {"type": "object", "properties": {
    "location": {"type": "object", "properties": {"city": {"type": "string"}, "country": {"type": "string", "maxLength": 32}}},
    "unit": {"enum": ["celsius", "fahrenheit"]}, "days": {"type": "integer"},
    "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 8}, "detailed": {"type": "boolean"}}}


def timed(fn, iters):
    """us per call, from device events around replays of a graph of CALLS_PER_GRAPH back-to-back calls."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS_PER_GRAPH):
            fn()
    reps = max(1, iters // CALLS_PER_GRAPH)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (reps * CALLS_PER_GRAPH)


def vocabulary(V: int):
    rng = np.random.default_rng(0)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz ETAOIN0123456789\"{}:,.-_", dtype=np.uint8)
    lens = np.concatenate([np.ones(256, dtype=np.int64), rng.integers(2, 13, size=V - 256)])
    off = np.zeros(V + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    data = letters[rng.integers(0, letters.size, size=int(off[-1]))].copy()
    data[:256] = np.arange(256, dtype=np.uint8)
    return off, data


def compile_table():
    from tests import grammar_cases as gc
    print("| grammar | states | byte classes | table words | compile ms |\n|---|---|---|---|---|")
    jobs = [("regex " + p, lambda p=p: G.compile_regex(p)) for p in gc.REGEX_PATTERNS + [gc.CHAIN, gc.WORDS]]
    jobs += [("json " + n, lambda s=s: G.compile_json(s)) for n, s in gc.JSON_SCHEMAS.items()]
    jobs += [("json tool call (this file's SCHEMA)", lambda: G.compile_json(SCHEMA))]
    G.compile_regex(r"\w")  # the Unicode class tables are built once per process: not part of a compile
    for name, job in jobs:
        t0 = time.perf_counter()
        g = job()
        ms = (time.perf_counter() - t0) * 1e3
        words = 132 + (g.n_states * g.n_classes + 1) // 2
        print(f"| `{name}` | {g.n_states} | {g.n_classes} | {words} | {ms:.1f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--compile", action="store_true", help="CPU only: state counts and compile times")
    a = ap.parse_args()
    if a.compile:
        compile_table()
        return
    assert torch.cuda.is_available(), "needs a GPU"
    from polykey_service_amd.ops import grammar as gram
    from polykey_service_amd.ops import penalties
    B, V = a.rows, a.vocab
    off, data = vocabulary(V)
    g = G.compile_json(SCHEMA)
    st = gram.GrammarState(B, off, data, "cuda")
    words = torch.from_numpy(gram.pack(g.cmap, g.trans, g.accept)).cuda()
    gram.load(st, 0, 0, words, words.numel())
    in_string = g.walk(0, b'{"location": {"city": "Os')
    start = 0
    pen = penalties.PenaltyState(B, V, "cuda")
    torch.manual_seed(0)
    x = (torch.randn(B, V, device="cuda") * 3).to(torch.bfloat16)
    full = lambda v, dt: torch.full((B,), v, dtype=dt, device="cuda")
    rep, freq, pres = full(1.0, torch.float32), full(0.0, torch.float32), full(0.0, torch.float32)
    toks = torch.randint(0, 256, (B,), dtype=torch.int32, device="cuda")
    print(f"B = {B}, V = {V}, JSON-schema grammar of {g.n_states} states x {g.n_classes} byte classes "
          f"({132 + (g.n_states * g.n_classes + 1) // 2} table words), vocabulary of {int(off[-1])} bytes, "
          f"{a.iters} calls each (graphs of {CALLS_PER_GRAPH}), device events\n")
    print("| constrained rows | state | pk_grammar_mask us | ids kept per row | pk_grammar_advance us | pk_penalty_apply us |")
    print("|---|---|---|---|---|---|")
    for n in (0, 1, 8, B):
        for label, state in (("inside a string", in_string), ("start", start)):
            if n == 0 and label == "start":
                continue
            slots = torch.full((B,), -1, dtype=torch.int32)
            slots[:n] = torch.arange(n, dtype=torch.int32)
            ent = [[s, 0, state, 1, 2] + [-1] * (gram.MAX_END - 1) for s in range(B)]
            gram.seed(st, torch.tensor(ent, dtype=torch.int32).cuda().reshape(-1), B)
            slots = slots.cuda()
            penalties.apply(pen, x, slots, rep, freq, pres)
            gram.mask(st, pen.out, slots, B, V)
            torch.cuda.synchronize()
            kept = int(torch.isfinite(pen.out[0, :V]).sum()) if n else 0
            t_mask = timed(lambda: gram.mask(st, pen.out, slots, B, V), a.iters)
            t_adv = timed(lambda: gram.advance(st, slots, toks, B, V), a.iters)
            t_pen = timed(lambda: penalties.apply(pen, x, slots, rep, freq, pres), a.iters)
            print(f"| {n} | {label if n else '-'} | {t_mask:.1f} | {kept} | {t_adv:.1f} | {t_pen:.1f} |")


if __name__ == "__main__":
    main()
