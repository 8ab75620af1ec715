"""pk_logprobs next to pk_sample at the 8B decode shape (B = 64 rows, V = 128,256, bf16 logits).

Device-event times per call (graph replays of 20 back-to-back calls), every row at the same
``n_top`` (-1 = nobody asked: the launch every decode step pays; 0 = sampled token only; 5; 20),
and pk_sample on the same logits for greedy rows and for top-k + top-p rows (the yardstick: a
comparable number of passes over the row).  Prints a markdown table
(profiles/logprobs_kernel.md).

Usage: ``python tools/bench_logprobs.py [--rows 64] [--vocab 128256] [--iters 400]``
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.ops import sampler  # noqa: E402

CALLS_PER_GRAPH = 20


def timed(fn, iters):
    """us per call, from device events around replays of a graph of CALLS_PER_GRAPH back-to-back
    calls: the engine launches these kernels from a graph too, and a Python launch loop would
    time the host's launch rate (~8 us per call) instead of the kernel."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, V = a.rows, a.vocab
    torch.manual_seed(0)
    x = (torch.randn(B, V, device="cuda") * 3).to(torch.bfloat16)
    full = lambda v, dt: torch.full((B,), v, dtype=dt, device="cuda")
    seeds, offs = torch.arange(B, dtype=torch.int32, device="cuda"), full(3, torch.int32)
    toks = torch.empty(B, dtype=torch.int32, device="cuda")
    rows = []

    def sample(temp, k, p):
        args = (full(temp, torch.float32), full(k, torch.int32), full(p, torch.float32), full(0.0, torch.float32),
                seeds, offs)
        return timed(lambda: sampler.sample(x, *args, out=toks), a.iters)

    rows.append(("pk_sample greedy", sample(0.0, 0, 1.0)))
    rows.append(("pk_sample top-k 50 + top-p 0.9 (T = 0.8)", sample(0.8, 50, 0.9)))
    out = torch.zeros((B, sampler.LOGPROB_WORDS), dtype=torch.int32, device="cuda")
    for n in (-1, 0, 5, 20):
        nt = full(n, torch.int32)
        rows.append((f"pk_logprobs n_top = {n}", timed(lambda: sampler.logprobs(x, toks, nt, out), a.iters)))
    print(f"B = {B}, V = {V}, bf16 logits ({B * V * 2 / 1e6:.1f} MB), {a.iters} calls each "
          f"(graphs of {CALLS_PER_GRAPH}), device events\n")
    print("| kernel | us / call |\n|---|---|")
    for name, us in rows:
        print(f"| {name} | {us:.1f} |")


if __name__ == "__main__":
    main()
