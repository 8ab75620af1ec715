"""The penalty kernels next to pk_sample / pk_logprobs at the 8B decode shape (B = 64 rows,
V = 128,256, bf16 logits).

Device-event times per call (graph replays of 20 back-to-back calls): pk_penalty_apply with no
row penalised (what every decode step pays; yardstick: pk_logprobs n_top = -1 in the same run)
and with all rows penalised (yardstick: its bytes, V * (2 + 2 + 4) per row, as a share of HBM
bandwidth), pk_penalty_update, and pk_sample_alt without alt rows against pk_sample (greedy and
top-k + top-p; pk_sample runs twice, its own repeat spread is the margin).  Prints a markdown
table (profiles/penalties_kernel.md).

Usage: ``python tools/bench_penalties.py [--rows 64] [--vocab 128256] [--iters 400] [--hbm-tbs 8.0]``
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.ops import penalties, sampler  # noqa: E402

CALLS_PER_GRAPH = 20


def timed(fn, iters):
    """us per call, from device events around replays of a graph of CALLS_PER_GRAPH back-to-back
    calls (tools/bench_logprobs.py: a Python launch loop would time the host's launch rate)."""
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
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the share is stated against")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, V = a.rows, a.vocab
    torch.manual_seed(0)
    x = (torch.randn(B, V, device="cuda") * 3).to(torch.bfloat16)
    full = lambda v, dt: torch.full((B,), v, dtype=dt, device="cuda")
    seeds, offs = torch.arange(B, dtype=torch.int32, device="cuda"), full(3, torch.int32)
    toks = torch.randint(0, V, (B,), dtype=torch.int32, device="cuda")
    st = penalties.PenaltyState(B, V, "cuda")
    # a history of 2,000 prompt and 500 generated tokens per slot, 300 biases
    g = torch.Generator().manual_seed(1)
    n_p, n_o, n_b = 2000, 500, penalties.MAX_BIAS
    per = n_p + n_o + 2 * n_b
    ids = torch.randint(0, V, (B, per), generator=g, dtype=torch.int32)
    for b in range(B):
        ids[b, n_p + n_o:n_p + n_o + n_b] = torch.randperm(V, generator=g)[:n_b].to(torch.int32)
    ids[:, n_p + n_o + n_b:] = (torch.rand(B, n_b, generator=g) * 10 - 5).view(torch.int32)
    entries = torch.tensor([[b, b * per, n_p, n_o, n_b, 1] for b in range(B)], dtype=torch.int32)
    penalties.seed(st, entries.cuda().reshape(-1), B, ids.cuda().reshape(-1), B * per)
    torch.cuda.synchronize()
    none, every = full(-1, torch.int32), torch.arange(B, dtype=torch.int32, device="cuda")
    rep, freq, pres = full(1.3, torch.float32), full(0.37, torch.float32), full(0.11, torch.float32)
    rows = []
    penalties.apply(st, x, every, rep, freq, pres)  # st.out holds the penalised rows pk_sample_alt reads below
    torch.cuda.synchronize()

    def sample(temp, k, p, alt):
        args = (full(temp, torch.float32), full(k, torch.int32), full(p, torch.float32), full(0.0, torch.float32),
                seeds, offs)
        kw = dict(alt=st.out, alt_slots=alt) if alt is not None else {}
        return timed(lambda: sampler.sample(x, *args, out=toks, **kw), a.iters)

    for name, (t, k, p) in (("greedy", (0.0, 0, 1.0)), ("top-k 50 + top-p 0.9 (T = 0.8)", (0.8, 50, 0.9))):
        rows.append((f"pk_sample {name}", sample(t, k, p, None)))
        rows.append((f"pk_sample {name}, repeated", sample(t, k, p, None)))
        rows.append((f"pk_sample_alt {name}, no alt rows", sample(t, k, p, none)))
        rows.append((f"pk_sample_alt {name}, every row from the fp32 copy", sample(t, k, p, every)))
    lp_out = torch.zeros((B, sampler.LOGPROB_WORDS), dtype=torch.int32, device="cuda")
    rows.append(("pk_logprobs n_top = -1", timed(lambda: sampler.logprobs(x, toks, none, lp_out), a.iters)))
    rows.append(("pk_penalty_apply, no row penalised",
                 timed(lambda: penalties.apply(st, x, none, rep, freq, pres), a.iters)))
    t_all = timed(lambda: penalties.apply(st, x, every, rep, freq, pres), a.iters)
    rows.append(("pk_penalty_apply, every row penalised", t_all))
    rows.append(("pk_penalty_update, every row", timed(lambda: penalties.update(st, every, toks, B), a.iters)))
    rows.append(("pk_penalty_update, no row", timed(lambda: penalties.update(st, none, toks, B), a.iters)))
    nbytes = B * V * (2 + 2 + 4)
    print(f"B = {B}, V = {V}, bf16 logits ({B * V * 2 / 1e6:.1f} MB), {a.iters} calls each "
          f"(graphs of {CALLS_PER_GRAPH}), device events\n")
    print("| kernel | us / call |\n|---|---|")
    for name, us in rows:
        print(f"| {name} | {us:.1f} |")
    tbs = nbytes / (t_all * 1e-6) / 1e12
    print(f"\npk_penalty_apply, every row: {nbytes / 1e6:.1f} MB in {t_all:.1f} us = {tbs:.2f} TB/s "
          f"({100 * tbs / a.hbm_tbs:.0f} % of {a.hbm_tbs:.1f} TB/s)")


if __name__ == "__main__":
    main()
