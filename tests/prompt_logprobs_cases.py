"""Shared checkers of the prompt-logprobs tests: a float64 reference of one scored row (independent of
ops/reference.py), the constructed rows that separate the tie rules, and a checker of
``model_runner.prompt_targets``.  tests/unit/test_prompt_logprobs_cases.py proves that each checker
rejects the mutants it is there to catch."""
import torch

from polykey_service_amd.engine.sequence import SamplingParams, Sequence

NMAX = 20
NINF = float("-inf")


# ------------------------------------------------------------------ one row, exactly
def reference_rows(x: torch.Tensor, V: int, targets, n_top):
    """Per row None (not asked: ``targets < 0`` or ``n_top < 0``) or ``(logprob, rank, ids, list
    logprobs)`` in float64.  rank = 1 + #{j : x_j > x_t, or x_j == x_t and j < t} with -0.0 == +0.0
    (0 for a target >= V); ids: the n largest in (value descending, id ascending) order, padded with
    -1 / -inf to 20.  A row whose maximum is -inf has logprob -inf everywhere."""
    out = []
    for r in range(x.shape[0]):
        t, n = int(targets[r]), int(n_top[r])
        if t < 0 or n < 0:
            out.append(None)
            continue
        row = x[r, :V].double()
        row = torch.where(row == 0, torch.zeros_like(row), row)  # -0.0 == +0.0
        m = row.max()
        dead = bool(torch.isneginf(m))
        lse = NINF if dead else float(m + torch.log(torch.exp(row - m).sum()))
        if t < V:
            xt = row[t]
            rank = 1 + int((row > xt).sum()) + int((row[:t] == xt).sum())
            lp = NINF if dead or bool(torch.isneginf(xt)) else float(xt) - lse
        else:
            rank, lp = 0, NINF
        n = min(n, NMAX, V)
        vals, idx = torch.sort(row, descending=True, stable=True)
        ids = idx[:n].tolist() + [-1] * (NMAX - n)
        top = [NINF if dead or v == NINF else v - lse for v in vals[:n].tolist()] + [NINF] * (NMAX - n)
        out.append((lp, rank, ids, top))
    return out


def tie_rows(V: int = 64):
    """Rows (fp32, exact small values) on which the tie rules differ: → (x [R, V], targets [R])."""
    x = torch.zeros(5, V)
    x[0, :] = 1.5                       # all equal
    x[1, :] = (torch.arange(V) % 7).float()  # runs of ties at every level
    x[2, :] = 0.0
    x[2, 1::2] = -0.0                   # signed zeros
    x[3, :] = -2.0
    x[3, [3, V // 2, V - 1]] = 7.0      # the maximum three times
    x[4, :] = torch.arange(V).float()   # no ties
    x[4, ::5] = NINF
    targets = torch.tensor([V // 2, 9, V - 1, V // 2, 10], dtype=torch.int32)
    return x, targets


def check_rows(fn, x, targets, n: int = 5):
    """``fn(row fp32 [V], target, n) -> (rank, ids[:n])`` against the reference on every row."""
    V = x.shape[1]
    want = reference_rows(x, V, targets, torch.full((x.shape[0],), n, dtype=torch.int32))
    for r, (_, wrank, wids, _) in enumerate(want):
        rank, ids = fn(x[r], int(targets[r]), n)
        assert rank == wrank, (r, rank, wrank)
        assert list(ids) == wids[:n], (r, list(ids), wids[:n])


# ------------------------------------------------------------------ targets of a step's rows
def make_seq(prompt, n_top=0, recorded=(), outputs=(), asks=True):
    s = Sequence("r", list(prompt), SamplingParams(prompt_logprobs=n_top if asks else None))
    s.output_ids = list(outputs)
    for i in recorded:
        s.prompt_logprobs[i] = (-1.0, 1, [])
        s.prompt_lp_missing -= 1
    return s


def target_scenarios():
    """Steps as ``prompt_targets`` sees them, every token id distinct: → [(name, chunks)]."""
    a = make_seq(range(100, 106))                          # P = 6, asks
    b = make_seq(range(200, 203), n_top=3)                 # P = 3, asks
    c = make_seq(range(300, 304), asks=False, outputs=[310])
    d = make_seq(range(400, 408), recorded=range(1, 5), outputs=[410, 411])  # preempted: entries 1..4 exist
    e = make_seq(range(500, 504), recorded=range(1, 4), outputs=[510])       # complete: asks nothing more
    return [
        ("non-final chunk of A, then all of B", [(a, 0, 4), (b, 0, 3)]),
        ("decode row of C, final chunk of A", [(c, 4, 1), (a, 4, 2)]),
        ("recompute of D over prompt and outputs", [(d, 0, 10)]),
        ("recompute of D in two chunks", [(d, 0, 3), (b, 0, 2)]),
        ("complete E recomputed next to A", [(e, 0, 5), (a, 0, 6)]),
        ("one-row last chunk of B as a decode row", [(b, 2, 1)]),
    ]


def expected_targets(chunks):
    """The rule, spelled out position by position."""
    out = []
    for seq, start, length in chunks:
        for p in range(start, start + length):
            want = -1
            rec = seq.prompt_logprobs
            if rec is not None and p + 1 < len(seq.prompt_ids) and rec[p + 1] is None:
                want = seq.prompt_ids[p + 1]
            out.append(want)
    return out


def check_targets(fn):
    for name, chunks in target_scenarios():
        got = list(fn(chunks))
        assert got == expected_targets(chunks), (name, got, expected_targets(chunks))
