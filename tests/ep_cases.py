"""The contract of the IPC expert all-to-all (csrc/comm/ep_alltoall.hip), modelled on the CPU, with
the inputs, criteria and mutants shared by tests/parallel/test_ep_alltoall_exact_gpu.py (the HIP
kernels) and tests/unit/test_ep_cases.py (the CPU proof that those tests can fail).

Nothing here is taken from ``polykey_service_amd``: the model is written from the header comment of
ep_alltoall.hip and the docstrings of ``EpAllToAll.dispatch`` / ``return_``.

Contract (W ranks, capacity C rows per (source, destination) pair, rows of H bf16)
  dispatch   rank s holds send_x [n, H] sorted by destination, send_e [n] and offsets [W + 1]: the
             rows of destination d are [offsets[d], offsets[d+1]), n_sd of them.  After the call
             recv_x[d][s C + i] = send_x[s][offsets_s[d] + i] and recv_e[d][s C + i] = the matching id
             for i < n_sd, recv_e[d][s C + i] = -1 for n_sd <= i < C, and every other row of recv_x is
             left as it was.
  return     ret_x[s][offsets_s[d] + i] = y[d][s C + i] for i < n_sd: the source gets its rows back in
             the order it sent them.  Rows of ret_x at and above the rank's total are left as they were.

Data
  rows       bit patterns, not values: bf16 tensors are int16 views here, filled with a hash of
             (source rank, call number, send row, column) and a few planted -0 / NaN / -inf patterns.
             A copy kernel preserves bits, so every comparison is ``torch.equal`` of integers.
  ids        a hash of (source rank, call number, send row) in [0, 8).
  "expert"   y_bits[d][s C + i] = recv_x_bits ^ key(d, recv_e): a 16-bit key that differs per
             (destination rank, expert id).  A returned row proves that it went to the right rank, carried
             the right id and came back to the right place in the send order.
  sentinels  SENT_X in recv_x and ret_x; SENT_E = 7, a valid-looking local expert id, in recv_e, so
             padding that is not written stays a plausible id and fails the comparison with -1.

Every rank can compute every other rank's send data from (world, shape, call number) alone.
"""
from typing import List, NamedTuple, Optional

import torch

SENT_X = 0x5A5A
SENT_E = 7
I16, I32 = torch.int16, torch.int32

# name -> (C, H).  A: one 16-byte unit per row, fewer rows than the 64 workgroups.  B: 257 units, so
# the 256-thread column loop makes a second trip with a remainder of one, and up to 200 rows to one
# peer, so the 64-workgroup row loop makes three or four trips.  C: with n = C to one peer the id-copy
# loop (stride 64 x 256 = 16384) makes its second trip, with n = 3 the padding loop does.
SHAPES = {"A": (40, 8), "B": (200, 2056), "C": (16400, 8)}
WORLDS = (2, 3, 4, 8)
# the call sequence: call number = index.  "small" follows "full" with the same target rank, so that
# rank's regions shrink from C rows to 3; "idle": the ranks with (rank + call) odd send nothing (call
# 4: the odd ranks, call 5: the even ones).
CALLS = ("even", "full", "small", "self", "idle", "idle", "edges", "bits")
TARGET = 1  # the rank "full" and "small" aim at
_M31 = (1 << 31) - 1


def _mix(v: torch.Tensor) -> torch.Tensor:
    v = ((v ^ (v >> 15)) * 0x2C1B3C6D) & _M31
    v = ((v ^ (v >> 12)) * 0x297A2D39) & _M31
    return v ^ (v >> 15)


def to_i16(v: torch.Tensor) -> torch.Tensor:
    """The low 16 bits of an integer tensor as int16 (two's complement, no out-of-range cast)."""
    return (((v & 0xFFFF) ^ 0x8000) - 0x8000).to(I16)


def counts(world: int, C: int, call: int) -> List[List[int]]:
    """n[s][d]: rows rank s sends rank d in call ``call``; a rank's total never exceeds C."""
    W, kind = world, CALLS[call]
    n = [[0] * W for _ in range(W)]
    for s in range(W):
        if kind == "even":
            for d in range(W):
                n[s][d] = max(C // W - (s + 2 * d + call) % 3, 0)
        elif kind == "full":
            n[s][TARGET] = C
        elif kind == "small":
            for d in range(W):
                n[s][d] = 3 if d == TARGET else (s + d) % 2
        elif kind == "self":
            n[s][s] = max(C // 2 - s, 1)
        elif kind == "idle":
            if (s + call) % 2 == 0:
                for d in range(W):
                    n[s][d] = max(C // W - d % 2, 0)
        elif kind == "edges":
            base = min(64, C // 3)
            for j, c in enumerate((base - 1, base, base + 1) if W >= 3 else (base - 1, base + 1)):
                n[s][(s + j) % W] = c
        elif kind == "bits":
            for d in range(W):
                n[s][d] = int(_mix(torch.tensor(s * 8 + d + call * 64 + 12345))) & 1
        assert sum(n[s]) <= C and all(0 <= c <= C for c in n[s])
    return n


class Send(NamedTuple):
    x: torch.Tensor    # [n, H] int16: the bits of the bf16 rows, sorted by destination
    e: torch.Tensor    # [n] int32
    off: torch.Tensor  # [W + 1] int32


def row_bits(src: int, call: int, rows: int, H: int) -> torch.Tensor:
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(H, dtype=torch.int64)[None, :]
    b = _mix((r * 0x9E3779B + c * 0x85EBCA7 + src * 0xC2B2AE3 + call * 0x27D4EB2 + 0x1656671) & _M31) & 0xFFFF
    if rows:
        b[0, 0], b[0, 1], b[0, 2], b[0, 3] = 0x8000, 0x7FC1, 0xFF80, 0x7F81  # -0, quiet NaN, -inf, signalling NaN
        b[rows - 1, H - 1] = 0xFFFF
    return to_i16(b)


def row_ids(src: int, call: int, rows: int) -> torch.Tensor:
    r = torch.arange(rows, dtype=torch.int64)
    return (_mix((r * 0x9E3779B + src * 0xC2B2AE3 + call * 0x27D4EB2 + 77) & _M31) % 8).to(I32)


def make_sends(world: int, shape: str, call: int) -> List[Send]:
    """What every rank sends in call ``call``."""
    C, H = SHAPES[shape]
    out = []
    for s, row in enumerate(counts(world, C, call)):
        off = torch.tensor([0] + row, dtype=torch.int64).cumsum(0).to(I32)
        total = int(off[-1])
        out.append(Send(row_bits(s, call, total, H), row_ids(s, call, total), off))
    return out


def key(d, e: torch.Tensor) -> torch.Tensor:
    """int16 key of (destination rank, expert id >= -1): multiplication by an odd number is a bijection
    of the 16-bit integers, so the keys of the 8 x 16 pairs all differ.  Integer tensor ops only."""
    return to_i16((e.to(I32) + d * 16 + 1) * 40503)


def expert_bits(d: int, recv_x: torch.Tensor, recv_e: torch.Tensor) -> torch.Tensor:
    """The "expert" of rank d over all W C rows of its receive regions (int16 in, int16 out)."""
    return recv_x ^ key(d, recv_e)[:, None]


class Buffers:
    """recv_x / recv_e / ret_x of W ranks, filled with the sentinels."""

    def __init__(self, world: int, C: int, H: int):
        self.recv_x = [torch.full((world * C, H), SENT_X, dtype=I16) for _ in range(world)]
        self.recv_e = [torch.full((world * C,), SENT_E, dtype=I32) for _ in range(world)]
        self.ret_x = [torch.full((C, H), SENT_X, dtype=I16) for _ in range(world)]


DISPATCH_MUTANTS = ("rows_from_64_dropped", "columns_from_unit_256_dropped", "region_swapped", "ids_without_lo",
                    "padding_not_written", "padding_first_16384_only", "ids_from_16384_not_copied",
                    "one_row_too_many")
RETURN_MUTANTS = ("return_ignores_offset", "return_uses_destination_offsets", "return_one_row_past_total")
MUTANTS = DISPATCH_MUTANTS + RETURN_MUTANTS


def dispatch_ref(world: int, C: int, sends: List[Send], bufs: Buffers, mutant: Optional[str] = None) -> None:
    """One dispatch call of all ranks, in place on ``bufs.recv_x`` / ``bufs.recv_e``."""
    assert mutant is None or mutant in MUTANTS
    for d in range(world):
        rx, re = bufs.recv_x[d], bufs.recv_e[d]
        for s in range(world):
            x, e, off = sends[s]
            lo, n = int(off[d]), int(off[d + 1]) - int(off[d])
            base = (d if mutant == "region_swapped" else s) * C
            nx = min(n, 64) if mutant == "rows_from_64_dropped" else n
            if mutant == "columns_from_unit_256_dropped":
                rx[base:base + nx, :2048] = x[lo:lo + nx, :2048]
            else:
                rx[base:base + nx] = x[lo:lo + nx]
            if mutant == "one_row_too_many" and n < C:  # the next send row, or zeros past the last
                rx[base + n] = x[lo + n] if lo + n < x.shape[0] else 0
            ne = min(n, 16384) if mutant == "ids_from_16384_not_copied" else n
            re[base:base + ne] = e[:ne] if mutant == "ids_without_lo" else e[lo:lo + ne]
            if mutant == "padding_first_16384_only":
                re[base + n:base + min(C, n + 16384)] = -1
            elif mutant != "padding_not_written":
                re[base + n:base + C] = -1


def return_ref(world: int, C: int, y: List[torch.Tensor], sends: List[Send], bufs: Buffers,
               mutant: Optional[str] = None) -> None:
    """One return call of all ranks, in place on ``bufs.ret_x``.  y[d]: [W C, H] int16."""
    assert mutant is None or mutant in MUTANTS
    for s in range(world):
        rt, off = bufs.ret_x[s], sends[s].off
        total = int(off[-1])
        if mutant == "return_one_row_past_total" and total < C:
            rt[total] = y[world - 1][s * C + min(int(off[world]) - int(off[world - 1]), C - 1)]
        for d in range(world):
            lo, n = int(off[d]), int(off[d + 1]) - int(off[d])
            if mutant == "return_ignores_offset":
                lo = 0
            elif mutant == "return_uses_destination_offsets":
                lo = int(sends[d].off[s])
            n = max(min(n, C - lo), 0)
            rt[lo:lo + n] = y[d][s * C:s * C + n]


def _first_bad(got: torch.Tensor, want: torch.Tensor):
    bad = (got != want).reshape(got.shape[0], -1).any(-1).nonzero().flatten()
    return int(bad.numel()), bad[:4].tolist()


def check_dispatch(rank: int, world: int, C: int, recv_x: torch.Tensor, recv_e: torch.Tensor, sends: List[Send],
                   before_x: torch.Tensor):
    """Rank ``rank``'s receive regions after a dispatch of ``sends``: recv_x [W C, H] int16 and recv_e
    [W C] int32 as found, before_x what recv_x held before the call.  Asserts the contract bit for bit
    and returns the expected (recv_x, recv_e).  A gather over all W C rows at once, not the loops of
    dispatch_ref."""
    assert recv_x.dtype == I16 and recv_e.dtype == I32 and recv_x.shape == before_x.shape
    assert recv_x.shape[0] == world * C and recv_e.shape == (world * C,)
    lo = torch.tensor([int(s.off[rank]) for s in sends])
    n = torch.tensor([int(s.off[rank + 1]) - int(s.off[rank]) for s in sends])
    start = torch.tensor([0] + [s.x.shape[0] for s in sends]).cumsum(0)[:-1]
    all_x, all_e = torch.cat([s.x for s in sends]), torch.cat([s.e for s in sends])
    row = torch.arange(world * C)
    src, i = row // C, row % C
    valid = i < n[src]
    at = (start[src] + lo[src] + i)[valid]
    want_x = before_x.clone()
    want_x[valid] = all_x[at]
    want_e = torch.full((world * C,), -1, dtype=I32)
    want_e[valid] = all_e[at]
    if not torch.equal(recv_e, want_e):
        cnt, rows = _first_bad(recv_e, want_e)
        raise AssertionError(("recv_e", rank, cnt, [(r // C, r % C, int(recv_e[r]), int(want_e[r])) for r in rows],
                              n.tolist()))
    if not torch.equal(recv_x, want_x):
        cnt, rows = _first_bad(recv_x, want_x)
        raise AssertionError(("recv_x", rank, cnt, [(r // C, r % C, "sent" if bool(valid[r]) else "untouched")
                                                    for r in rows], n.tolist()))
    return want_x, want_e


def check_return(rank: int, world: int, C: int, ret_x: torch.Tensor, sends: List[Send], before_ret: torch.Tensor):
    """Rank ``rank``'s ret_x [C, H] int16 after the return of a call whose receivers applied
    ``expert_bits``: row j, sent to rank d with id e, is back at row j as bits ^ key(d, e); rows at and
    above the rank's total are as before.  Returns the expected ret_x.  Computed from the send data
    alone, not from a model of the receivers."""
    assert ret_x.dtype == I16 and ret_x.shape == before_ret.shape and ret_x.shape[0] == C
    x, e, off = sends[rank]
    total = int(off[-1])
    dest = torch.bucketize(torch.arange(total), off[1:].long(), right=True)
    want = before_ret.clone()
    want[:total] = x ^ key(dest.to(I32), e)[:, None]
    if not torch.equal(ret_x, want):
        cnt, rows = _first_bad(ret_x, want)
        raise AssertionError(("ret_x", rank, cnt, [(r, int(dest[r]) if r < total else "untouched") for r in rows],
                              off.tolist()))
    return want


# ------------------------------------------------------------------------ the MoE layer over EP
MOE_E, MOE_K, MOE_H, MOE_I, MOE_C = 8, 2, 256, 256, 64
MOE_BIG = 24  # tokens of the busiest rank; its first 18 route to expert 0
# world -> rounds of per-rank token counts: a 0 (an idle rank that still serves its peers), a 1 and a
# 24 at every world size (two rounds where two ranks cannot hold all three)
MOE_TOKENS = {2: ((0, MOE_BIG), (1, 3)), 4: ((0, 1, MOE_BIG, 5),), 8: ((0, 1, MOE_BIG, 5, 3, 2, 7, 4),)}


def moe_routes(rank: int, T: int):
    """(first, second) expert of every token of a rank: the first 18 tokens go to expert 0 first, so
    with 24 tokens its owner (rank 0, which has no token of its own in that round) gets more than one
    16-row tile for it from a peer; expert 7 is never used."""
    out = []
    for t in range(T):
        first = 0 if t < 18 else (t + rank) % 7
        second = 1 + (3 * t + rank) % 6
        if second == first:
            second = second % 6 + 1
        out.append((first, second))
    return out


def moe_operands(world: int, rnd: int):
    """In the style of moe_cases.MoeCase.build -> (xs, router, w13, w2): xs[r] [T_r, H] bf16 with grid
    logits in the first E columns (the largest 1 to 1.5 above the second) and integers elsewhere, a
    one-hot router, and ONE integer weight set for all ranks, NaN in every expert that no rank's token
    routes to."""
    import numpy as np
    E, H, I = MOE_E, MOE_H, MOE_I
    xs, used = [], set()
    for r, T in enumerate(MOE_TOKENS[world][rnd]):
        g = torch.Generator().manual_seed(1000 * world + 100 * rnd + r)
        rng = np.random.default_rng(1000 * world + 100 * rnd + r)
        x = (torch.randint(0, 2, (T, H), generator=g) + 1.0) * (torch.randint(0, 2, (T, H), generator=g) * 2.0 - 1)
        for t, (first, second) in enumerate(moe_routes(r, T)):
            gaps = rng.integers(1, 17, size=E - 1) / 8
            gaps[0] = rng.integers(8, 13) / 8
            gaps[1] = rng.integers(1, 5) / 8
            v = rng.integers(0, 33) / 8 - np.concatenate([[0.0], np.cumsum(gaps)])
            rest = [e for e in rng.permutation(E) if e not in (first, second)]
            x[t, [first, second] + rest] = torch.from_numpy(v).float()
            used.update((first, second))
        xs.append(x.to(torch.bfloat16))
    g = torch.Generator().manual_seed(77 + 10 * world + rnd)
    router = torch.zeros(E, H)
    router[torch.arange(E), torch.arange(E)] = 1.0
    w13 = torch.randint(0, 2, (E, 2 * I, H), generator=g) * 2.0 - 1
    w13[:, :, :E] = 0
    w2 = torch.randint(0, 2, (E, H, I), generator=g) * 2.0 - 1
    for e in range(E):
        if e not in used:
            w13[e] = float("nan")
            w2[e] = float("nan")
    b = torch.bfloat16
    return xs, router.to(b), w13.to(b), w2.to(b)
