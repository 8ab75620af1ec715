"""Float64 references, inputs, criteria and mutants shared by the exact MoE tests:
tests/kernels/test_moe_exact.py (the HIP kernels) and tests/unit/test_moe_cases.py (the CPU proof
that those tests can fail).

Everything here runs on the CPU and nothing is taken from ``polykey_service_amd.ops``: the
references are written from the comments of csrc/kernels/moe.hip, skinny_tile.h and gemm_prefill.hip.

Inputs
  grid logits     multiples of 1/8 in [-16, 16]: exact in bf16, ``l - max`` exact in fp32, and any two
                  either tied exactly or 0.125 apart, so ``exp`` cannot reorder them and the expert ids
                  must equal the reference's on every row.  Rows carry planted ties at and across the
                  k-th place and -inf entries (never a whole row).
  integer GEMMs   A in {+-1, +-2}, W in {+-1}: every partial sum is an integer, exact in fp32 in any
                  order; every full sum is asserted to be at most 256 in magnitude, exact in bf16.  The
                  expected output is the integer itself, bit for bit.
  poison          NaN weights for experts without rows, NaN A rows past ``offsets[-1]``, NaN token
                  rows no local slot reads, outputs pre-filled with a finite sentinel.

Criteria (u = 2^-8, one bf16 ulp at 1)
  route weights   |w - w64| <= W_RTOL |w64|
  combine         |out - ref64| <= u |ref64| + k 2^-23 sum_j |w_j y_j|
  norm x, SiLU    |out - ref64| <= 2.25 u |ref64|   (two bf16 roundings + 0.25 u for rsqrtf / exp)
  end to end      |out - moe64| <= 4.25 u sum_j w_j sum_i |h_ji w2_ji|
Each ``check_*`` raises AssertionError or returns the largest error / bound ratio it saw.
"""
import dataclasses

import numpy as np
import torch

U = 2.0 ** -8
NINF = float("-inf")
SENT = -24576.0     # finite sentinel, exact in bf16 and fp32; no test input produces it
SENT_I = -7777      # int32 sentinel

# Relative error of the routing weights against float64.  Largest value measured on the MI355X over
# ROUTE_CASES, both renorm values: 1.95e-6 from pk_moe_topk_softmax and 1.82e-6 from the routing
# norm kernel, both at (5, 64, 64), where the smallest weights are exp(-32) of the largest (the error
# of the fast exp grows with its argument; the cases with k <= 4 stay below 9e-7).  Times 4 for the
# spread of the fast exp at a 32-wide logit range: 7.8e-6.  The ceiling the older test used is 1e-5.
W_RTOL = 4 * 1.95e-6


def bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16, back in float64."""
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------- routing
def route64(logits: torch.Tensor, k: int, renorm: bool, tie_high: bool = False):
    """softmax over experts in float64, then the k largest with ties to the lower expert id
    (``tie_high``: mutant, ties to the higher id) -> (ids [T, k] int64, weights [T, k] float64)."""
    l = logits.double()
    p = torch.softmax(l, -1)
    if tie_high:
        E = l.shape[1]
        order = (E - 1) - torch.sort(l.flip(-1), dim=-1, descending=True, stable=True).indices
    else:
        order = torch.sort(l, dim=-1, descending=True, stable=True).indices
    ids = order[:, :k]
    w = torch.gather(p, 1, ids)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    return ids, w


def grid_logits(T: int, E: int, k: int, seed: int) -> torch.Tensor:
    """[T, E] bf16 grid logits.  Each row draws E distinct grid values, then by row % 4:
      0  the k-th and (k+1)-th largest tied (k == E: the last two)
      1  the two largest tied
      2  a three-way tie around the k-th place
      3  no tie
    Every row with row % 5 == 4 has about half its entries at -inf (never the largest)."""
    g = np.random.default_rng(seed)
    out = np.empty((T, E))
    for t in range(T):
        v = g.choice(257, size=E, replace=False).astype(np.float64) / 8 - 16
        order = np.argsort(-v, kind="stable")
        kind = t % 4
        if E >= 2 and kind == 0:
            a = min(k, E - 1)
            v[order[a]] = v[order[a - 1]]
        elif E >= 2 and kind == 1:
            v[order[1]] = v[order[0]]
        elif E >= 3 and kind == 2:
            a = min(max(k, 1), E - 2)
            v[order[a]] = v[order[a + 1]] = v[order[a - 1]]
        if t % 5 == 4:
            drop = g.permutation(order[1:])[: E // 2]
            v[drop] = NINF
        out[t] = v
    return torch.from_numpy(out).to(torch.bfloat16)


# (T, E, k): one token; the second workgroup; E = 64 (bit 63 of `taken`); k == E; E = 3, k = 1
ROUTE_CASES = ((1, 8, 2), (257, 8, 2), (300, 64, 4), (5, 64, 64), (40, 3, 1))


def strided(logits: torch.Tensor, pad: int = 5) -> torch.Tensor:
    """The logits as a column slice of a wider buffer whose other columns hold +16 (the largest
    grid value): a kernel that ignored the stride would read them."""
    T, E = logits.shape
    buf = torch.full((T, E + pad), 16.0, dtype=logits.dtype)
    buf[:, 2:2 + E] = logits
    return buf


def check_route(ids, w, logits, k, renorm, rtol=W_RTOL, rows=None):
    """ids equal to route64 on every row (of ``rows``), distinct and in [0, E); weights within
    ``rtol`` (a number or one per row) of float64 in relative error."""
    T, E = logits.shape
    ids = torch.as_tensor(ids).long().reshape(T, k)
    w = torch.as_tensor(w).double().reshape(T, k)
    rids, rw = route64(logits, k, renorm)
    sel = torch.ones(T, dtype=torch.bool) if rows is None else rows
    assert bool(((ids >= 0) & (ids < E)).all()), "expert id out of range"
    assert bool((torch.sort(ids, -1).values.diff(dim=-1) > 0).all()), "repeated expert id in a row"
    bad = (ids != rids).any(-1) & sel
    assert not bool(bad.any()), ("ids differ from route64", bad.nonzero().flatten()[:8].tolist())
    tol = torch.as_tensor(rtol, dtype=torch.float64).reshape(-1, 1) * rw.abs()
    err = (w - rw).abs()
    assert bool(torch.isfinite(w).all()), "non-finite weight"
    over = (err > tol).any(-1) & sel
    assert not bool(over.any()), ("weights", over.nonzero().flatten()[:8].tolist(),
                                  float((err / rw.abs().clamp_min(1e-300))[sel].max()))
    rel = torch.where(rw != 0, err / rw.abs().clamp_min(1e-300), torch.zeros_like(err))
    return float(rel[sel].max()) if bool(sel.any()) else 0.0


ROUTE_NORM_H = 1024
ROUTE_NORM_NNZ = 24


def route_norm_case(T: int, E: int, seed: int, S: int, H: int = ROUTE_NORM_H):
    """Inputs of the split-K add + RMSNorm + route kernel whose router logits are exact, to be run
    with eps = 0 -> (slabs [S, T, H] fp32, residual [T, H], norm weight [H], router [E, H], the new
    residual v, the normalised rows x = v * nw, the logits [T, E]).

    The slabs are integers that sum to 0 or +-2 and the residual makes the new residual v = +-1
    everywhere, so mean(v^2) = 1 and x = v * nw with nw in {1, 2}, exactly.  The router has
    ROUTE_NORM_NNZ entries of +-1 per expert, spread over the row: every logit is an integer below
    256 in magnitude, exact in fp32 in any summation order and exact in bf16, ties included, so the
    ids must equal route64's on every row and no row has to be set aside."""
    g = torch.Generator().manual_seed(seed)
    total = (torch.randint(0, 3, (T, H), generator=g) - 1) * 2.0
    slabs = torch.randint(-3, 4, (S, T, H), generator=g).float()
    slabs[S - 1] = total - slabs[: S - 1].sum(0)
    sign = torch.randint(0, 2, (T, H), generator=g) * 2.0 - 1
    res = torch.where(total == 0, sign, -torch.sign(total))
    v = total + res
    nw = torch.randint(1, 3, (H,), generator=g).float()
    router = torch.zeros(E, H)
    for e in range(E):
        pos = torch.randperm(H, generator=g)[:ROUTE_NORM_NNZ]
        router[e, pos] = torch.randint(0, 2, (ROUTE_NORM_NNZ,), generator=g) * 2.0 - 1
    x = v * nw
    logits = x.double() @ router.double().t()
    assert float(v.abs().min()) == 1 == float(v.abs().max()) and float(logits.abs().max()) <= 256
    b = torch.bfloat16
    return slabs, res.to(b), nw.to(b), router.to(b), v.to(b), x.to(b), logits.to(b)


# --------------------------------------------------------------------------------------- align
def align_ref(ids, e_lo: int, e_hi: int, unstable: bool = False, keep_nonlocal: bool = False):
    """Stable counting sort of the slots by expert, slots outside [e_lo, e_hi) dropped ->
    (offsets [E_local + 1], sorted [m], inv [n]) as int64 numpy arrays; inv = -1 for dropped slots.
    Mutants: ``unstable`` reverses the slot order within each expert; ``keep_nonlocal`` files a
    non-local slot under the nearest local expert."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    El = e_hi - e_lo
    buckets = [[] for _ in range(El)]
    for i, e in enumerate(ids):
        if e_lo <= e < e_hi:
            buckets[e - e_lo].append(i)
        elif keep_nonlocal:
            buckets[min(max(e - e_lo, 0), El - 1)].append(i)
    offsets = np.zeros(El + 1, dtype=np.int64)
    order = []
    for e, b in enumerate(buckets):
        order += b[::-1] if unstable else b
        offsets[e + 1] = len(order)
    sorted_ = np.asarray(order, dtype=np.int64)
    inv = np.full(ids.shape[0], -1, dtype=np.int64)
    inv[sorted_] = np.arange(len(order))
    return offsets, sorted_, inv


@dataclasses.dataclass(frozen=True)
class AlignCase:
    name: str
    n: int
    E: int
    e_lo: int
    e_hi: int
    kind: str  # "mixed": random ids with -1 and E + 3 among them; "one": every slot to e_lo; "none": no local slot

    def ids(self) -> np.ndarray:
        g = np.random.default_rng(1000 + self.n + 7 * self.E + self.e_lo)
        if self.kind == "one":
            return np.full(self.n, self.e_lo, dtype=np.int32)
        if self.kind == "none":
            pool = [e for e in range(-1, self.E + 4) if not self.e_lo <= e < self.e_hi]
            return g.choice(pool, size=self.n).astype(np.int32)
        ids = g.integers(0, self.E, size=self.n).astype(np.int32)
        ids[g.random(self.n) < 0.1] = -1          # the padding of the expert-parallel IPC path
        ids[g.random(self.n) < 0.05] = self.E + 3
        return ids


ALIGN_CASES = tuple(
    [AlignCase(f"n{n}", n, 8, 0, 8, "mixed") for n in (0, 1, 1023, 1024, 1025, 2049)]
    + [AlignCase("El1", 1025, 8, 3, 4, "mixed"), AlignCase("El64", 2049, 64, 0, 64, "mixed"),
       AlignCase("El64_lo", 1024, 70, 6, 70, "mixed"), AlignCase("lo2", 1025, 8, 2, 6, "mixed"),
       AlignCase("one", 1025, 8, 2, 6, "one"), AlignCase("one_1024", 1024, 64, 63, 64, "one"),
       AlignCase("none", 1025, 8, 2, 6, "none"), AlignCase("none_1", 1, 8, 7, 8, "none")])


def check_align(offsets, sorted_, inv, ids, e_lo, e_hi, sentinel=SENT_I):
    """Against align_ref and, independently, the properties of a stable grouping.  ``sorted_`` has n
    entries pre-filled with ``sentinel``; only the first m = offsets[-1] may be written."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    offsets, sorted_, inv = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (offsets, sorted_, inv))
    n, El = ids.shape[0], e_hi - e_lo
    local = (ids >= e_lo) & (ids < e_hi)
    m = int(local.sum())
    assert offsets.shape[0] == El + 1 and offsets[0] == 0 and offsets[-1] == m, "offsets ends"
    assert np.array_equal(np.diff(offsets), np.bincount(ids[local] - e_lo, minlength=El)), "group sizes"
    head = sorted_[:m]
    assert np.array_equal(np.sort(head), np.nonzero(local)[0]), "sorted[:m] is not a permutation of the local slots"
    for e in range(El):
        seg = head[offsets[e]:offsets[e + 1]]
        assert np.all(ids[seg] == e + e_lo), ("slot under another expert", e)
        assert np.all(np.diff(seg) > 0), ("slots do not ascend within expert", e)
    assert np.array_equal(inv[head], np.arange(m)), "inv[sorted[p]] != p"
    assert np.all(inv[~local] == -1), "inv of a non-local slot"
    assert np.all(sorted_[m:] == sentinel), "sorted written past offsets[-1]"
    r_off, r_sorted, r_inv = align_ref(ids, e_lo, e_hi)
    assert np.array_equal(offsets, r_off) and np.array_equal(head, r_sorted) and np.array_equal(inv, r_inv)


# --------------------------------------------------------------------------- permute / combine
def permute_ref(x: torch.Tensor, sorted_, k: int) -> torch.Tensor:
    """out[p] = x[sorted[p] // k] for p < m."""
    return x[torch.as_tensor(np.asarray(sorted_, dtype=np.int64)) // k]


def combine64(y, inv, w, T: int, k: int, swap=False, keep_nonlocal=False, shift=False):
    """out[t] = sum_j w[t, j] y[inv[t k + j]] over the slots with inv >= 0, in float64 ->
    (out [T, H], sum_j |w y| [T, H]).  Mutants: ``swap`` exchanges the weights of slots 0 and 1;
    ``keep_nonlocal`` reads row 0 for inv = -1; ``shift`` writes token t's sum to token t + 1."""
    y = y.double()
    inv = torch.as_tensor(np.asarray(inv, dtype=np.int64)).reshape(T, k)
    w = torch.as_tensor(w).double().reshape(T, k)
    if swap and k >= 2:
        w = w[:, [1, 0] + list(range(2, k))]
    H = y.shape[1]
    out = torch.zeros((T, H), dtype=torch.float64)
    mag = torch.zeros((T, H), dtype=torch.float64)
    for j in range(k):
        p = inv[:, j]
        if keep_nonlocal:
            p = p.clamp(min=0)
        ok = p >= 0
        term = w[ok, j:j + 1] * y[p[ok]]
        out[ok] += term
        mag[ok] += term.abs()
    if shift:
        out, mag = out.roll(1, 0), mag.roll(1, 0)
    return out, mag


def check_combine(out, ref, mag, k):
    """|out - ref64| <= u |ref64| + k 2^-23 sum_j |w_j y_j|."""
    out = out.double()
    bound = U * ref.abs() + k * 2.0 ** -23 * mag
    err = (out - ref).abs()
    assert bool(torch.isfinite(out).all()), "non-finite output"
    assert bool((err <= bound).all()), ("combine", float((err - bound).max()))
    return float((err / bound.clamp_min(1e-300)).max())


def check_exact(out: torch.Tensor, ref: torch.Tensor, what="output"):
    """Bit equality (of the values: both are finite), sentinel rows included."""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    o, r = out.double(), ref.double()
    assert bool(torch.isfinite(o).all()), (what, "non-finite value")
    bad = o != r
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


def check_rel(out, ref, factor, what):
    """|out - ref64| <= factor u |ref64| -> the largest error / (u |ref64|)."""
    out = out.double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), (what, "non-finite value")
    err = (out - ref).abs()
    assert bool((err <= factor * U * ref.abs()).all()), (what, float((err / (U * ref.abs()).clamp_min(1e-300)).max()))
    return float((err / (U * ref.abs()).clamp_min(1e-300)).max())


def combine_case(T: int, k: int, H: int, integer: bool, seed: int, extra_rows: int = 3):
    """-> (y [R, H] bf16, inv [T k] int32, w [T, k] fp32): R = T k + extra rows, inv a random
    injection into the rows with about a quarter of the slots non-local (-1) and, for T >= 2, every
    slot of token 1 non-local.  ``integer``: y in {+-1, +-2, +-4} and w multiples of 1/8 in
    [1/8, 1], so every product and sum (|sum| <= 16, a multiple of 1/8) is exact in fp32 and bf16."""
    g = torch.Generator().manual_seed(seed)
    R = T * k + extra_rows
    inv = torch.randperm(R, generator=g)[: T * k].to(torch.int32)
    inv[torch.rand(T * k, generator=g) < 0.25] = -1
    if T >= 2:
        inv[k:2 * k] = -1
    inv[0] = max(int(inv[0]), 1)   # token 0 keeps a local slot
    if integer:
        y = (torch.randint(0, 3, (R, H), generator=g).float().exp2() * (torch.randint(0, 2, (R, H), generator=g) * 2 - 1))
        w = torch.randint(1, 9, (T, k), generator=g).float() / 8
        if k >= 2:
            w[:, 1] = torch.where(w[:, 1] == w[:, 0], (w[:, 0] * 8 % 8 + 1) / 8, w[:, 1])  # slots 0 and 1 differ
    else:
        y = torch.randn(R, H, generator=g)
        w = torch.rand(T, k, generator=g) + 0.05
        w = w / w.sum(-1, keepdim=True)
    return y.to(torch.bfloat16), inv, w.float()


def rmsnorm64(r: torch.Tensor, nw: torch.Tensor, eps: float) -> torch.Tensor:
    r = r.double()
    return r / torch.sqrt((r * r).mean(-1, keepdim=True) + eps) * nw.double()


# --------------------------------------------------------------------------------- grouped GEMM
def deinterleave(v: torch.Tensor, block: int = 16):
    """Columns [g0..g15, u0..u15, g16.., u16.., ...] of a gate/up projection interleaved by
    ``block`` -> (gate [R, I], up [R, I])."""
    R, N2 = v.shape
    v = v.reshape(R, N2 // (2 * block), 2, block)
    return v[:, :, 0].reshape(R, -1), v[:, :, 1].reshape(R, -1)


def silu64(g: torch.Tensor) -> torch.Tensor:
    return g.double() * torch.sigmoid(g.double())


def grouped64(a, w, offsets, k_lo=0, k_hi=None, next_expert=False, drop=()):
    """Rows [offsets[e], offsets[e+1]) of a times w[e]^T over k in [k_lo, k_hi), float64 ->
    [R, N]; rows in no group are NaN.  Mutants: ``next_expert`` uses w[e + 1]; ``drop``: k indices
    left out of the sum."""
    a, w = a.double(), w.double()
    offs = [int(o) for o in offsets]
    G, N, K = w.shape
    k_hi = K if k_hi is None else k_hi
    cols = [c for c in range(max(k_lo, 0), min(k_hi, K)) if c not in set(drop)]
    out = torch.full((a.shape[0], N), float("nan"), dtype=torch.float64)
    for e in range(G):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            we = w[(e + 1) % G] if next_expert else w[e]
            out[lo:hi] = a[lo:hi][:, cols] @ we[:, cols].t()
    return out


def with_sentinel(ref: torch.Tensor) -> torch.Tensor:
    """The rows no group owns (NaN in grouped64) hold the sentinel."""
    return torch.where(torch.isnan(ref), torch.full_like(ref, SENT), ref)


def silu_ref(full: torch.Tensor, swap=False, block=16) -> torch.Tensor:
    """SiLU(gate) * up of an interleaved float64 projection (NaN rows stay NaN)."""
    g, u = deinterleave(full, block)
    if swap:
        g, u = u, g
    return silu64(g) * u


@dataclasses.dataclass(frozen=True)
class GemmCase:
    """One grouped GEMM input: group sizes, trailing rows no group owns, N, K."""
    sizes: tuple
    N: int
    K: int
    max_rows: int
    tail: int = 3
    seed: int = 0

    @property
    def offsets(self):
        return [0] + list(np.cumsum(self.sizes))

    @property
    def id(self):
        return f"N{self.N}-K{self.K}-max{self.max_rows}"

    def build(self):
        """-> (A [R, K] bf16 with NaN tail rows, W [G, N, K] bf16 with NaN experts where the group is
        empty, offsets).  Gate sums are kept small (see int_operands)."""
        return int_operands(self.sizes, self.N, self.K, self.tail, self.seed)


GATE_FREE_K = 64


def int_operands(sizes, N, K, tail, seed):
    """Integer operands with poison.  A in {+-1, +-2}, W in {+-1}.  Asserts max |sum| <= 256.

    The gate rows of W (interleave block 16: rows n with (n // 16) % 2 == 0) are read as gates only
    by the SiLU epilogues.  SiLU(g) u leaves the normal range of fp32 and bf16 below g = -87, where a
    relative criterion means nothing, so gate sums are kept within about +-70: outside the last
    GATE_FREE_K columns A repeats each even column negated in the odd one, and the gate rows of W
    repeat it unchanged, so those pairs cancel exactly (every k element still enters the sum: leaving
    one out changes it by 1 or 2).  All other rows of W are free, and their sums over the same A have
    the full variance."""
    g = torch.Generator().manual_seed(seed)
    G, R = len(sizes), int(sum(sizes)) + tail
    offs = [0] + list(np.cumsum(sizes))
    A = (torch.randint(0, 2, (R, K), generator=g) + 1.0) * (torch.randint(0, 2, (R, K), generator=g) * 2.0 - 1)
    W = torch.randint(0, 2, (G, N, K), generator=g) * 2.0 - 1
    Z = K - GATE_FREE_K
    if Z > 0:
        A[:, 1:Z:2] = -A[:, 0:Z:2]
        gate = ((torch.arange(N) // 16) % 2 == 0)
        Wg = W[:, gate]
        Wg[:, :, 1:Z:2] = Wg[:, :, 0:Z:2]
        W[:, gate] = Wg
    full = grouped64(A, W, offs)
    mx = float(full[~torch.isnan(full)].abs().max()) if R > tail else 0.0
    assert mx <= 256, f"|sum| = {mx} > 256: not exact in bf16"
    gmin = float(deinterleave(torch.nan_to_num(full))[0].min()) if R > tail else 0.0
    assert gmin >= -80, f"gate sum {gmin}: SiLU(g) u would leave the normal range"
    A[R - tail:] = float("nan")
    for e, s in enumerate(sizes):
        if s == 0:
            W[e] = float("nan")
    return A.to(torch.bfloat16), W.to(torch.bfloat16), torch.tensor(offs, dtype=torch.int32)


# pk_moe_gemm (N % 128 != 0): one case per M tile count, K of one and of three 128-deep steps
MOE_GEMM_CASES = tuple(GemmCase(tuple(s for s in (0, 1, 16, 17, mr) if s <= mr), 96, K, mr, seed=mr + K)
                       for mr in (16, 32, 48, 64) for K in (128, 384))
# gemm.grouped_linear: 64-row tiles and 128-row tiles; K = 256 S
SKINNY_CASES = tuple(GemmCase(sizes, N, 256 * S, mr, seed=N + S + mr)
                     for sizes, mr in (((0, 1, 15, 16, 17, 64), 64), ((65, 128, 0, 1), 128))
                     for N in (128, 256) for S in (1, 2, 4))
# gemm_prefill.grouped_linear: 256-row tiles; K = 64, 192 take the 8-wave kernel whatever the variant
PREFILL_CASES = tuple(GemmCase((255, 0, 256, 257, 1), 256, K, 257, tail=5, seed=K) for K in (64, 192, 128, 512))


def gemm_mutants(case: GemmCase, A, W, offs):
    """name -> float64 [R, N] projection of a mutated reference (full K)."""
    K = case.K
    return {"next_expert": grouped64(A, W, offs, next_expert=True),
            "drop_k": grouped64(A, W, offs, drop=(K // 2 + 3,)),
            "drop_vec8": grouped64(A, W, offs, drop=tuple(range(K - 16, K - 8)))}


def slab_refs(A, W, offs, S, shift=0):
    """Split-K slabs: slab s sums k in [s K/S, (s+1) K/S) (mutant ``shift``: inner boundaries moved)."""
    K = W.shape[2]
    kper = K // S
    cuts = [0] + [s * kper + shift for s in range(1, S)] + [K]
    return torch.stack([grouped64(A, W, offs, cuts[s], cuts[s + 1]) for s in range(S)])


def gather_case(T, k, E, e_lo, e_hi, N, K, seed):
    """Gathered-A grouped GEMM: token rows x [T, K] (NaN where no local slot reads the token),
    random routing ids [T, k] (distinct per token), W [E_local, N, K] with NaN experts that get no
    slot -> (x, W, ids, offsets, sorted, A_permuted with a NaN tail [T k, K])."""
    g = np.random.default_rng(seed)
    ids = np.stack([g.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    offsets, sorted_, _ = align_ref(ids, e_lo, e_hi)
    sizes = tuple(int(s) for s in np.diff(offsets))
    A, W, offs = int_operands(sizes, N, K, T * k - int(offsets[-1]), seed)
    m = int(offsets[-1])
    x = torch.full((T, K), float("nan"), dtype=torch.bfloat16)
    tok = torch.as_tensor(sorted_) // k
    # the permuted rows decide the token rows: a token read by two local slots gets the first's row
    first = {}
    for p in range(m):
        first.setdefault(int(tok[p]), p)
    for t, p in first.items():
        x[t] = A[p]
    A = torch.cat([x[tok], A[m:]])
    full = grouped64(A[:m], W, offs) if m else None
    assert full is None or float(torch.nan_to_num(full).abs().max()) <= 256
    return x, W, ids, offs, torch.as_tensor(sorted_, dtype=torch.int32), A


# ---------------------------------------------------------------------------------- end to end
def interleave(gate: torch.Tensor, up: torch.Tensor, block: int = 16) -> torch.Tensor:
    I, K = gate.shape
    return torch.stack([gate.reshape(I // block, block, K), up.reshape(I // block, block, K)], 1).reshape(2 * I, K)


@dataclasses.dataclass(frozen=True)
class MoeCase:
    name: str
    T: int
    H: int
    I: int
    E: int = 8
    k: int = 2

    def build(self, e_lo, e_hi):
        """x [T, H]: columns [0, E) carry grid logits (top two 1 to 1.5 apart), the rest integers;
        router one-hot so logit_e = x[:, e]; w13 (those columns zeroed) and w2 integers, for the local
        experts, NaN where no token is routed."""
        T, H, I, E, k = self.T, self.H, self.I, self.E, self.k
        g = torch.Generator().manual_seed(T + H + I)
        rng = np.random.default_rng(T + I)
        x = (torch.randint(0, 2, (T, H), generator=g) + 1.0) * (torch.randint(0, 2, (T, H), generator=g) * 2.0 - 1)
        for t in range(T):
            # descending grid values: the second 1 to 1.5 below the first (swapped slot weights differ
            # by e), the third within 0.5 of the second (the top two hold well under all the mass, so
            # leaving out the renormalisation shows), the rest 0.125 to 2 apart
            gaps = rng.integers(1, 17, size=E - 1) / 8
            gaps[0] = rng.integers(8, 13) / 8
            gaps[1] = rng.integers(1, 5) / 8
            v = rng.integers(0, 33) / 8 - np.concatenate([[0.0], np.cumsum(gaps)])
            # the largest goes to expert t % E and the second to (3 t + 7) % E (never the same), so
            # every expert range of EP_RANGES is used by some token and unused by another
            first, second = t % E, (3 * t + 7) % E
            rest = [e for e in rng.permutation(E) if e not in (first, second)]
            x[t, [first, second] + rest] = torch.from_numpy(v).float()
        router = torch.zeros(E, H)
        router[torch.arange(E), torch.arange(E)] = 1.0
        w13 = torch.randint(0, 2, (E, 2 * I, H), generator=g) * 2.0 - 1
        w13[:, :, :E] = 0
        w2 = torch.randint(0, 2, (E, H, I), generator=g) * 2.0 - 1
        ids, _ = route64(x[:, :E], k, True)
        used = set(ids.flatten().tolist())
        for e in range(E):
            if e not in used:
                w13[e] = float("nan")
                w2[e] = float("nan")
        b = torch.bfloat16
        return x.to(b), router.to(b), w13[e_lo:e_hi].contiguous().to(b), w2[e_lo:e_hi].contiguous().to(b)


MOE_CASES = (MoeCase("skinny", 5, 256, 256), MoeCase("tiles", 70, 256, 256), MoeCase("moe_gemm", 5, 256, 96))
EP_RANGES = ((0, 8), (2, 6), (7, 8))


def moe64(x, router, w13, w2, k, e_lo, e_hi, renorm=True, swap=False, next_expert=False, gate_up_swap=False,
          keep_nonlocal=False, shift=False):
    """Mixtral sparse MLP over the experts [e_lo, e_hi) in float64 -> (out [T, H],
    B = sum_j w_j sum_i |h_ji w2_ji| [T, H]).  The keyword mutants as in the stage references."""
    x64, T = x.double(), x.shape[0]
    E, El = router.shape[0], e_hi - e_lo
    ids, w = route64(x64 @ router.double().t(), k, renorm)
    if swap:
        w = w[:, [1, 0] + list(range(2, k))]
    out = torch.zeros(x.shape, dtype=torch.float64)
    B = torch.zeros(x.shape, dtype=torch.float64)
    for t in range(T):
        for j in range(k):
            e = int(ids[t, j])
            if not e_lo <= e < e_hi:
                if not keep_nonlocal:
                    continue
                e = min(max(e, e_lo), e_hi - 1)
            le = (e - e_lo + 1) % El if next_expert else e - e_lo
            g, u = deinterleave((w13[le].double() @ x64[t])[None])
            if gate_up_swap:
                g, u = u, g
            h = (silu64(g) * u)[0]
            w2e = w2[le].double()
            out[t] += w[t, j] * (w2e @ h)
            B[t] += w[t, j] * (w2e.abs() @ h.abs())
    if shift:
        out, B = out.roll(1, 0), B.roll(1, 0)
    return out, B


def check_moe(out, ref, B):
    """|out - moe64| <= 4.25 u B: two roundings in h, one in y, one in the output, 0.25 u of
    headroom.  A token without a local slot has B = 0 and must be exactly zero."""
    out = out.double()
    assert bool(torch.isfinite(out).all()), "non-finite output"
    err = (out - ref).abs()
    bound = 4.25 * U * B
    assert bool((err <= bound).all()), ("moe", float((err / (U * B).clamp_min(1e-300)).max()))
    return float((err / (U * B).clamp_min(1e-300)).max())
