"""Case builders and the float64 reference for the multi-LoRA shrink / expand tests, shared by the
CPU tests (tests/unit/test_lora_cases.py: the cases can fail -- they reject wrong references) and
the GPU tests (tests/kernels/test_lora.py: the kernels pass them).

The function under test, per row m with slot = idx[m] >= 0 (a row with idx = -1 is neither read
nor written):

    t[m, j]    = bf16( rinv[m] * sum_k x[m, k] * A[slot][j, k] )            one rounding
    delta[m,n] = s[slot] * sum_j B[slot][n, j] * t[m, seg(n) * seg_r + j]   s applied last
    slab form:  slab0[m, n] += delta       bf16 form:  out[m, n] = bf16(float(out[m, n]) + delta)

rinv[m] = 1 / sqrt(sum_p parts[p, m] / K + eps) in correctly rounded fp32 operations (or 1).

Grid cases are exact.  x holds integers in [-2, 2]; every row of every A holds at most eight
non-zeros from {+-1, +-2} at positions of its own, so |sum_k| <= 32: an integer that bf16 holds,
exact in fp32 in ANY summation order.  B holds values from {0, +-0.5, +-1, +-2}, the scales are
powers of two, the buffers start as small integers; every partial sum of the expand is a multiple
of 2^-8 far below 2^24 such units.  A correct kernel therefore equals the float64 reference bit for
bit.  With a row scale, rinv is one of {1, 2, 1.5, 1.25} and one entry of every A row is +-129, so
the (still exact) sums reach +-286 and need more bits than bf16 holds: the product rinv * sum is
ONE fp32 multiplication of exact operands, which the reference performs in fp32 too, and t is its
bf16 rounding -- so these cases (and only these) tell a t rounded before the row scale, or never
rounded, from the contract.

Rows cycle through the slots (-1, 0, 2, 1), so no 16-row tile (nor any 8-row tile) is uniform; the
x rows of -1 rows are NaN, and so is every byte of padding around the operands.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

import torch

BF16 = torch.bfloat16
SEG_R = 64          # padded rank per sub-projection (max_lora_rank)
SLOTS = 3
ROW_SLOTS = (-1, 0, 2, 1)
SCALES = (0.5, 2.0, 0.25)
KS = (512, 2048)
RANKS = (1, 8, 16, 24)
ROWS = (1, 3, 16, 17, 64, 65)
# kind -> (N, b0, b1, il): tiny-llama's fused qkv (512 | 128 | 128), an interleaved gate_up, one block
KINDS = {"qkv": (768, 512, 640, 0), "gate_up": (2048, 2048, 2048, 16), "single": (768, 768, 768, 0)}
MUTANTS = ("index_ignored", "neg_as_slot0", "scale_dropped", "q_for_k", "gate_up_swapped", "deinterleave_wrong",
           "t_not_rounded", "round_before_scale", "rowscale_skipped", "last_rank_dropped", "overwrite", "slab1")


@dataclasses.dataclass
class Case:
    x: torch.Tensor            # [M, K] bf16, a strided view (row stride K + 8)
    A: torch.Tensor            # [SLOTS, R, K] bf16, R = segments * seg_r, zero past each slot's rank
    B: torch.Tensor            # [SLOTS, N, seg_r] bf16, rows in the fused order of the weight
    scale: torch.Tensor        # [SLOTS] fp32
    ranks: torch.Tensor        # [SLOTS] int32
    idx: torch.Tensor          # [M] int32
    seg: Tuple[int, int, int]  # b0, b1, il
    seg_r: int
    parts: Optional[torch.Tensor] = None   # [nparts, M] fp32 or None
    eps: float = 0.0
    name: str = ""

    @property
    def M(self):
        return self.x.shape[0]

    @property
    def K(self):
        return self.x.shape[1]

    @property
    def N(self):
        return self.B.shape[1]

    @property
    def R(self):
        return self.A.shape[1]

    @property
    def nseg(self):
        return self.R // self.seg_r


def col_segments(N: int, seg: Tuple[int, int, int]) -> torch.Tensor:
    b0, b1, il = seg
    n = torch.arange(N)
    return ((n // il) % 2) if il > 0 else (n >= b0).long() + (n >= b1).long()


def slot_ranks(r: int) -> Tuple[int, int, int]:
    """Ranks of the three slots of a case of nominal rank ``r``: r, the full padded rank, about half."""
    return (r, SEG_R, max(1, r // 2))


def row_indices(M: int) -> torch.Tensor:
    return torch.tensor([ROW_SLOTS[m % 4] for m in range(M)], dtype=torch.int32)


def _strided(v: torch.Tensor) -> torch.Tensor:
    """``v`` [M, K] as a view with row stride K + 8 into a NaN-filled buffer."""
    M, K = v.shape
    buf = torch.full((M, K + 8), float("nan"), dtype=v.dtype)
    buf[:, :K] = v
    return buf[:, :K]


def _parts_for(M: int, K: int, nparts: int = 3) -> torch.Tensor:
    """Sum-of-squares parts whose rows give rinv = 1, 2, ~1.5, ~1.25 in turn: mean = 1, 1/4,
    fl(4/9), fl(16/25) exactly (the mean times K, a power of two, split over the parts as
    1/2 + 1/4 + 1/4: every partial sum is exact)."""
    means = torch.tensor([1.0, 0.25, 4.0 / 9.0, 0.64], dtype=torch.float32)
    tot = means[torch.arange(M) % 4] * K
    w = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float32)[:nparts]
    return (w[:, None] * tot[None, :]).contiguous()


def grid_case(kind: str, K: int, r: int, M: int, rowscale: bool = False, seed: int = 0) -> Case:
    N, b0, b1, il = KINDS[kind]
    seg = (b0, b1, il)
    nseg = int(col_segments(N, seg).max()) + 1
    R = nseg * SEG_R
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 104729 * r + 31 * M + len(kind))
    idx = row_indices(M)
    x = torch.randint(-2, 3, (M, K), generator=g).float()
    x[idx < 0] = float("nan")
    ranks = slot_ranks(r)
    A = torch.zeros((SLOTS, R, K))
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0])
    for s in range(SLOTS):
        for sg in range(nseg):
            for j in range(ranks[s]):
                pos = torch.randperm(K, generator=g)[:8]
                if j == ranks[s] - 1:
                    pos[0], pos[1] = 0, K - 1  # the first and the last k column, in the last rank row
                    pos = torch.unique(pos)
                A[s, sg * SEG_R + j, pos] = vals[torch.randint(0, 4, (pos.numel(),), generator=g)]
                if rowscale:  # one large odd entry: the sum needs more bits than bf16 holds
                    A[s, sg * SEG_R + j, pos[-1]] = 129.0 if j % 2 else -129.0
    bvals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    B = bvals[torch.randint(0, 7, (SLOTS, N, SEG_R), generator=g)]
    for s in range(SLOTS):
        B[s, :, ranks[s]:] = 0.0
        B[s, :, ranks[s] - 1] = bvals[1 + (torch.arange(N) + s) % 6]  # the last rank column is never zero
    return Case(_strided(x.to(BF16)), A.to(BF16), B.to(BF16), torch.tensor(SCALES, dtype=torch.float32),
                torch.tensor(ranks, dtype=torch.int32), idx, seg, SEG_R,
                _parts_for(M, K) if rowscale else None, 0.0, f"{kind}-K{K}-r{r}-M{M}{'-rs' if rowscale else ''}")


def grid_cases(kind: str, K: int, r: int) -> List[Case]:
    """Every row count of one (kind, K, rank); the row scale on every other one."""
    return [grid_case(kind, K, r, M, rowscale=bool(i % 2)) for i, M in enumerate(ROWS)]


def random_case(kind: str, K: int, N: int, ranks: Tuple[int, int, int], M: int, seed: int = 0) -> Case:
    """Gaussian operands (bf16) on the shape family of ``kind`` scaled to N columns; no row scale."""
    N0, b0, b1, il = KINDS[kind]
    seg = (b0 * N // N0, b1 * N // N0, il)
    nseg = int(col_segments(N, seg).max()) + 1
    g = torch.Generator().manual_seed(77 * seed + K + N + sum(ranks) + M)
    idx = row_indices(M)
    x = torch.randn((M, K), generator=g)
    x[idx < 0] = float("nan")
    A = torch.randn((SLOTS, nseg * SEG_R, K), generator=g) * K ** -0.5
    B = torch.randn((SLOTS, N, SEG_R), generator=g) * 0.5
    for s in range(SLOTS):
        B[s, :, ranks[s]:] = 0.0
        for sg in range(nseg):
            A[s, sg * SEG_R + ranks[s]:(sg + 1) * SEG_R] = 0.0
    return Case(_strided(x.to(BF16)), A.to(BF16), B.to(BF16), torch.tensor([1.0, 0.37, 2.5], dtype=torch.float32),
                torch.tensor(ranks, dtype=torch.int32), idx, seg, SEG_R, None, 0.0,
                f"rand-{kind}-K{K}-N{N}-r{ranks[0]}-M{M}")


def initial_out(c: Case, form: str, seed: int = 0) -> torch.Tensor:
    """The buffer the expand adds into: two fp32 slabs [2, M, N] (slab form) or bf16 [M, N]."""
    g = torch.Generator().manual_seed(5 + seed + c.M + c.N)
    if form == "slab":
        return torch.randint(-8, 9, (2, c.M, c.N), generator=g).float()
    return torch.randint(-8, 9, (c.M, c.N), generator=g).to(BF16)


def rinv_fp32(c: Case) -> Optional[torch.Tensor]:
    """rinv of every row in fp32: 1 / sqrt(sum(parts) / K + eps), each operation correctly rounded."""
    if c.parts is None:
        return None
    ss = c.parts.double().sum(0).float()  # exact by construction (grid) / within the bound's slack (random)
    return 1.0 / torch.sqrt(ss / float(c.K) + torch.tensor(c.eps, dtype=torch.float32))


def sums_f64(c: Case, idx: torch.Tensor) -> torch.Tensor:
    """sum_k x[m, k] * A[idx[m]][j, k] in float64, [M, R]; rows without a slot are NaN."""
    out = torch.full((c.M, c.R), float("nan"), dtype=torch.float64)
    for m in range(c.M):
        s = int(idx[m])
        if s >= 0:
            out[m] = c.A[s].double() @ c.x[m].double()
    return out


def reference_t(c: Case, mutant: Optional[str] = None) -> torch.Tensor:
    """t [M, R] as float64 (bf16 values unless a mutant says otherwise); NaN rows = not written."""
    idx = c.idx.clone()
    if mutant == "index_ignored":
        idx[:] = 0
    elif mutant == "neg_as_slot0":
        idx[idx < 0] = 0
    sig = sums_f64(c, idx)
    rinv = rinv_fp32(c)
    if mutant == "round_before_scale":
        sig = sig.float().to(BF16).double()
    # one fp32 multiplication of the (exact) sum by rinv (NaN rows stay NaN), then the one rounding
    if c.parts is None or mutant == "rowscale_skipped":
        prod = sig
    else:
        prod = (sig.float() * rinv[:, None]).double()
    t = prod if mutant == "t_not_rounded" else prod.float().to(BF16).double()
    if mutant == "last_rank_dropped":
        for m in range(c.M):
            s = int(idx[m])
            if s >= 0:
                for sg in range(c.nseg):
                    t[m, sg * c.seg_r + int(c.ranks[s]) - 1] = 0.0
    return t


def reference_out(c: Case, form: str, init: torch.Tensor, mutant: Optional[str] = None,
                  t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The buffer after shrink + expand (``t``: a given t [M, R] instead of the reference's)."""
    idx = c.idx.clone()
    if mutant == "index_ignored":
        idx[:] = 0
    elif mutant == "neg_as_slot0":
        idx[idx < 0] = 0
    if t is None:
        t = reference_t(c, mutant)
    seg = col_segments(c.N, c.seg)
    if mutant == "q_for_k":
        seg = torch.where(seg == 1, torch.zeros_like(seg), seg)
    elif mutant == "gate_up_swapped" and c.seg[2] > 0:
        seg = 1 - seg
    elif mutant == "deinterleave_wrong" and c.seg[2] > 0:
        seg = (torch.arange(c.N) >= c.N // 2).long()
    cols = seg[:, None] * c.seg_r + torch.arange(c.seg_r)[None, :]
    out = init.clone()
    for m in range(c.M):
        s = int(idx[m])
        if s < 0:
            continue
        scale = 1.0 if mutant == "scale_dropped" else float(c.scale[s])
        delta = scale * (c.B[s].double() * t[m].double()[cols]).sum(-1)
        if form == "slab":
            k = 1 if mutant == "slab1" else 0
            out[k, m] = (delta if mutant == "overwrite" else out[k, m].double() + delta).float()
        else:
            out[m] = (delta if mutant == "overwrite" else out[m].double() + delta).float().to(BF16)
    return out


def true_out(c: Case, form: str, init: torch.Tensor) -> torch.Tensor:
    """float64 [M, N]: init + s * B (A x) with NO intermediate rounding (rows without a slot: init)."""
    seg = col_segments(c.N, c.seg)
    cols = seg[:, None] * c.seg_r + torch.arange(c.seg_r)[None, :]
    sig = sums_f64(c, c.idx)
    out = (init[0] if form == "slab" else init).double().clone()
    for m in range(c.M):
        s = int(c.idx[m])
        if s >= 0:
            out[m] += float(c.scale[s]) * (c.B[s].double() * sig[m][cols]).sum(-1)
    return out


def error_bound(c: Case, form: str, init: torch.Tensor) -> torch.Tensor:
    """Per element [M, N], against :func:`true_out`, for cases without a row scale:

        |err| <= s sum_j |B[n,j]| (2^-9 |t_j| + K 2^-24 sum_k |x_k A_jk|) + r 2^-24 s sum_j |B[n,j] t_j|

    (the rounding of t to bf16, the shrink's fp32 sums in any order, the expand's fp32 sums), plus
    half a bf16 ulp of the result -- 2^-9 of the binade's upper end -- in the bf16 form.  Rows
    without a slot: 0."""
    t = reference_t(c)
    seg = col_segments(c.N, c.seg)
    cols = seg[:, None] * c.seg_r + torch.arange(c.seg_r)[None, :]
    out = torch.zeros((c.M, c.N), dtype=torch.float64)
    for m in range(c.M):
        s = int(c.idx[m])
        if s < 0:
            continue
        absum = c.A[s].double().abs() @ c.x[m].double().abs()  # [R]
        tj = 2.0 ** -9 * t[m].abs() + c.K * 2.0 ** -24 * absum
        Bs = c.B[s].double().abs()
        sc = abs(float(c.scale[s]))
        out[m] = sc * (Bs * tj[cols]).sum(-1) + int(c.ranks[s]) * 2.0 ** -24 * sc * (Bs * t[m].abs()[cols]).sum(-1)
    if form == "bf16":
        res = true_out(c, form, init).abs()
        half_ulp = torch.pow(2.0, torch.floor(torch.log2(res.clamp_min(1e-30))) - 8)
        out += torch.where(out > 0, half_ulp, torch.zeros_like(half_ulp))
    return out
