"""Case builders, float64 references and criteria for the dense bf16 GEMM tests, shared by the CPU
tests (tests/unit/test_gemm_cases.py: the cases can fail -- they reject wrong references) and the
GPU tests (tests/kernels/test_gemm_exact.py: the kernels pass them).  No GPU is touched here.

The function under test is  acc[m, n] = sum_k x[m, k] * w[n, k]  (bf16 operands, fp32 sums) and the
epilogues the kernels document:

    bf16 out           bf16(acc)                                   one rounding
    slabs              fp32 sums over K / S consecutive columns    no rounding on grid inputs
    SiLU               bf16(bf16(silu(bf16(g))) * bf16(u))         gate / up interleaved in blocks of 16
    residual update    new = bf16(bf16(sum of slabs) + r);  parts[b, m] = sum of new[m, cols of b]^2
    NormIn prologue    x' = bf16(bf16(v * rinv[m]) * w_norm[k])    rinv = rsqrt(sum of parts / K + eps)
    RowScale           acc * rinv[m] ahead of the epilogue
    QKV + RoPE         q, k = bf16(neox rotation of bf16(acc));  v = bf16(acc);  k, v to the paged caches

Exact cases
-----------
Grid cases hold small integers, so every product and every partial sum is an integer whose
magnitude is bounded by sum_k |x| |w| < 2^24: exact in fp32 in ANY summation order, and a correct
kernel equals the float64 reference bit for bit after the documented roundings.  Every builder
asserts that budget in float64 (:func:`assert_budget`).  Two magnitude classes:

    "small"     x in {-1, 0, 1}, w in [-2, 2]: |acc| stays below 256 (bf16(acc) == acc) and the sums
                of squares of the updated residual stay integral and below 2^24: the parts are exact.
    "rounding"  x, w in [-4, 4], every fourth weight row aligned with the signs of row 0 of x:
                |acc| exceeds 256, so bf16(acc) actually rounds.  Only this class can tell
                bf16(bf16(acc) + r) from bf16(acc + r) (the builder asserts that the two differ).

Needle cases: everything is zero but one weight at (n*, k*) and one activation at (m*, k*).

Inexact steps and their derived bounds (u = 2^-24, the relative error of one fp32 rounding)
---------------------------------------------------------------------------------------------
rinv = rsqrtf(ss / K + eps).  The parts are integers whose sum stays below 2^24, so ss is exact.
  * NormIn cases give row m the single part K * 4^j(m), j = m % 4, and eps = 1e-5: rinv is 2^-j
    (1 - e) with 0 < e < 2^-17 plus a few fp32 ulp, far less than half a bf16 ulp (2^-9), so
    bf16(v * rinv) is exactly v * 2^-j for every bf16 v: the prologue is bit-exact, and the
    per-row exponents expose a row mix-up.  The builder asserts this with rinv perturbed by 2^-16.
  * RowScale cases use arbitrary integer parts and the INTERVAL criterion with
        DELTA_R = 5 u:
    the division ss / K (correctly rounded by default; 1 ulp = 2 u allowed) and the addition of eps
    (u) perturb the argument by 3 u, which rsqrt halves (1.5 u); rsqrtf itself is within 1 ulp = 2 u
    (ROCm HIP math API accuracy table); the product acc * rinv rounds once more (u): 4.5 u, and
    5 u covers the second-order terms.  fp32 slabs must lie within DELTA_R |ref|; a bf16 value
    derived from them must lie between the bf16 roundings of the interval's ends.  When S row-scaled
    slabs are summed by a reducer, the S - 1 fp32 additions of (no longer integral) slabs add
    (S - 1) u sum_s |slab_s|: :func:`rowscale_err`.

silu(x) = x / (1 + __expf(-x)).  __expf is exp2 of x * log2(e): the product's rounding and the
  rounded constant move the exponent by at most 1.5 |x| u relative in the result, the hardware
  exp2 is within 1 ulp (2 u): e has relative error (2 + 1.5 |x|) u, which 1 + e passes on with
  weight e / (1 + e) <= 1; the addition rounds (u) and the division is within 2.5 ulp (5 u) even
  when it is not the correctly rounded one:
        DELTA_S(x) = (8 + 2 |x|) u.
  Below x = -88.7 __expf overflows and the kernel returns -0 where |silu| <= 89 e^-88.7 < 2^-121:
  an absolute 2^-118 is added.  silu is not monotone, so the interval of bf16(g) is mapped through
  the range of silu over it.  Exact anchor: a gate that is exactly 0 gives exactly 0 (no slack).

Parts of the "rounding" class are sums of n non-negative fp32 terms (n squares, each rounded once,
n - 1 additions) in unknown order: |got - ref| <= n u ref.

RoPE is exact by construction: the tests supply a table whose (cos, sin) pairs are (1, 0), (0, 1),
(0, -1), (-1, 0), (1/2, 1/2), (1/2, -1/2), varying per position and per dimension: every product
is exact in fp32, FMA-contracted or not, and the one bf16 rounding is the reference's.

The interval criteria leave no element out.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

import torch

BF16 = torch.bfloat16
U = 2.0 ** -24
DELTA_R = 5 * U
SILU_ABS = 2.0 ** -118
EPS = 1e-5
POISON = -1000.0  # finite, bf16-exact, never produced by a case

MUTANTS = (
    "kblock_swap", "kstep_swap", "kchunk_swap", "tile16_swap", "half64_swap", "drop_last_split", "split_shift",
    "row_leak", "gate_up_swap", "gate_next_up", "round_once", "parts_old", "parts_next_row", "rinv_div_n",
    "rinv_next_row", "normw_shift8", "rope_halves_swapped", "sin_flip", "pos_next_row", "khead_next",
    "v_untransposed", "slot_neg_cached")

# the shapes of the GPU tests
SHAPES = [(128, 256), (256, 512), (384, 1024), (256, 2048)]
LONG_SHAPE = (128, 14336)
ROWS = [1, 15, 16, 17, 40, 64]
ROWS_TILED = [65, 128, 200]
NPARTS = [1, 3, 16, 20, 64]
QKV_HEADS = [(2, 1, 32), (4, 2, 64)]
PREFILL_M = [1, 255, 256, 257, 513]
PREFILL_N = [256, 512]
PREFILL_K = [64, 128, 192, 320, 1024]


def splits(K: int, cand=(1, 2, 4, 8)) -> List[int]:
    return [S for S in cand if K % (256 * S) == 0]


def bf(t: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value, as float64."""
    return t.double().float().to(BF16).double()


def is_bf16(t: torch.Tensor) -> bool:
    return bool((bf(t) == t.double()).all())


@dataclasses.dataclass
class Case:
    x: torch.Tensor  # [M, K] bf16
    w: torch.Tensor  # [N, K] bf16, row-major
    name: str = ""
    unit: float = 1.0  # every product is a multiple of this

    @property
    def M(self):
        return self.x.shape[0]

    @property
    def N(self):
        return self.w.shape[0]

    @property
    def K(self):
        return self.w.shape[1]


def assert_budget(c: Case) -> None:
    """Every product is a multiple of ``unit`` and sum_k |x| |w| < 2^24 units: every partial sum, in
    any order and over any subset of k, is exact in fp32."""
    x, w = c.x.double() / c.unit, c.w.double()
    assert bool((x == x.round()).all()) and bool((w == w.round()).all()), c.name
    assert float((x.abs() @ w.abs().t()).max()) < 2 ** 24, c.name


def _gen(*key) -> torch.Generator:
    s = 0
    for v in key:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def grid_case(N: int, K: int, M: int, seed: int = 0, cls: str = "rounding") -> Case:
    g = _gen(11, N, K, M, seed, len(cls))
    if cls == "small":
        x = torch.randint(-1, 2, (M, K), generator=g)
        w = torch.randint(-2, 3, (N, K), generator=g)
    else:
        x = torch.randint(-4, 5, (M, K), generator=g)
        w = torch.randint(-4, 5, (N, K), generator=g)
        sgn = torch.where(x[0] < 0, -1, 1)
        w[::4] = w[::4].abs() * sgn[None, :]  # acc[0, 4 i] = sum |x| |w|: well above 256
    c = Case(x.to(BF16), w.to(BF16), f"grid-{cls}-{N}x{K}-m{M}-s{seed}")
    assert_budget(c)
    acc = c.x.double() @ c.w.double().t()
    if cls == "small":
        assert float(acc.abs().max()) <= 256, c.name  # bf16(acc) == acc
    elif K >= 256:  # (the short-K prefill cases stay below 256)
        assert bool((bf(acc) != acc).any()), c.name   # bf16(acc) rounds
    return c


def silu_case(N: int, K: int, M: int, seed: int = 0, cls: str = "rounding") -> Case:
    """A grid case for interleaved gate / up rows whose gate rows 32..47 are zero: the exact anchor
    (output columns 16..31 must be exactly 0)."""
    c = grid_case(N, K, M, seed + 50, cls)
    c.w[32:48] = 0
    c.name = "silu-" + c.name
    return c


def needle_case(N: int, K: int, M: int, n: int, k: int, m: int, xv: float = 3.0, wv: float = -1.5) -> Case:
    x = torch.zeros((M, K), dtype=BF16)
    w = torch.zeros((N, K), dtype=BF16)
    x[m, k] = xv
    w[n, k] = wv
    return Case(x, w, f"needle-{N}x{K}-m{M}-n{n}-k{k}-row{m}", unit=0.5)


def _uniq(vals, hi) -> List[int]:
    return sorted({v for v in vals if 0 <= v < hi})


def decode_needle_points(N: int, K: int, M: int, S: int = 1) -> List[Tuple[int, int, int]]:
    """(n*, k*, m*): the product of the corners of the decode tiling -- first / last row of a 16-row
    tile, a 64-row half block and a 128-row n-block; edges of an 8-element fragment, a 32-deep
    k-block, a 128-deep k-step, a 256-deep chunk and the split; rows 0, 15, 16, M - 1."""
    ns = _uniq((0, 15, 16, 63, 64, 127, 128, N - 1), N)
    ks = _uniq((0, 7, 8, 31, 32, 127, 128, 255, 256, K // S - 1, K // S, K - 1), K)
    ms = _uniq((0, 15, 16, M - 1), M)
    return [(n, k, m) for n in ns for k in ks for m in ms]


def prefill_needle_points(M: int, N: int, K: int) -> List[Tuple[int, int, int]]:
    """(n*, k*, m*) over the edges of the 16-row MFMA block, the 64-deep k-tile and the 128 / 256-row
    wave / workgroup tile: every (m*, k*) pair with n* cycling, and every (n*, k*) pair with m* cycling."""
    ms = _uniq((0, 15, 16, 127, 128, 255, 256, M - 1), M)
    ns = _uniq((0, 15, 16, 127, 128, 255, 256, N - 1), N)
    ks = _uniq((0, 7, 8, 63, 64, 127, 128, K - 1), K)
    pts = {(ns[(i + j) % len(ns)], k, m) for i, m in enumerate(ms) for j, k in enumerate(ks)}
    pts |= {(n, k, ms[(i + j) % len(ms)]) for i, n in enumerate(ns) for j, k in enumerate(ks)}
    return sorted(pts)


# ------------------------------------------------------------------------------- GEMM references
def _swap(t: torch.Tensor, dim: int, a: int, b: int, n: int) -> torch.Tensor:
    if t.shape[dim] < max(a, b) + n:
        return t
    idx = torch.arange(t.shape[dim])
    idx[a:a + n], idx[b:b + n] = torch.arange(b, b + n), torch.arange(a, a + n)
    return t.index_select(dim, idx)


def _operands(c: Case, mutant: Optional[str]):
    x, w = c.x.double(), c.w.double()
    if mutant == "kblock_swap":     # two 32-deep k-blocks of the weight
        w = _swap(w, 1, 0, 32, 32)
    elif mutant == "kstep_swap":    # two 128-deep k-steps
        w = _swap(w, 1, 0, 128, 128)
    elif mutant == "kchunk_swap":   # two 256-deep chunks
        w = _swap(w, 1, 0, 256, 256)
    elif mutant == "tile16_swap":   # two 16-row tiles
        w = _swap(w, 0, 0, 16, 16)
    elif mutant == "half64_swap":   # the two 64-row halves of an n-block
        w = _swap(w, 0, 0, 64, 64)
    return x, w


def ref_slabs(c: Case, S: int = 1, mutant: Optional[str] = None, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [S, M, N]: slab s = the sum over columns [s K / S, (s + 1) K / S).  ``x``: float64
    activations in place of the case's (the output of a norm prologue)."""
    x0, w = _operands(c, mutant)
    x = x0 if x is None else x
    kper = c.K // S
    b = [i * kper for i in range(S + 1)]
    if mutant == "split_shift" and S > 1:  # the first split takes one 256-chunk of the second
        b[1] += 256
    out = torch.stack([x[:, b[i]:b[i + 1]] @ w[:, b[i]:b[i + 1]].t() for i in range(S)])
    if mutant == "drop_last_split" and S > 1:
        out[-1] = 0
    return out


def ref_acc(c: Case, S: int = 1, mutant: Optional[str] = None, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    return ref_slabs(c, S, mutant, x).sum(0)


def ref_bf16(c: Case, S: int = 1, mutant: Optional[str] = None) -> torch.Tensor:
    return bf(ref_acc(c, S, mutant))


def expect_buf(ref: torch.Tensor, pad_rows: int = 2, pad_cols: int = 8, mutant: Optional[str] = None) -> torch.Tensor:
    """``ref`` [M, N] inside a NaN buffer [M + pad_rows, N + pad_cols]: what a sentinel buffer holds
    after the kernel wrote its [M, N] view."""
    M, N = ref.shape
    buf = torch.full((M + pad_rows, N + pad_cols), float("nan"), dtype=torch.float64)
    buf[:M, :N] = ref
    if mutant == "row_leak":  # the rows that pad the last 16-row tile are copies of row M - 1
        buf[M, :N] = ref[M - 1]
    return buf


# ------------------------------------------------------------------------------------- intervals
def iv_abs(v: torch.Tensor, err) -> Tuple[torch.Tensor, torch.Tensor]:
    return v - err, v + err


def iv_bf(iv):
    return bf(iv[0]), bf(iv[1])


def iv_mul(a, b):
    p = torch.stack([a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]])
    return p.min(0).values, p.max(0).values


def silu64(x: torch.Tensor) -> torch.Tensor:
    return x / (1.0 + torch.exp(-x))


SILU_ARGMIN = -1.2784645427610738  # silu'(x) = 0


def iv_silu(g):
    """The values x / (1 + __expf(-x)) may take for x in [g.lo, g.hi]: the range of silu over the
    interval, widened by DELTA_S and the overflow floor -- except that silu(0) is exactly 0."""
    lo, hi = g
    a, b = silu64(lo), silu64(hi)
    smin, smax = torch.minimum(a, b), torch.maximum(a, b)
    inside = (lo < SILU_ARGMIN) & (hi > SILU_ARGMIN)
    smin = torch.where(inside, torch.full_like(smin, float(silu64(torch.tensor(SILU_ARGMIN, dtype=torch.float64)))), smin)
    mag = torch.maximum(lo.abs(), hi.abs())
    d = (8.0 + 2.0 * mag) * U
    zero = (lo == 0) & (hi == 0)
    slack = torch.where(zero, torch.zeros_like(mag), torch.full_like(mag, SILU_ABS))
    return smin - d * smin.abs() - slack, smax + d * smax.abs() + slack


def split_gate_up(y: torch.Tensor):
    """[M, 2I] interleaved in blocks of 16 -> gate [M, I], up [M, I]."""
    v = y.reshape(y.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(y.shape[0], -1), v[:, :, 1].reshape(y.shape[0], -1)


def ref_silu(acc: torch.Tensor, err=0.0, mutant: Optional[str] = None):
    """(lo, hi), float64 [M, N / 2] of bf16 values: the interval of
    bf16(bf16(silu(bf16(g))) * bf16(u)) for the interleaved pre-activations ``acc`` [M, N] known to
    within ``err`` (absolute; 0 for the exact grid cases)."""
    g, u = split_gate_up(acc)
    eg, eu = (split_gate_up(err) if isinstance(err, torch.Tensor) else (err, err))
    if mutant == "gate_up_swap":
        g, u, eg, eu = u, g, eu, eg
    elif mutant == "gate_next_up":  # the gate of block b with the up of block b + 1
        u = torch.roll(u, -16, 1)
        eu = torch.roll(eu, -16, 1) if isinstance(eu, torch.Tensor) else eu
    gi, ui = iv_bf(iv_abs(g, eg)), iv_bf(iv_abs(u, eu))
    return iv_bf(iv_mul(iv_bf(iv_silu(gi)), ui))


def inside(got: torch.Tensor, iv) -> bool:
    """Every element within [lo, hi]; NaN exactly where the interval is NaN."""
    got = got.double().cpu()
    lo, hi = iv
    ok = ((got >= lo) & (got <= hi)) | (got.isnan() & lo.isnan() & hi.isnan())
    return got.shape == lo.shape and bool(ok.all())


def disjoint(a, b) -> bool:
    """Some element at which no value satisfies both intervals (a kernel with a's bug fails b)."""
    return bool(((a[1] < b[0]) | (a[0] > b[1])).any())


def iv_pad(iv, pad_rows: int = 2, pad_cols: int = 8, mutant: Optional[str] = None):
    return expect_buf(iv[0], pad_rows, pad_cols, mutant), expect_buf(iv[1], pad_rows, pad_cols, mutant)


def within_rel(got: torch.Tensor, ref: torch.Tensor, err) -> bool:
    """|got - ref| <= err at every element (err: a tensor of absolute bounds)."""
    got = got.double().cpu()
    return got.shape == ref.shape and bool(((got - ref).abs() <= err).all())


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, err: torch.Tensor) -> float:
    """max |got - ref| / err over the elements with err > 0 (recorded, never used as a bound)."""
    got = got.double().cpu()
    m = err > 0
    return float(((got - ref).abs()[m] / err[m]).max()) if bool(m.any()) else 0.0


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as values, NaN positions included (-0.0 == 0.0: the sign of a zero sum is not part of
    the contract)."""
    a, b = a.double().cpu(), b.double().cpu()
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------- residual update
def residual_case(N: int, K: int, M: int, seed: int = 0, cls: str = "small", nblk: int = 128):
    """(case, r_old float64 [M, N] of integers in [-8, 8]) for residual += x @ w^T."""
    c = grid_case(N, K, M, seed + 100, cls)
    r = torch.randint(-8, 9, (M, N), generator=_gen(13, N, K, M, seed)).double()
    acc = ref_acc(c)
    new, parts = ref_add_residual(acc, r, nblk)
    if cls == "small":  # exact parts
        assert float(parts.max()) < 2 ** 24, c.name
    else:               # the two rounding orders differ somewhere
        assert bool((bf(acc + r) != new).any()), c.name
    return c, r


def ref_add_residual(acc: torch.Tensor, r_old: torch.Tensor, nblk: int, mutant: Optional[str] = None):
    """(new residual float64 [M, N], parts float64 [N / nblk, M]) of
    new = bf16(bf16(acc) + r_old), parts[b, m] = sum of new[m, b nblk : (b + 1) nblk]^2."""
    M, N = acc.shape
    new = bf(acc + r_old) if mutant == "round_once" else bf(bf(acc) + r_old)
    src = r_old if mutant == "parts_old" else new
    parts = src.view(M, N // nblk, nblk).pow(2).sum(-1).t().contiguous()
    if mutant == "parts_next_row":
        parts = torch.roll(parts, -1, 1)
    return new, parts


def parts_err(parts: torch.Tensor, nblk: int, cls: str) -> torch.Tensor:
    """Absolute bound on the parts: exact while they stay below 2^24 ("small"), else n u ref."""
    if cls == "small":
        return torch.zeros_like(parts)
    return nblk * U * parts


# ---------------------------------------------------------------------------- rinv, norm prologue
def pow2_parts(M: int, nparts: int, K: int) -> torch.Tensor:
    """fp32 [nparts, M]: row m has the single part K 4^(m % 4), in part m % nparts."""
    p = torch.zeros((nparts, M), dtype=torch.float32)
    m = torch.arange(M)
    p[m % nparts, m] = (K * 4.0 ** (m % 4)).float()
    return p


def int_parts(M: int, nparts: int, seed: int = 0) -> torch.Tensor:
    """fp32 [nparts, M] of integers in [1, 4000]: any sum of them is exact."""
    return torch.randint(1, 4001, (nparts, M), generator=_gen(17, M, nparts, seed)).float()


def ref_rinv(parts: torch.Tensor, K: int, eps: float = EPS, mutant: Optional[str] = None, N: int = 0) -> torch.Tensor:
    """float64 [M]: 1 / sqrt(sum of parts / K + eps), eps as the fp32 value the kernel receives."""
    ss = parts.double().sum(0)
    assert float(ss.max()) < 2 ** 24
    e = float(torch.tensor(eps, dtype=torch.float32))
    r = 1.0 / torch.sqrt(ss / (N if mutant == "rinv_div_n" else K) + e)
    return torch.roll(r, -1) if mutant == "rinv_next_row" else r


def ref_norm_in(res: torch.Tensor, rinv: torch.Tensor, nw: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [M, K]: bf16(bf16(v * rinv[m]) * w_norm[k])."""
    nw = nw.double()
    if mutant == "normw_shift8":
        nw = torch.roll(nw, -8)
    return bf(bf(res.double() * rinv[:, None]) * nw[None, :])


def norm_case(N: int, K: int, M: int, seed: int = 0, nparts: int = 1):
    """(case, norm weight bf16 [K], parts fp32 [nparts, M]): the case's x is the residual stream
    (integers in [-8, 8]), its parts make rinv a power of two, the norm weight holds integers in
    [-3, 3] without 0; the normalised activations are multiples of 1/8 of magnitude <= 24."""
    g = _gen(19, N, K, M, seed)
    res = torch.randint(-8, 9, (M, K), generator=g)
    w = torch.randint(-2, 3, (N, K), generator=g)
    nw = torch.randint(1, 4, (K,), generator=g) * (2 * torch.randint(0, 2, (K,), generator=g) - 1)
    parts = pow2_parts(M, nparts, K)
    c = Case(res.to(BF16), w.to(BF16), f"norm-{N}x{K}-m{M}-p{nparts}-s{seed}")
    rinv = ref_rinv(parts, K)
    want = res.double() * (2.0 ** -(torch.arange(M) % 4).double())[:, None]
    for pert in (1.0 - 2.0 ** -16, 1.0, 1.0 + 2.0 ** -16):  # far more than the fp32 error of rinv
        assert bool((bf(res.double() * (rinv * pert)[:, None]) == want).all()), c.name
    xn = ref_norm_in(res, rinv, nw)
    assert is_bf16(want * nw.double()[None, :])
    assert_budget(Case(xn.to(BF16), c.w, c.name, unit=0.125))
    return c, nw.to(BF16), parts


def rowscale_err(slabs: torch.Tensor, rinv: torch.Tensor) -> torch.Tensor:
    """Absolute bound [M, N] on the sum of the S row-scaled fp32 slabs ``slabs * rinv``: DELTA_R per
    slab plus the S - 1 additions of the reducer, both relative to sum_s |slab_s|."""
    S = slabs.shape[0]
    return (DELTA_R + (S - 1) * U) * (slabs.abs().sum(0) * rinv[:, None])


# ------------------------------------------------------------------------------ QKV, RoPE, caches
ROPE_PAIRS = [(1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0), (0.5, 0.5), (0.5, -0.5)]
ROPE_POS = 512


def rope_table(P: int = ROPE_POS) -> torch.Tensor:
    """fp32 [P, 128] = cos[64] | sin[64]; the pair of (position p, dimension d) varies with both."""
    p = torch.arange(P).view(P, 1)
    d = torch.arange(64).view(1, 64)
    idx = (5 * p + 3 * d + (p * d) % 7) % 6
    pairs = torch.tensor(ROPE_PAIRS)
    return torch.cat([pairs[idx, 0], pairs[idx, 1]], dim=1).float().contiguous()


def rope_positions(M: int) -> torch.Tensor:
    """Distinct per row."""
    return ((37 * torch.arange(M) + 5) % ROPE_POS).to(torch.int32)


def cache_slots(M: int, bs: int):
    """(slots int32 [M], number of blocks): consecutive from the last slot of block 0, so they cross
    a block boundary at once; row M // 2 is not cached (slot -1) when M > 1; slot 0 stays unused."""
    slots = (bs - 1 + torch.arange(M)).to(torch.int32)
    if M > 1:
        slots[M // 2] = -1
    return slots, (bs - 1 + M) // bs + 2


def qkv_case(nq: int, nkv: int, K: int, M: int, seed: int = 0) -> Case:
    """A "small" grid case with N = (nq + 2 nkv) * 128."""
    return grid_case((nq + 2 * nkv) * 128, K, M, seed + 200, "small")


def ref_rope(v: torch.Tensor, pos: torch.Tensor, cs: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """Neox rotation of float64 [M, H, 128] -> bf16 values (float64)."""
    pos = pos.long()
    if mutant == "pos_next_row":
        pos = torch.roll(pos, -1)
    t = cs.double()[pos]
    co, si = t[:, None, :64], t[:, None, 64:]
    if mutant == "sin_flip":
        si = -si
    a, b = v[..., :64], v[..., 64:]
    if mutant == "rope_halves_swapped":
        a, b = b, a
    return bf(torch.cat([a * co - b * si, b * co + a * si], dim=-1))


def ref_qkv(acc: torch.Tensor, pos, cs, slots, nq: int, nkv: int, bs: int, nblocks: int,
            kc0: Optional[torch.Tensor] = None, vc0: Optional[torch.Tensor] = None, mutant: Optional[str] = None):
    """(q float64 [M, nq, 128], K cache, V cache as logical float64 [nblocks, nkv, bs, 128]) of the
    QKV epilogue on the pre-activations ``acc`` [M, (nq + 2 nkv) * 128]; the caches start from
    ``kc0`` / ``vc0`` (logical) or from POISON."""
    M = acc.shape[0]
    h = acc.view(M, nq + 2 * nkv, 128)
    qk = ref_rope(bf(h[:, :nq + nkv]), pos, cs, mutant)
    q, k, v = qk[:, :nq], qk[:, nq:], bf(h[:, nq + nkv:])
    if mutant == "khead_next":
        k = torch.roll(k, 1, 1)
    kc = torch.full((nblocks, nkv, bs, 128), POISON, dtype=torch.float64) if kc0 is None else kc0.double().clone()
    vc = torch.full((nblocks, nkv, bs, 128), POISON, dtype=torch.float64) if vc0 is None else vc0.double().clone()
    if mutant == "v_untransposed":
        from polykey_service_amd.ops import reference
        vidx = reference.vcache_index(bs).view(-1)
        inv = torch.empty_like(vidx)
        inv[vidx] = torch.arange(vidx.numel())
        vphys = vc.view(nblocks, nkv, bs * 128)[:, :, inv]  # physical order of the logical start
    for m in range(M):
        s = int(slots[m])
        if s < 0:
            if mutant != "slot_neg_cached":
                continue
            s = 0
        kc[s // bs, :, s % bs] = k[m]
        if mutant == "v_untransposed":  # token-major rows where the layout wants 8-key runs
            vphys[s // bs, :, (s % bs) * 128:(s % bs + 1) * 128] = v[m]
        else:
            vc[s // bs, :, s % bs] = v[m]
    if mutant == "v_untransposed":
        vc = vphys[:, :, vidx].view(nblocks, nkv, bs, 128)
    return q, kc, vc


# --------------------------------------------------------------------- synthetic slabs (consumers)
def int_slabs(S: int, M: int, N: int, seed: int = 0, mag: int = 8) -> torch.Tensor:
    """fp32 [S, M, N] of integers in [-mag, mag]: any sum of them is exact."""
    return torch.randint(-mag, mag + 1, (S, M, N), generator=_gen(23, S, M, N, seed, mag)).float()


def addnorm_case(M: int, H: int, S: int, seed: int = 0):
    """(slabs fp32 [S, M, H], r_old bf16, norm weight bf16, new residual float64, x float64) for
    residual = bf16(bf16(sum of slabs) + r_old); x = bf16(bf16(residual * rinv) * w) with rinv from
    the row's OWN sum of squares: every 8 columns of new row m hold a permutation of
    2^j {2, 1, 1, 1, 1, 0, 0, 0} with random signs, j = m % 4, so the sum of squares is H 4^j
    exactly and rinv is a power of two as in :func:`norm_case`."""
    g = _gen(29, M, H, S, seed)
    slabs = int_slabs(S, M, H, seed)
    pat = torch.tensor([2, 1, 1, 1, 1, 0, 0, 0])
    perm = torch.rand((M, H // 8, 8), generator=g).argsort(-1)
    sign = 2 * torch.randint(0, 2, (M, H // 8, 8), generator=g) - 1
    new = (pat[perm] * sign).view(M, H).double() * (2.0 ** (torch.arange(M) % 4).double())[:, None]
    p = slabs.double().sum(0)
    r = new - p
    assert is_bf16(p) and is_bf16(r) and bool((bf(bf(p) + r) == new).all())
    assert bool((new.pow(2).sum(-1) == H * 4.0 ** (torch.arange(M) % 4).double()).all())
    nw = (torch.randint(1, 4, (H,), generator=g) * (2 * torch.randint(0, 2, (H,), generator=g) - 1)).double()
    rinv = 1.0 / torch.sqrt(new.pow(2).sum(-1) / H + float(torch.tensor(EPS, dtype=torch.float32)))
    x = ref_norm_in(new, rinv, nw)
    for pert in (1.0 - 2.0 ** -16, 1.0 + 2.0 ** -16):
        assert bool((ref_norm_in(new, rinv * pert, nw) == x).all())
    return slabs, r.to(BF16), nw.to(BF16), new, x


# -------------------------------------------------------------------------------------- sentinels
def sentinel_rows(x: torch.Tensor, extra: int = 3, pad_cols: int = 8) -> torch.Tensor:
    """``x`` [M, K] as a view into a NaN buffer [M + extra, K + pad_cols]: the rows at and beyond M
    are NaN and the row stride is above K (a multiple of 8)."""
    buf = torch.full((x.shape[0] + extra, x.shape[1] + pad_cols), float("nan"), dtype=x.dtype, device=x.device)
    buf[: x.shape[0], : x.shape[1]] = x
    return buf[: x.shape[0], : x.shape[1]]


def sentinel_out(M: int, N: int, device, dtype=BF16, pad_rows: int = 2, pad_cols: int = 8):
    """(NaN buffer [M + pad_rows, N + pad_cols], its [M, N] view the kernel writes)."""
    buf = torch.full((M + pad_rows, N + pad_cols), float("nan"), dtype=dtype, device=device)
    return buf, buf[:M, :N]


def sentinel_flat(n: int, device, tail: int = 64, dtype=torch.float32) -> torch.Tensor:
    """A NaN workspace of n + tail elements (the tail must stay NaN)."""
    return torch.full((n + tail,), float("nan"), dtype=dtype, device=device)


# ------------------------------------------------------------------------------- fused MLP anchor
def select_down(N: int, I: int, S: int):
    """(w bf16 [N, I], k int64 [S, N], v float64 [S, N]): a down weight with ONE non-zero per
    (output column n, split s), +-1 or +-2 at k[s, n] inside split s, so that slab
    [s, m, n] = v[s, n] * h[m, k[s, n]] exactly, whatever the summation order."""
    kper = I // S
    n = torch.arange(N).view(1, N)
    s = torch.arange(S).view(S, 1)
    k = s * kper + (n * 37 + s * 5) % kper
    v = (1.0 + (n + s) % 2) * (1.0 - 2.0 * ((n // 2 + s) % 2))
    w = torch.zeros((N, I), dtype=torch.float64)
    w[n.expand(S, N).reshape(-1), k.reshape(-1)] = v.double().reshape(-1)
    return w.to(BF16), k, v.double()
