"""Case builders and the float64 reference for the weight-only MXFP4 (W4) GEMM tests, shared by the
CPU tests (tests/unit/test_gemm_w4_cases.py: the cases can fail -- they reject wrong references)
and the GPU tests (tests/kernels/test_gemm_w4.py: the kernels pass them).

The function under test:  y[m, n] = sum_k x[m, k] * E2M1[nib[n, k]] * 2^(X[n, k // 32] - 127)  [* rinv[m]],
then the mode's epilogue: one bf16 rounding ("bf16"), fp32 slabs per k-split ("partial"), or
bf16(bf16(silu(bf16(gate))) * bf16(up)) of the interleaved gate / up columns ("silu").

Grid cases are exact: activations are integers in [-4, 4], nibbles are all 16 codes, and the scale
bytes X[n, kb] span ``nscales`` consecutive values from ``X0``.  Every product is then a multiple of
the quantum 0.5 * 2^(X0 - 127), and |sum_k |x| |w|| <= K * 4 * 6 * 2^(X0 + nscales - 1 - 127), i.e.
at most 48 K 2^(nscales - 1) quanta: below 2^24 for nscales = 8 at K <= 1024 (2^22.6) and for
nscales = 4 at K = 14336 (2^22.4).  :func:`grid_case` computes ``max |sum| / quantum`` from the data
and asserts it is below 2^24, so every partial sum is exact in fp32 in ANY summation order and a
correct kernel equals the float64 reference bit for bit after the one final rounding.

Every-code case: all 16 nibbles x every scale byte in [2, 252], probed with one-hot activations.
Position-coded case: X[n, kb] takes 16 distinct values as a function of (n, kb) that changes with
the next row, the next 16-row tile, the next k-block and the next k-step, probed with one-hot
activations at the layout's edges.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import torch

BF16 = torch.bfloat16
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
MUTANTS = ("nibble_swap", "scale_next_kblock", "scale_next_row", "scale_next_kstep", "sign_ignored",
           "bias_off_by_one", "table_3_4_swapped")

# (N, K) of the kernel tests and the row counts: every MT (1, 2, 4; 40 rows = three 16-row tiles
# run the MT = 4 kernel), the 128-row MT = 8 variant with one and two row tiles, ragged last tiles
SHAPES = [(128, 256), (256, 512), (384, 1024), (768, 512), (1024, 14336)]
ROWS = [1, 15, 16, 17, 40, 64, 65, 128, 200]
X0 = 118  # the lowest scale byte of the grid cases: 2^-9


@dataclasses.dataclass
class Case:
    x: torch.Tensor        # [M, K] bf16
    nib: torch.Tensor      # [N, K / 2] uint8, low nibble = even k (the interchange layout)
    xs: torch.Tensor       # [N, K / 32] uint8 e8m0
    name: str = ""

    @property
    def M(self):
        return self.x.shape[0]

    @property
    def N(self):
        return self.nib.shape[0]

    @property
    def K(self):
        return self.nib.shape[1] * 2


def pack_nibbles(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] codes 0..15 -> [N, K / 2] bytes, low nibble = even k."""
    c = codes.to(torch.int64).view(codes.shape[0], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8)


def codes_of(nib: torch.Tensor) -> torch.Tensor:
    n = nib.to(torch.int64)
    return torch.stack([n & 15, n >> 4], dim=-1).view(nib.shape[0], -1)


def dequant64(c: Case, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [N, K]: E2M1[nibble] * 2^(X - 127), written out independently of ops/reference.py;
    ``mutant``: one of :data:`MUTANTS`, a wrong reading of the same bytes."""
    codes, xs = codes_of(c.nib), c.xs.to(torch.int64)
    table = torch.tensor(E2M1, dtype=torch.float64)
    bias = 127
    if mutant == "nibble_swap":            # high nibble = even k
        codes = codes.view(c.N, -1, 2).flip(-1).reshape(c.N, -1)
    elif mutant == "scale_next_kblock":    # the scale of k-block kb + 1
        xs = torch.roll(xs, -1, dims=1)
    elif mutant == "scale_next_row":       # the scale of row n + 1
        xs = torch.roll(xs, -1, dims=0)
    elif mutant == "scale_next_kstep":     # the scale of the same block of the next 128-deep k-step
        xs = torch.roll(xs, -4, dims=1)
    elif mutant == "sign_ignored":
        codes = codes & 7
    elif mutant == "bias_off_by_one":
        bias = 126
    elif mutant == "table_3_4_swapped":
        table = table.clone()
        table[[3, 4, 11, 12]] = table[[4, 3, 12, 11]]
    else:
        assert mutant is None, mutant
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), (xs - bias).double())
    return (table[codes].view(c.N, -1, 32) * scale[..., None]).view(c.N, -1)


def grid_scales(N: int, K: int, nscales: int) -> torch.Tensor:
    n = torch.arange(N).view(N, 1)
    kb = torch.arange(K // 32).view(1, -1)
    return (X0 + (5 * (n % 16) + 7 * (n // 16) + 3 * kb) % nscales).to(torch.uint8)


def exactness(c: Case) -> float:
    """max over outputs of sum_k |x| |w|, in quanta (the common divisor of every product of a case
    with integer activations): below 2^24 every partial sum is exact in fp32."""
    quantum = 0.5 * 2.0 ** (int(c.xs.min()) - 127)
    return float((c.x.double().abs() @ dequant64(c).abs().t()).max()) / quantum


def grid_case(N: int, K: int, M: int, seed: int = 0) -> Case:
    g = torch.Generator().manual_seed(1000003 * seed + 31 * N + 7 * K + M)
    x = torch.randint(-4, 5, (M, K), generator=g).to(BF16)
    codes = torch.randint(0, 16, (N, K), generator=g)
    c = Case(x, pack_nibbles(codes), grid_scales(N, K, 8 if K <= 1024 else 4), f"grid-{N}x{K}-m{M}")
    assert exactness(c) < 2.0 ** 24, (c.name, exactness(c))
    return c


def random_case(N: int, K: int, M: int, seed: int = 0) -> Case:
    """Random-valued: normal activations, every nibble, scale bytes in [118, 126]."""
    g = torch.Generator().manual_seed(77 + seed + N + K + M)
    x = torch.randn((M, K), generator=g).to(BF16)
    codes = torch.randint(0, 16, (N, K), generator=g)
    xs = torch.randint(118, 127, (N, K // 32), generator=g).to(torch.uint8)
    return Case(x, pack_nibbles(codes), xs, f"random-{N}x{K}-m{M}")


def every_code_case(rows: Optional[slice] = None) -> Case:
    """N = 256, K = 512: every k-block of a row holds all 16 nibbles, and the 4096 (row, k-block)
    pairs hold every scale byte in [2, 252] at least 16 times.  Activations: rows ``rows`` of the
    512 x 512 identity (default: all), so y[m, n] = w[n, k_m]."""
    N, K = 256, 512
    n = torch.arange(N).view(N, 1)
    codes = (torch.arange(K).view(1, K) + n) % 16
    xs = (2 + (16 * n + torch.arange(K // 32).view(1, -1)) % 251).to(torch.uint8)
    x = torch.eye(K, dtype=BF16)[rows if rows is not None else slice(None)]
    return Case(x.contiguous(), pack_nibbles(codes), xs, f"every-code-{rows}")


def position_kstars(K: int) -> List[int]:
    """k* over the edges of a word (8 elements), a lane's 16-byte load (its words are the k-blocks:
    32 apart), a k-block, a 128-deep k-step, a 256-deep LDS chunk, the splits of S = 2 and 4, and K."""
    ks = {0, 7, 8, 15, 16, 31, 32, 39, 63, 64, 95, 96, 127, 128, 255, 256, K // 4 - 1, K // 4, K // 2 - 1, K // 2,
          3 * K // 4 - 1, 3 * K // 4, K - 129, K - 128, K - 33, K - 32, K - 1}
    return sorted(k for k in ks if 0 <= k < K)


def position_rows(N: int) -> List[int]:
    """First and last row of a 16-row tile and of a 128-row n-block."""
    return sorted({n for n in (0, 15, 16, 127, 128, 143, N - 128, N - 113, N - 16, N - 1) if 0 <= n < N})


def position_case(N: int = 256, K: int = 1024) -> Case:
    """X[n, kb] = 119 + (5 (n % 16) + 7 (n // 16) + 3 kb) % 16: 16 distinct values; the next row (+5),
    the next tile (+7), the next n-block (+8), the next k-block (+3) and the same block of the next
    k-step (+12) all differ mod 16.  Nibbles are non-zero, activations one-hot at :func:`position_kstars`."""
    n = torch.arange(N).view(N, 1)
    k = torch.arange(K).view(1, K)
    mag = 1 + (n + k) % 7
    codes = mag + 8 * (((n + k) // 7) % 2)
    xs = (119 + (5 * (n % 16) + 7 * (n // 16) + 3 * torch.arange(K // 32).view(1, -1)) % 16).to(torch.uint8)
    ks = position_kstars(K)
    x = torch.zeros((len(ks), K), dtype=BF16)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    return Case(x, pack_nibbles(codes), xs, f"position-{N}x{K}")


# ----------------------------------------------------------------------------- float64 reference
def ref_slabs(c: Case, S: int = 1, rinv: Optional[torch.Tensor] = None, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [S, M, N]: slab s = sum over k-split s [* rinv]."""
    x, w = c.x.double(), dequant64(c, mutant)
    kper = c.K // S
    out = torch.stack([x[:, i * kper:(i + 1) * kper] @ w[:, i * kper:(i + 1) * kper].t() for i in range(S)])
    if rinv is not None:
        out = out * rinv.double()[None, :, None]
    return out


def ref_sum(c: Case, S: int = 1, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [M, N]: the sum of the slabs."""
    return ref_slabs(c, S, rinv, mutant).sum(0)


def ref_bf16(c: Case, S: int = 1, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [M, N]: one rounding of the sum (the bf16 out / the reduced slabs)."""
    return ref_sum(c, S, rinv, mutant).float().to(BF16)


def split_gate_up(y: torch.Tensor):
    """[M, 2I] interleaved in blocks of 16 -> gate [M, I], up [M, I]."""
    v = y.reshape(y.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(y.shape[0], -1), v[:, :, 1].reshape(y.shape[0], -1)


def ref_silu(c: Case, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [M, N / 2]: bf16(bf16(silu(bf16(gate))) * bf16(up)), silu in float64."""
    g, u = split_gate_up(ref_sum(c, 1, rinv, mutant))
    g, u = g.float().to(BF16).double(), u.float().to(BF16).double()
    sg = (g / (1.0 + torch.exp(-g))).float().to(BF16).double()
    return (sg * u).float().to(BF16)


def abs_dot(c: Case) -> torch.Tensor:
    """float64 [M, N]: sum_k |x| |w| (the summation-error term of the random bounds)."""
    return c.x.double().abs() @ dequant64(c).abs().t()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as values, NaN positions included (-0.0 == 0.0: the sign of a zero sum is not part
    of the contract)."""
    a, b = a.double().cpu(), b.double().cpu()
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------------- sentinels
def sentinel_rows(x: torch.Tensor, extra: int = 3) -> torch.Tensor:
    """``x`` as a view into a buffer whose rows at and beyond M are NaN."""
    buf = torch.full((x.shape[0] + extra, x.shape[1]), float("nan"), dtype=x.dtype, device=x.device)
    buf[: x.shape[0]] = x
    return buf[: x.shape[0]]


def sentinel_out(M: int, N: int, device, dtype=BF16, pad_rows: int = 2, pad_cols: int = 8):
    """(NaN buffer [M + pad_rows, N + pad_cols], its [M, N] view the kernel writes)."""
    buf = torch.full((M + pad_rows, N + pad_cols), float("nan"), dtype=dtype, device=device)
    return buf, buf[:M, :N]


def outside_is_nan(buf: torch.Tensor, M: int, N: int) -> bool:
    return bool(buf[M:].isnan().all()) and bool(buf[:, N:].isnan().all())
