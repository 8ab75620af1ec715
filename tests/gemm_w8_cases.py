"""Case builders and the float64 reference for the weight-only FP8 (W8) GEMM tests, shared by the
CPU tests (tests/unit/test_gemm_w8_cases.py: the cases can fail -- they reject wrong references)
and the GPU tests (tests/kernels/test_gemm_w8.py: the kernels pass them).

The function under test:  y[m, n] = (sum_k x[m, k] * widen(byte[n, k])) * scale[n]  [* rinv[m]],
then the mode's epilogue: one bf16 rounding ("bf16"), fp32 slabs per k-split ("partial"), or
bf16(bf16(silu(bf16(gate))) * bf16(up)) of the interleaved gate / up columns ("silu").

Grid cases are exact: activations are integers in [-4, 4], weight bytes come from the e4m3 values
{0, +-0.5, +-1, +-1.5, +-2, +-3, +-4, +-6, +-8} and scales are powers of two, 2^((n % 8) - 4).
Every product is a multiple of 0.5 of magnitude <= 32, so for K <= 14336 every partial sum is an
integer below 2^24 half-units: exact in fp32 in ANY summation order, and the power-of-two scale
is exact too.  A correct kernel therefore equals the float64 reference bit for bit after the one
final rounding.  ``scales="mixed"`` multiplies the scale of channel n by {1, 1.25, 1.5}[n % 3]:
for K <= 1024 (|acc| <= 2^16 half-units, times 5 or 3: below 2^19) the scaled value is still exact
in fp32, and only these cases can tell a scale applied BEFORE the bf16 rounding from one applied
after it (a power of two commutes with rounding).

Needle cases: everything is zero but one byte at (n*, k*) and one activation at (m*, k*), so
exactly one output element is non-zero, with an exact value.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import torch

FP8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
GRID_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0, -8.0]
MUTANTS = ("scale_next", "kblock_swap", "tile_swap", "gate_up_swap", "drop_last_split", "scale_after_round")

# (N, K) of the kernel tests and the row counts: every MT (1, 2, 4; 40 rows = three 16-row tiles
# run the MT = 4 kernel), the 128-row MT = 8 variant with one and two row tiles, ragged last tiles
SHAPES = [(128, 256), (256, 512), (384, 1024), (768, 512), (1024, 14336)]
ROWS = [1, 15, 16, 17, 40, 64, 65, 128, 200]


@dataclasses.dataclass
class Case:
    x: torch.Tensor        # [M, K] bf16
    b: torch.Tensor        # [N, K] e4m3 bytes, row-major
    scale: torch.Tensor    # [N] fp32
    name: str = ""

    @property
    def M(self):
        return self.x.shape[0]

    @property
    def N(self):
        return self.b.shape[0]

    @property
    def K(self):
        return self.b.shape[1]


def channel_scales(N: int, kind: str = "pow2") -> torch.Tensor:
    n = torch.arange(N)
    s = torch.pow(2.0, ((n % 8) - 4).float())
    if kind == "mixed":
        s = s * torch.tensor([1.0, 1.25, 1.5])[n % 3]
    return s.float()


def grid_case(N: int, K: int, M: int, seed: int = 0, scales: str = "pow2") -> Case:
    g = torch.Generator().manual_seed(1000003 * seed + 31 * N + 7 * K + M)
    x = torch.randint(-4, 5, (M, K), generator=g).to(BF16)
    vals = torch.tensor(GRID_VALUES)
    w = vals[torch.randint(0, len(GRID_VALUES), (N, K), generator=g)]
    b = w.to(FP8)
    assert torch.equal(b.float(), w)  # the grid values are e4m3 values
    assert scales == "pow2" or K <= 1024
    return Case(x, b, channel_scales(N, scales), f"grid-{scales}-{N}x{K}-m{M}")


def random_case(N: int, K: int, M: int, seed: int = 0) -> Case:
    """Random-valued: normal activations, every finite e4m3 byte, scales in [2^-7, 2^-5)."""
    g = torch.Generator().manual_seed(77 + seed + N + K + M)
    x = torch.randn((M, K), generator=g).to(BF16)
    byte = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    byte = torch.where((byte & 0x7F) == 0x7F, byte & 0x80, byte).to(torch.uint8)  # no NaN encodings
    scale = (2.0 ** -7) * (1.0 + 3.0 * torch.rand(N, generator=g))
    return Case(x, byte.view(FP8), scale.float(), f"random-{N}x{K}-m{M}")


def needle_case(N: int, K: int, M: int, n: int, k: int, m: int, xv: float = 3.0, wv: float = -1.5) -> Case:
    x = torch.zeros((M, K), dtype=BF16)
    w = torch.zeros((N, K))
    x[m, k] = xv
    w[n, k] = wv
    return Case(x, w.to(FP8), channel_scales(N), f"needle-{N}x{K}-m{M}-n{n}-k{k}-row{m}")


def needle_points(N: int, K: int) -> List[tuple]:
    """(n*, k*) over the corners of the packed layout: first / last row of a 16-row tile and of a
    128-row n-block; k* at the edges of an 8-byte fragment, a 16-byte load, a 32-deep k-block, a
    128-deep k-step, a 256-deep chunk and the whole K (k* = 0 is in the first split, K - 1 in the
    last, whatever the split)."""
    ns = sorted({n for n in (0, 15, 16, 127, 128, 143, N - 128, N - 1) if 0 <= n < N})
    ks = sorted({k for k in (0, 7, 8, 31, 32, 127, 128, 255, 256, K - 1) if 0 <= k < K})
    return [(n, k) for n in ns for k in ks]


# ----------------------------------------------------------------------------- float64 reference
def _inputs(c: Case, mutant: Optional[str]):
    x, w, s = c.x.double(), c.b.double(), c.scale.double()
    if mutant == "scale_next":          # the scale of channel n + 1
        s = torch.roll(s, -1)
    elif mutant == "kblock_swap":       # two 32-deep k-blocks of the weight swapped
        w = w.clone()
        w[:, 0:32], w[:, 32:64] = c.b.double()[:, 32:64], c.b.double()[:, 0:32]
    elif mutant == "tile_swap":         # two 16-row tiles of the weight swapped (scales stay)
        w = w.clone()
        w[0:16], w[16:32] = c.b.double()[16:32], c.b.double()[0:16]
    return x, w, s


def ref_slabs(c: Case, S: int = 1, rinv: Optional[torch.Tensor] = None, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [S, M, N]: slab s = (sum over k-split s) * scale [* rinv]."""
    x, w, s = _inputs(c, mutant)
    kper = c.K // S
    out = torch.stack([x[:, i * kper:(i + 1) * kper] @ w[:, i * kper:(i + 1) * kper].t() for i in range(S)])
    out = out * s[None, None, :]
    if rinv is not None:
        out = out * rinv.double()[None, :, None]
    if mutant == "drop_last_split" and S > 1:
        out = out[:-1]
    return out


def ref_sum(c: Case, S: int = 1, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """float64 [M, N]: the sum of the slabs."""
    return ref_slabs(c, S, rinv, mutant).sum(0)


def ref_bf16(c: Case, S: int = 1, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [M, N]: one rounding of the scaled sum (the bf16 out / the reduced slabs)."""
    if mutant == "scale_after_round":   # bf16(bf16(sum) * scale): the scale after the rounding
        _, _, s = _inputs(c, None)
        acc = (ref_sum(c, S, rinv) / s[None, :]).float().to(BF16).double()
        return (acc * s[None, :]).float().to(BF16)
    return ref_sum(c, S, rinv, mutant).float().to(BF16)


def split_gate_up(y: torch.Tensor):
    """[M, 2I] interleaved in blocks of 16 -> gate [M, I], up [M, I]."""
    v = y.reshape(y.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(y.shape[0], -1), v[:, :, 1].reshape(y.shape[0], -1)


def ref_silu(c: Case, rinv=None, mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [M, N / 2]: bf16(bf16(silu(bf16(gate))) * bf16(up)), silu in float64."""
    g, u = split_gate_up(ref_sum(c, 1, rinv, mutant))
    if mutant == "gate_up_swap":
        g, u = u, g
    g, u = g.float().to(BF16).double(), u.float().to(BF16).double()
    sg = (g / (1.0 + torch.exp(-g))).float().to(BF16).double()
    return (sg * u).float().to(BF16)


def abs_dot(c: Case) -> torch.Tensor:
    """float64 [M, N]: scale[n] * sum_k |x| |w| (the summation-error term of the random bounds)."""
    return (c.x.double().abs() @ c.b.double().abs().t()) * c.scale.double()[None, :]


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
