"""Case builders, float64 references and criteria for the row-wise kernels of
csrc/kernels/norm_act.hip and csrc/kernels/embedding.hip, shared by the CPU tests
(tests/unit/test_rowwise_cases.py: the cases reject wrong references) and the GPU tests
(tests/kernels/test_rowwise_exact.py: the kernels pass them).  No GPU is touched here.  The
intervals, ``bf``, ``same_bits``, ``inside`` and the derivations of DELTA_R = 5 u and
DELTA_S(x) = (8 + 2 |x|) u are those of tests/gemm_cases.py.

RMSNorm and fused add + RMSNorm
-------------------------------
    r = rsqrtf(ss / H + eps), ss the fp32 sum of the squares;  y = bf16(bf16(v * r) * g);
    fused: v = bf16(a + b) is stored as the new residual and ss is taken from that rounded value.
The product bf16 * bf16 is exact in fp32, so the only inexact quantities are r and the product
v * r: r(1 +- rel) is mapped through both roundings and the output must lie between the ends.

    family     rows                                                      rel              criterion
    pow4       quads (+-2,0,0,0) 2^j and (+-1,+-1,+-1,+-1) 2^j: every    DELTA_R          same_bits
               square is 4^j or 4 4^j, ss is exact in any order and
               ss / H = 4^j; r = 2^-j (1 - e), e = eps / (2 4^j) far
               below half a bf16 ulp (2^-9) for j >= -4, so
               bf16(v * r) = v 2^-j in {0, +-1, +-2}: y is 0, +-g, +-2g
               (the builder asserts it with r perturbed by +-2^-16)
    int        integers in [-20, 20]: H max^2 < 2^24, ss exact            DELTA_R          interval
    eps        pow4 rows with j = -9 (ss / H = 3.8e-6 < eps) alternating  DELTA_R          interval,
               with all-zero rows                                                          zero rows 0
    gauss      randn * 3: ss is a sum of H rounded squares in unknown     (H / 2 + 5) u    interval
               order, n u ref, which rsqrt halves
    rounding   (fused only) up to 128 sums a + b = +-(4 m + 3) q per row  DELTA_R          interval
               need nine significant bits and round away from zero, the
               rest are integers in [-3, 3] q, q = 2^-(t % 5): ss of the
               rounded AND of the unrounded sums are integers below 2^24
               in units of q^2, and the two differ

SiLU-and-mul
------------
    bf16(bf16(silu(g)) * u),  silu(x) = x / (1 + __expf(-x)):  gemm_cases.iv_silu, iv_bf, iv_mul.
Two gate ranges are tightened to exact values:
  * g >= 18: e = __expf(-g) <= e^-18 (1 + 30 u) < 1.6e-8 < 2^-25, so 1 + e rounds to 1 and g / 1 is
    g in either division (the reciprocal of 1 is 1): bf16(silu) is exactly g.  (+inf included.)
  * g <= -89: -g log2(e) >= 128.4, the exp2 overflows to +inf, 1 + inf = inf and g / inf is -0 for
    every finite g; the criterion accepts a zero of either sign.  g = -inf gives inf / inf = NaN,
    as in float64.
The builder asserts that the float64 formula agrees with both: bf16(silu64(g)) == g for every bf16
g >= 18, and |silu64(g)| stays below the overflow floor gemm_cases.SILU_ABS for g <= -89.
NaN is expected exactly where the float64 formula gives NaN (NaN gates, -inf, and inf * 0).

Embedding: a bit copy, compared as int16; rows of ids outside the shard are 0x0000.
Staging copy: a bit copy of ``bytes`` bytes; what follows keeps its sentinel.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

import torch

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, DELTA_R, U, _gen, bf, is_bf16, iv_bf, iv_mul

NORM_MUTANTS = ("eps_dropped", "eps_outside_rsqrt", "mean_over_h_minus_512", "first_vector_only", "weight_by_thread",
                "weight_shift8", "round_once", "rinv_next_row", "in_stride_is_h", "out_stride_is_in_stride")
FUSED_MUTANTS = ("ss_from_x_only", "ss_from_old_residual", "ss_unrounded", "norm_of_unrounded")
SILU_MUTANTS = ("gate_up_swap", "up_offset_2i", "il_block8", "il_half_swap", "silu_unrounded", "last_group_dropped")
EMBED_MUTANTS = ("first_row_dropped", "mask_off_by_one_low", "start_ignored", "tail_vector_dropped", "row_stride_2048")

# H -> (VPT, threads) of the launcher
WIDTHS = {512: (1, 64), 1536: (1, 192), 5120: (1, 640), 8192: (1, 1024), 9216: (2, 576), 24576: (4, 768),
          40960: (8, 640)}
NORM_T = [1, 3, 17]
NORM_EPS = [1e-5, 1e-6]
FAMILIES = ["pow4", "int", "eps", "gauss"]
FUSED_FAMILIES = FAMILIES + ["rounding"]

SILU_I = [8, 16, 2040, 2048, 2064, 14336]
SILU_T = [1, 5]
SILU_UPS = [1.0, -1.0, 1.5, 0.0]
GATE_EXACT = 18.0
GATE_ZERO = -89.0

EMBED_V = 1000
EMBED_H = [8, 2040, 2048, 2056, 5120]
EMBED_T = [1, 77]
# (start, local, the ids fall into the shard)
EMBED_SHARDS = [(0, EMBED_V, True), (250, 300, True), (500, 1, True), (700, 300, True), (400, 200, False)]
NAN_BITS = 0x7FC0  # what torch.full(nan) stores in a bf16 buffer

COPY_BYTES = [16, 4080, 4096, 4112, 64 * 256 * 16, 64 * 256 * 16 + 16, (1 << 20) + 48]
COPY_SENTINEL = -0x0badf00d


def pick_vpt(H: int) -> Tuple[int, int]:
    """(VPT, threads) as the launcher picks them; (-1, 0) for an unsupported width."""
    vecs = H // 8
    for vpt in (1, 2, 4, 8):
        if H % 8 == 0 and vecs % vpt == 0 and vecs // vpt <= 1024 and (vecs // vpt) % 64 == 0:
            return vpt, vecs // vpt
    return -1, 0


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def misses(mut, ref) -> bool:
    """Some element at which no value satisfies both intervals, or at which exactly one is NaN:
    a kernel with the mutant's bug fails the reference criterion there."""
    (ml, mh), (rl, rh) = mut, ref
    assert ml.shape == rl.shape
    mn, rn = ml.isnan() | mh.isnan(), rl.isnan() | rh.isnan()
    return bool(((mn != rn) | (~mn & ~rn & ((mh < rl) | (ml > rh)))).any())


def count_off(got: torch.Tensor, mid: torch.Tensor) -> int:
    """How many outputs differ from the zero-slack reference (a record, never a criterion)."""
    got = got.double().cpu()
    return int((~((got == mid) | (got.isnan() & mid.isnan()))).sum())


# ------------------------------------------------------------------------------------------ norms
@dataclasses.dataclass
class NormCase:
    name: str
    family: str
    a: torch.Tensor            # float64 [T, H] of bf16 values: the input, or x of the fused kernel
    b: Optional[torch.Tensor]  # float64 [T, H]: the old residual of the fused kernel
    w: torch.Tensor            # float64 [H] of bf16 values
    eps: float
    rel: float                 # r, product rounding included, is known to within this relative error
    exact: bool = False        # the interval is a point at every element: same_bits

    @property
    def T(self):
        return self.a.shape[0]

    @property
    def H(self):
        return self.a.shape[1]


def _pow4_rows(T: int, H: int, g: torch.Generator, j: torch.Tensor) -> torch.Tensor:
    nq = H // 4
    kind = torch.randint(0, 2, (T, nq), generator=g)                     # 0: (2,0,0,0)  1: (1,1,1,1)
    pos = torch.randint(0, 4, (T, nq), generator=g)
    sign = (2 * torch.randint(0, 2, (T, nq, 4), generator=g) - 1).double()
    two = torch.zeros((T, nq, 4), dtype=torch.float64).scatter_(2, pos[..., None], 2.0)
    quad = torch.where(kind[..., None] == 1, torch.ones_like(two), two) * sign
    return quad.view(T, H) * (2.0 ** j.double())[:, None]


def _rounding_rows(T: int, H: int, g: torch.Generator):
    """(a, b, q): see the module docstring."""
    q = 2.0 ** -(torch.arange(T) % 5).double()
    v = torch.randint(-3, 4, (T, H), generator=g).double()
    d = torch.randint(-2, 3, (T, H), generator=g).double()
    a, b = v + d, -d
    n = min(128, H // 4)
    for t in range(T):
        cols = torch.randperm(H, generator=g)[:n]
        m = torch.randint(64, 68, (n,), generator=g).double()           # sums 259, 263, 267, 271
        s = (2 * torch.randint(0, 2, (n,), generator=g) - 1).double()
        a[t, cols] = s * (4 * m + 2)
        b[t, cols] = s
    return a * q[:, None], b * q[:, None], q


def norm_case(family: str, T: int, H: int, eps: float = 1e-5, fused: bool = False, seed: int = 0) -> NormCase:
    assert pick_vpt(H)[0] > 0
    g = _gen(31, FUSED_FAMILIES.index(family), T, H, int(fused), seed)
    w = bf(torch.randn(H, generator=g))
    name = f"{'fused-' if fused else ''}{family}-T{T}-H{H}-eps{eps:g}"
    unit, rel, exact, b = None, DELTA_R, False, None
    if family == "pow4":
        j = -4 + (3 * torch.arange(T) + seed) % 8                        # differs from row to row
        v, unit, exact = _pow4_rows(T, H, g, j), 2.0 ** j.double(), True
    elif family == "int":
        v, unit = torch.randint(-20, 21, (T, H), generator=g).double(), torch.ones(T, dtype=torch.float64)
    elif family == "eps":
        j = torch.full((T,), -9)
        v, unit = _pow4_rows(T, H, g, j), 2.0 ** j.double()
        v[1::2] = 0
    elif family == "gauss":
        v, rel = bf(torch.randn((T, H), generator=g) * 3), (H / 2 + 5) * U
    else:
        assert family == "rounding" and fused
        a, b, unit = _rounding_rows(T, H, g)
        v = bf(a + b)
    if fused and family == "gauss":
        a, b = v, bf(torch.randn((T, H), generator=g))
        b[:, ::7] = -a[:, ::7]                                           # a = -b: the new residual is 0
        v = bf(a + b)
    elif fused and family != "rounding":
        d = torch.randint(-8, 9, (T, H), generator=g).double() * unit[:, None]
        a, b = v + d, -d
        assert bool((bf(a + b) == v).all()), name
    elif not fused:
        a = v
    assert is_bf16(a) and is_bf16(w) and (b is None or is_bf16(b)), name
    c = NormCase(name, family, a, b, w, eps, rel, exact)
    # ---- the budget of the family
    if unit is not None:
        for src in ((v,) if family != "rounding" else (v, a + b)):
            sq = (src / unit[:, None]).pow(2)
            assert bool((sq == sq.round()).all()) and float(sq.sum(-1).max()) < 2 ** 24, name
    if family == "int":
        assert H * 20 ** 2 < 2 ** 24 and float(v.abs().max()) <= 20
    if family in ("pow4", "eps"):
        rows = slice(None) if family == "pow4" else slice(0, None, 2)
        assert bool((v[rows].pow(2).sum(-1) / H == unit[rows] ** 2).all()), name
    if family == "pow4":
        want = v / unit[:, None]
        assert set(want.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        for e in NORM_EPS:
            r = 1.0 / torch.sqrt(v.pow(2).sum(-1) / H + f32(e))
            for pert in (1.0 - 2.0 ** -16, 1.0, 1.0 + 2.0 ** -16):       # far more than the fp32 error of r
                assert bool((bf(v * (r * pert)[:, None]) == want).all()), name
        lo, hi = ref_norm(c)[0]
        assert bool((lo == hi).all()) and bool((lo == want * w[None, :]).all()), name
    if family == "eps":
        assert float((v.pow(2).sum(-1) / H).max()) < eps and (T == 1 or not bool(v[1].any()))
        lo, hi = ref_norm(c)[0]
        assert bool((lo[1::2] == 0).all()) and bool((hi[1::2] == 0).all())
    if family == "rounding":
        s = a + b
        odd = bf(s) != s
        assert 0 < int(odd.sum(-1).max()) <= 128 and bool((bf(s)[odd].abs() > s[odd].abs()).all()), name
        good = ref_norm(c)[0]
        for mutant in ("ss_unrounded", "norm_of_unrounded"):
            assert misses(ref_norm(c, mutant)[0], good), (name, mutant)
    return c


def _rinv(v: torch.Tensor, H: int, eps: float, threads: int, mutant: Optional[str]) -> torch.Tensor:
    """float64 [T]: 1 / sqrt(ss / H + eps), eps as the fp32 value the kernel receives."""
    sq = v.pow(2)
    vec = torch.arange(H) // 8
    if mutant == "mean_over_h_minus_512":    # the last wave's partial sum is lost
        sq = sq * (vec % threads < threads - 64).double()[None, :]
    elif mutant == "first_vector_only":      # ss from i = 0 only
        sq = sq * (vec < threads).double()[None, :]
    ms, e = sq.sum(-1) / H, f32(eps)
    if mutant == "eps_dropped":
        r = 1.0 / torch.sqrt(ms)
    elif mutant == "eps_outside_rsqrt":
        r = 1.0 / torch.sqrt(ms) + e
    else:
        r = 1.0 / torch.sqrt(ms + e)
    return torch.roll(r, -1) if mutant == "rinv_next_row" else r


def ref_norm(c: NormCase, mutant: Optional[str] = None):
    """((lo, hi) float64 [T, H] of bf16 values, new residual float64 [T, H] or None)."""
    H = c.H
    _, threads = pick_vpt(H)
    if c.b is None:
        new, v, src = None, c.a, c.a
    else:
        s = c.a + c.b                       # bf() rounds to fp32 first, as the kernel's addition does
        new = bf(s)
        src = {"ss_from_x_only": c.a, "ss_from_old_residual": c.b, "ss_unrounded": s}.get(mutant, new)
        v = s if mutant == "norm_of_unrounded" else new
    r = _rinv(src, H, c.eps, threads, mutant)
    w = c.w
    if mutant == "weight_by_thread":        # g[threadIdx.x] for every i
        col = torch.arange(H)
        w = w[(col // 8 % threads) * 8 + col % 8]
    elif mutant == "weight_shift8":
        w = torch.roll(w, -8)
    vr = iv_mul((v, v), ((r * (1 - c.rel))[:, None].expand_as(v), (r * (1 + c.rel))[:, None].expand_as(v)))
    if mutant != "round_once":
        vr = iv_bf(vr)
    wv = w[None, :].expand_as(v)
    return iv_bf(iv_mul(vr, (wv, wv))), new


def norm_mid(c: NormCase) -> torch.Tensor:
    """The float64 reference without any slack."""
    return ref_norm(dataclasses.replace(c, rel=0.0))[0][0]


# the column slices of the plain kernel: (row0, col0, extra columns, extra rows); row strides H + 24 and H + 16
IN_GEOM = (1, 8, 24, 2)
OUT_GEOM = (1, 8, 16, 2)


def sliced(x: torch.Tensor, geom, fill=float("nan")):
    """(buffer [T + extra rows, H + extra columns] of ``fill``, its [T, H] slice holding ``x``)."""
    row0, col0, pc, pr = geom
    T, H = x.shape
    buf = torch.full((T + pr, H + pc), fill, dtype=x.dtype, device=x.device)
    view = buf[row0:row0 + T, col0:col0 + H]
    view.copy_(x)
    return buf, view


def ref_norm_sliced(c: NormCase, mutant: Optional[str] = None):
    """(lo, hi) of the whole OUT_GEOM buffer after rms_norm read the IN_GEOM slice: NaN outside."""
    T, H = c.T, c.H
    inbuf, _ = sliced(c.a, IN_GEOM)
    sin = H if mutant == "in_stride_is_h" else inbuf.shape[1]
    idx = IN_GEOM[0] * inbuf.shape[1] + IN_GEOM[1] + torch.arange(T)[:, None] * sin + torch.arange(H)[None, :]
    iv = ref_norm(dataclasses.replace(c, a=inbuf.view(-1)[idx]), mutant)[0]
    wout = H + OUT_GEOM[2]
    n = (T + OUT_GEOM[3]) * wout
    sout = inbuf.shape[1] if mutant == "out_stride_is_in_stride" else wout
    odx = OUT_GEOM[0] * wout + OUT_GEOM[1] + torch.arange(T)[:, None] * sout + torch.arange(H)[None, :]
    ok = odx < n                            # (the mutant's model drops what falls beyond the buffer)
    out = []
    for e in iv:
        flat = torch.full((n,), float("nan"), dtype=torch.float64)
        flat[odx[ok]] = e[ok]
        out.append(flat.view(T + OUT_GEOM[3], wout))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------- SiLU
def iv_silu_gate(g: torch.Tensor):
    """The interval of x / (1 + __expf(-x)) for the exactly known gate ``g`` (float64 of bf16 values,
    NaN and infinities allowed): gemm_cases.iv_silu, tightened for g >= 18 and g <= -89."""
    lo, hi = gc.iv_silu((g, g))
    big, neg = g >= GATE_EXACT, (g <= GATE_ZERO) & (g > -float("inf"))
    fin = g[big & g.isfinite()]
    assert bool((bf(gc.silu64(fin)) == fin).all())                        # float64 agrees: bf16(silu) = g
    assert bool((gc.silu64(g[neg]).abs() < gc.SILU_ABS).all())            # float64 agrees: below the floor
    assert bool(((lo[neg] <= 0) & (hi[neg] >= 0)).all())
    zero = torch.zeros_like(g)
    lo = torch.where(big, g, torch.where(neg, -zero, lo))
    hi = torch.where(big, g, torch.where(neg, zero, hi))
    bad = g.isnan() | (g == -float("inf"))
    nan = torch.full_like(g, float("nan"))
    return torch.where(bad, nan, lo), torch.where(bad, nan, hi)


def join_gate_up(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """gate [T, I], up [T, I] -> [T, 2I] interleaved in blocks of 16 (inverse of split_gate_up)."""
    T = g.shape[0]
    return torch.stack([g.reshape(T, -1, 16), u.reshape(T, -1, 16)], dim=2).reshape(T, -1)


def silu_operands(x: torch.Tensor, il: bool, mutant: Optional[str] = None):
    """(gate, up) float64 [T, I] as the kernel of the layout pairs them."""
    T, I = x.shape[0], x.shape[1] // 2
    if not il:
        g, u = x[:, :I], x[:, I:]
        if mutant == "up_offset_2i":        # up read at 2 I: the gate of the next row
            u = torch.roll(g, -1, 0)
    elif mutant == "il_block8":             # blocks of 8 instead of 16
        v = x.reshape(T, -1, 2, 8)
        g, u = v[:, :, 0].reshape(T, I), v[:, :, 1].reshape(T, I)
    else:
        g, u = gc.split_gate_up(x)
        if mutant == "il_half_swap":        # the two 8-column halves of a block exchanged on the way in
            g = g.reshape(T, -1, 2, 8).flip(2).reshape(T, I)
            u = u.reshape(T, -1, 2, 8).flip(2).reshape(T, I)
    if mutant == "gate_up_swap":
        g, u = u, g
    return g, u


def ref_silu_mul(x: torch.Tensor, il: bool, mutant: Optional[str] = None, tail: int = 64, slack: bool = True):
    """(lo, hi) float64 of the flat output buffer [T * I + tail] (the tail stays NaN) for the bf16
    input ``x`` [T, 2I] (float64).  ``slack=False``: the zero-slack reference (both ends equal)."""
    T, I = x.shape[0], x.shape[1] // 2
    g, u = silu_operands(x, il, mutant)
    if slack:
        s = iv_silu_gate(g)
    else:
        m = gc.silu64(g)
        m = torch.where(m.abs() < gc.SILU_ABS, torch.zeros_like(m), m)
        s = (m, m)
    if mutant != "silu_unrounded":
        s = iv_bf(s)
    lo, hi = iv_bf(iv_mul(s, (u, u)))
    if mutant == "last_group_dropped" and (I // 8) % 256:
        lo, hi = lo.clone(), hi.clone()
        lo[:, (I // 8) // 256 * 2048:] = float("nan")
        hi[:, (I // 8) // 256 * 2048:] = float("nan")
    pad = torch.full((tail,), float("nan"), dtype=torch.float64)
    return torch.cat([lo.reshape(-1), pad]), torch.cat([hi.reshape(-1), pad])


def silu_gauss(T: int, I: int, seed: int = 0) -> torch.Tensor:
    """float64 [T, 2I] of bf16 values, randn * 2."""
    return bf(torch.randn((T, 2 * I), generator=_gen(37, T, I, seed)) * 2)


def all_gates() -> torch.Tensor:
    """bf16 [65536]: every bit pattern."""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)


def silu_sweep(il: bool) -> torch.Tensor:
    """bf16 [4, 2 * 65536]: row t pairs every bf16 bit pattern as gate with the up value SILU_UPS[t]."""
    g = all_gates()[None, :].expand(len(SILU_UPS), -1)
    u = torch.tensor(SILU_UPS, dtype=BF16)[:, None].expand_as(g)
    return (join_gate_up(g, u) if il else torch.cat([g, u], dim=1)).contiguous()


# -------------------------------------------------------------------------------------- embedding
def embed_table(local: int, H: int, seed: int = 0) -> torch.Tensor:
    """int16 [local, H] of random bit patterns (-0, NaN payloads, subnormals, infinities)."""
    return torch.randint(-32768, 32768, (local, H), generator=_gen(41, local, H, seed), dtype=torch.int32).to(torch.int16)


def embed_special_ids(start: int, local: int, holds: bool, V: int = EMBED_V) -> List[int]:
    """start - 1, start, start + local - 1, start + local, 0, V - 1, as far as they are valid ids
    (and, for the shard that must hold none of the ids, outside the shard)."""
    ids = [i for i in (start - 1, start, start + local - 1, start + local, 0, V - 1) if 0 <= i < V]
    if not holds:
        ids = [i for i in ids if not start <= i < start + local]
    return list(dict.fromkeys(ids))


def embed_ids(T: int, start: int, local: int, holds: bool, seed: int = 0, V: int = EMBED_V) -> torch.Tensor:
    """int64 [T]: the special ids at random positions among random ids (T >= 6)."""
    g = _gen(43, T, start, local, int(holds), seed)
    ids = torch.randint(0, V, (T,), generator=g)
    if not holds:
        out = torch.cat([torch.arange(0, start), torch.arange(start + local, V)])
        ids = out[torch.randint(0, out.numel(), (T,), generator=g)]
    sp = embed_special_ids(start, local, holds, V)
    ids[torch.randperm(T, generator=g)[:len(sp)]] = torch.tensor(sp)
    assert set(sp) <= set(ids.tolist()) and int(ids.min()) >= 0 and int(ids.max()) < V
    if not holds:
        assert not bool(((ids >= start) & (ids < start + local)).any())
    return ids


def ref_embedding(table: torch.Tensor, ids: torch.Tensor, start: int, local: int, mutant: Optional[str] = None,
                  tail: int = 64) -> torch.Tensor:
    """int16 [T * H + tail]: the output buffer, started from NaN, after the gather."""
    H = table.shape[1]
    loc = ids.reshape(-1).long() - (0 if mutant == "start_ignored" else start)
    low = {"first_row_dropped": 1, "mask_off_by_one_low": -1}.get(mutant, 0)
    mine = (loc >= low) & (loc < local)
    stride = 2048 if mutant == "row_stride_2048" else H
    flat = table.reshape(-1)
    idx = (loc[:, None] * stride + torch.arange(H)[None, :]) % flat.numel()   # (a mutant's stray reads wrap)
    out = torch.where(mine[:, None], flat[idx], torch.zeros((), dtype=torch.int16))
    if mutant == "tail_vector_dropped" and (H // 8) % 256:                   # the partial pass of the copy loop
        out[:, (H // 8) // 256 * 2048:] = NAN_BITS
    return torch.cat([out.reshape(-1), torch.full((tail,), NAN_BITS, dtype=torch.int16)])


# ----------------------------------------------------------------------------------- staging copy
def copy_grid(nbytes: int) -> Tuple[int, int]:
    """(workgroups, passes of the grid-stride loop of the busiest workgroup) of the launcher."""
    n16 = nbytes // 16
    grid = min(n16 // 256 + 1, 64)
    return grid, -(-n16 // (grid * 256))


def copy_source(nbytes: int, pin: bool = False) -> torch.Tensor:
    """int32 counter pattern of ``nbytes`` bytes plus 16 words the copy must not read into the
    destination."""
    n = nbytes // 4 + 16
    src = torch.zeros(n, dtype=torch.int32, pin_memory=pin)
    src.copy_(torch.arange(n, dtype=torch.int64).mul_(2654435761).remainder_(2 ** 31).to(torch.int32))
    return src
