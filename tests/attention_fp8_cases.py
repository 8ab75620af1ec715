"""FP8 (e4m3) twins of the exact attention cases (tests/attention_cases.py, used as a library).

A twin keeps the case's sequences, queries and block tables and replaces the caches: ``kc8`` /
``vc8`` are the bytes the reference cast ``e4m3(clamp(x / scale, -448, 448))`` makes of the
case's K / V (what the kernels read), and the ``Case`` itself holds the *dequantised* bf16
tensors ``scale * byte``, so ``attention_cases.reference`` / ``check`` / ``mutants`` apply
unchanged -- the float64 reference of an FP8 launch is the reference over what the cache holds.

Poison.  V poison 2^100 is not representable: it becomes the largest finite value, stored +-448
(it must stay finite: the kernels multiply a masked key's V by p = 0).  A quiet-poison case (K
poison 0) then needs ``v_scale >= 2`` for its slot after the context to stay loud enough
(tests/unit/test_attention_fp8_cases.py shows the misses at 1); the loud K poison 2^10 E has
entries 256 and is representable.

Scales are powers of two, so ``scale * byte`` is exact in bf16.  Negative zeros are cleared from
the twin's bytes.  The fused decode tests still meet the sign of a zero: their new rows are fp32
slab sums (which turn a -0 target into +0) rotated by quarter turns, and 0 * c - 0 * s is -0 for
some sign patterns.  ``fused_inputs`` therefore derives the bytes the launch must leave from the
slabs themselves, through the CPU reference writer, and the GPU caches are compared with those
byte for byte, sign of zero included; the expectation equals the twin's bytes everywhere else.
"""
import dataclasses
import functools

import torch

from polykey_service_amd.ops import reference as ref
from tests import attention_cases as ac

FP8 = ref.FP8
quantize = ref.quantize_fp8   # the reference cast: clamp in fp32, then torch's CPU round-to-nearest-even e4m3 cast


def dequantize(c: torch.Tensor, scale: float) -> torch.Tensor:
    """bf16 ``scale * byte`` (exact for the power-of-two scales used here)."""
    f = c.float() * scale
    out = f.to(torch.bfloat16)
    assert torch.equal(out.float(), f), "scale * byte is not a bf16 number"
    return out


def _no_negative_zero(c: torch.Tensor) -> torch.Tensor:
    b = c.view(torch.uint8).clone()
    b[b == 0x80] = 0
    return b.view(FP8)


@dataclasses.dataclass
class Fp8Case:
    case: ac.Case           # kc / vc: the dequantised bf16 caches (for reference() and mutants())
    kc8: torch.Tensor       # [blocks, nkv, bs, 128] float8_e4m3fn: the bytes the kernels read
    vc8: torch.Tensor       # [blocks, nkv, 128, bs] float8_e4m3fn
    k_scale: float
    v_scale: float


def fp8_twin(case: ac.Case, k_scale: float, v_scale: float) -> Fp8Case:
    kc8 = _no_negative_zero(quantize(case.kc, k_scale))
    vc8 = _no_negative_zero(quantize(case.vc, v_scale))
    twin = dataclasses.replace(case, kc=dequantize(kc8, k_scale), vc=dequantize(vc8, v_scale))
    assert torch.isfinite(twin.kc.float()).all() and torch.isfinite(twin.vc.float()).all()
    return Fp8Case(twin, kc8, vc8, k_scale, v_scale)


# (k_scale, v_scale) per case: quiet poison needs v_scale >= 2, loud cases run at either
DECODE = {"p128_g8_bs32_quiet": (0.5, 2.0), "p512_g4_bs32_loud": (1.0, 1.0), "p128_g16_bs96_loud": (2.0, 0.5)}
PREFILL = {"g1_bs32_quiet": (0.5, 2.0), "g4_bs96_quiet": (0.5, 2.0), "g8_bs32_loud": (1.0, 1.0),
           "g3_bs64_quiet": (2.0, 4.0)}
MIXED = (0.5, 2.0)


@functools.lru_cache(maxsize=None)
def decode_case(name: str, scales=None) -> Fp8Case:
    return fp8_twin(ac.decode_case(name), *(scales or DECODE[name]))


@functools.lru_cache(maxsize=None)
def prefill_case(name: str, scales=None) -> Fp8Case:
    return fp8_twin(ac.prefill_case(name), *(scales or PREFILL[name]))


@functools.lru_cache(maxsize=None)
def mixed_case() -> Fp8Case:
    return fp8_twin(ac.mixed_case(), *MIXED)


@functools.lru_cache(maxsize=None)
def reference(kind: str, name: str = "") -> ac.Ref:
    """The float64 reference over the dequantised cache, computed once per case."""
    f = {"decode": decode_case, "prefill": prefill_case}[kind](name) if kind != "mixed" else mixed_case()
    return ac.reference(f.case)


@dataclasses.dataclass
class Fp8FusedInputs:
    fi: ac.FusedInputs      # slabs / targets / positions / slots / rotation table of the twin
    kc0: torch.Tensor       # the FP8 caches before the launch: the new tokens' rows hold poison
    vc0: torch.Tensor
    kc_want: torch.Tensor   # the bytes the launch must leave: the CPU reference writer on the slab sums
    vc_want: torch.Tensor
    neg_zeros: int          # K bytes of kc_want that are -0 where the twin holds +0 (all its differences)


def fused_inputs(f: Fp8Case, S: int, fold: bool) -> Fp8FusedInputs:
    """attention_cases.fused_inputs of the twin.  The k / v targets are ``scale * byte`` of the
    rows the kernel must write, so they are FP8-representable by construction.  The expected
    caches come from what the kernel is actually given: the slabs summed in its order, rounded to
    bf16, rotated and quantised by ops.reference.rope_and_cache into a copy of kc0 / vc0.  They
    equal the twin's bytes except that some zeros of the new K rows are -0 (asserted here)."""
    case = f.case
    fi = ac.fused_inputs(case, S, fold)
    kc0, vc0 = quantize(fi.kc0, f.k_scale), quantize(fi.vc0, f.v_scale)
    kc, vc = kc0.clone(), vc0.clone()
    qkv = ac.sequential_sum(fi.slabs).to(torch.bfloat16)
    ref.rope_and_cache(qkv, fi.positions, fi.cos_sin, kc, vc, fi.slots, case.nq, case.nkv, ac.HD,
                       k_scale=f.k_scale, v_scale=f.v_scale)
    n, pairs = byte_mismatches(kc, f.kc8)
    assert pairs in ([], [[0x80, 0x00]]), pairs
    assert same_bytes(vc, f.vc8)
    return Fp8FusedInputs(fi, kc0, vc0, kc, vc, n)


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def byte_mismatches(got: torch.Tensor, want: torch.Tensor):
    """-> (number of differing bytes, the distinct (got, want) byte pairs, at most 8)."""
    g, w = got.cpu().view(torch.uint8), want.cpu().view(torch.uint8)
    bad = g != w
    pairs = torch.stack([g[bad], w[bad]], dim=1).unique(dim=0)[:8].tolist() if bool(bad.any()) else []
    return int(bad.sum()), pairs


# ------------------------------------------------------------------ rope_and_cache byte test
SPECIAL = (1.0625, 1.1875, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.0 ** -10, 448.0, -448.0, 464.0, 1e4, -0.0)


def writer_inputs(T: int, nq: int, nkv: int, seed: int) -> torch.Tensor:
    """qkv [T, (nq + 2 nkv) * 128] bf16: e4m3 rounding ties (1.0625 -> 1.0, 1.1875 -> 1.25), the
    subnormal edge (2^-9 kept, 1.5 * 2^-9 -> 2^-8, 2^-10 -> 0), the clamp (+-448, 464, 1e4) and
    -0.0, with either sign, spread over every row of q, k and v; the rest random."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, nq + 2 * nkv, ac.HD, generator=g) * 4
    sp = torch.tensor(SPECIAL)
    idx = torch.randint(0, len(SPECIAL), x.shape, generator=g)
    pick = torch.rand(x.shape, generator=g) < 0.5
    sign = torch.where(torch.rand(x.shape, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(pick, sp[idx] * sign, x).to(torch.bfloat16)
    for v in SPECIAL:   # every special value is present in k and in v
        b = torch.tensor(v).to(torch.bfloat16)
        for part in (x[:, nq:nq + nkv], x[:, nq + nkv:]):
            assert ((part == b) & (torch.signbit(part) == torch.signbit(b))).any(), v
    return x.view(T, -1)


def expected_cache(qkv, positions, cos_sin, slots, nq, nkv, bs, num_blocks, k_scale, v_scale, fill=0x7E):
    """(K bytes, V bytes, rotated qkv) by the CPU reference on caches pre-filled with ``fill``."""
    kc = torch.full((num_blocks, nkv, bs, ac.HD), fill, dtype=torch.uint8).view(FP8)
    vc = torch.full((num_blocks, nkv, ac.HD, bs), fill, dtype=torch.uint8).view(FP8)
    q = qkv.clone()
    ref.rope_and_cache(q, positions, cos_sin, kc, vc, slots, nq, nkv, ac.HD, k_scale=k_scale, v_scale=v_scale)
    return kc, vc, q
