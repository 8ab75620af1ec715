"""The W8 (weight-only FP8) GEMM on the CPU: the packed layout round trip, the quantiser, the
fp32 reference op against the float64 reference, and -- this repository's convention -- proof
that the inputs the GPU tests use can fail: the case set rejects every mutant reference."""
import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_w8
from polykey_service_amd.ops import reference as ref
from tests import gemm_w8_cases as wc

FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [256, 1024])
def test_pack_unpack_round_trip(N, K):
    g = torch.Generator().manual_seed(N + K)
    b = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    p = gemm_w8.pack_w8(b)
    assert p.shape == b.shape and p.dtype == torch.uint8 and not torch.equal(p, b)
    assert torch.equal(gemm_w8.unpack_w8(p), b)
    assert torch.equal(torch.sort(p.view(-1)).values, torch.sort(b.view(-1)).values)  # a permutation


def test_packed_layout_is_the_one_the_kernel_reads():
    """Byte (n, k) sits where the kernel's lane address finds it: n-block, 128-deep k-step, 16-row
    tile, 16-byte load jj, lane 16 g + r, half, element."""
    N, K = 256, 512
    b = (torch.arange(N * K, dtype=torch.int64) % 251).to(torch.uint8).view(N, K)
    p = gemm_w8.pack_w8(b).view(-1)
    for n, k in [(0, 0), (15, 7), (16, 8), (127, 31), (128, 32), (143, 127), (200, 128), (255, 511), (77, 300)]:
        nb, tile, r = n // 128, (n % 128) // 16, n % 16
        ks, kk = k // 128, k % 128
        s, g, e = kk // 32, (kk % 32) // 8, kk % 8
        jj, half = s // 2, s % 2
        off = nb * 128 * K + ks * 16384 + tile * 2048 + jj * 1024 + (16 * g + r) * 16 + half * 8 + e
        assert int(p[off]) == int(b[n, k]), (n, k)


def test_pack_rejects_other_shapes():
    for shape in ((64, 256), (128, 128), (192, 256), (128, 384)):
        with pytest.raises(AssertionError):
            gemm_w8.pack_w8(torch.zeros(shape, dtype=torch.uint8))


# ------------------------------------------------------------------------------------- quantiser
def test_quantiser_bytes_scales_and_error_bound():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn((128, 256), generator=g) * torch.logspace(-3, 2, 128)[:, None]).to(torch.bfloat16)
    w[7] = 0                       # an all-zero row
    w[9, 3] = 1e-30                # far below the row's subnormal step
    b, scale = ref.quantize_fp8_rows(w)
    assert b.dtype == FP8 and scale.dtype == torch.float32 and scale.shape == (128,)
    amax = w.float().abs().amax(1)
    assert torch.equal(scale[amax > 0], (amax / 448.0)[amax > 0]) and float(scale[7]) == 1.0
    assert int(b[7].view(torch.uint8).max()) == 0
    # the bytes are quantize_fp8 of w / scale, and the row maximum lands on +-448
    assert torch.equal(b.view(torch.uint8), ref.quantize_fp8(w.float() / scale[:, None]).view(torch.uint8))
    assert torch.equal(b.float().abs().amax(1)[amax > 0], torch.full((127,), 448.0))
    # e4m3 keeps 3 mantissa bits: round-to-nearest is off by at most half an ulp = 2^-4 |q| for a
    # normal q, and by at most half the subnormal step 2^-9 below 2^-6; q = w / scale itself is one
    # fp32 division (relative 2^-24).  In float64:
    q = w.double() / scale.double()[:, None]
    err = (b.double() - q).abs()
    bound = torch.maximum(2.0 ** -4 * q.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64)) + 2.0 ** -23 * q.abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    deq = b.double() * scale.double()[:, None]
    assert bool(((deq - w.double()).abs() <= scale.double()[:, None] * bound).all())
    # the handle: packed bytes, scales, shape, bytes held
    h = gemm_w8.W8.from_weight(w)
    assert h.shape == (128, 256) and h.nbytes == 128 * 256 + 4 * 128 and h.packed.dtype == torch.uint8
    assert torch.equal(h.bytes_rowmajor().view(torch.uint8), b.view(torch.uint8)) and torch.equal(h.scale, scale)
    assert torch.equal(h.dequant().double(), deq.float().double())


# --------------------------------------------------------------------------- fp32 reference op
@pytest.mark.parametrize("N,K", [(128, 256), (384, 1024), (256, 14336)])
def test_fp32_reference_is_exact_on_the_grid(N, K):
    c = wc.grid_case(N, K, 17)
    assert torch.equal(ref.w8_linear(c.x, c.b, c.scale).double(), wc.ref_sum(c))
    assert torch.equal(ref.w8_linear_f64(c.x, c.b, c.scale), wc.ref_sum(c))
    rinv = torch.pow(2.0, -(torch.arange(17) % 5).float())
    assert torch.equal(ref.w8_linear(c.x, c.b, c.scale, rinv).double(), wc.ref_sum(c, rinv=rinv))
    # the CPU ops are that reference plus the epilogue
    h = gemm_w8.W8.from_bytes(c.b, c.scale)
    assert wc.same_bits(gemm_w8.linear(c.x, h), wc.ref_bf16(c))
    ws = torch.empty(16 * 17 * N)  # room for the largest split the GPU tiling could pick
    assert wc.same_bits(gemm_w8.linear_partial(c.x, h, ws).view().sum(0), wc.ref_sum(c))
    # SiLU: gate and up are exact, fp32 silu is not float64 silu: its last-bit difference can flip
    # the bf16 rounding of silu(gate) (2^-8 relative) and with it the rounding of the product;
    # for a very negative gate fp32's sigmoid underflows (below 2^-126 it may flush to zero): an
    # absolute 2^-126 |gate| on silu, times |up|
    got, want = gemm_w8.linear_silu(c.x, h).double(), wc.ref_silu(c).double()
    gate, up = (t.abs() for t in wc.split_gate_up(wc.ref_sum(c)))
    assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 2.0 ** -126 * (1 + gate) * (1 + up)).all())
    assert wc.same_bits(gemm_w8.widen(h), c.b.float()) and gemm_w8.widen(h).dtype == torch.bfloat16
    y = torch.randn(5, N).to(torch.bfloat16)
    want = (y.float() * c.scale[None, :]).to(torch.bfloat16)
    assert wc.same_bits(gemm_w8.col_scale(y.clone(), c.scale), want)


def test_random_case_reference_within_its_bound():
    """The fp32 op against float64 on random values, within the bound the GPU tests use."""
    c = wc.random_case(384, 1024, 17)
    got = ref.w8_linear(c.x, c.b, c.scale).to(torch.bfloat16).double()
    want = wc.ref_sum(c)
    bound = 2.0 ** -8 * want.abs() + c.K * 2.0 ** -23 * wc.abs_dot(c)
    assert bool(((got - want).abs() <= bound).all())
    assert not bool(c.b.float().isnan().any())


# --------------------------------------------------------------------------------------- mutants
def _case_set():
    """What the GPU tests run, at the sizes that keep this CPU test quick: grids (power-of-two and
    mixed scales) and the needles of two shapes."""
    cases = [wc.grid_case(N, K, M) for (N, K) in wc.SHAPES[:4] for M in (1, 17)]
    cases += [wc.grid_case(N, K, 17, scales="mixed") for (N, K) in wc.SHAPES[:4]]
    for N, K in ((256, 512), (384, 1024)):
        cases += [wc.needle_case(N, K, 17, n, k, m) for (n, k) in wc.needle_points(N, K) for m in (0, 16)]
    return cases


def _views(c, mutant):
    """Every output the GPU tests compare, for one reference (mutant or not)."""
    S = 4 if c.K % 1024 == 0 else 2
    return [wc.ref_bf16(c, mutant=mutant), wc.ref_sum(c, S, mutant=mutant), wc.ref_bf16(c, S, mutant=mutant),
            wc.ref_silu(c, mutant=mutant)]


@pytest.mark.parametrize("mutant", wc.MUTANTS)
def test_the_case_set_rejects_each_mutant(mutant):
    rejected = 0
    for c in _case_set():
        rejected += any(not wc.same_bits(a, b) for a, b in zip(_views(c, None), _views(c, mutant)))
    assert rejected > 0, mutant


def test_needles_have_one_nonzero_output_and_reject_layout_mutants():
    N, K, M = 384, 1024, 17
    pts = wc.needle_points(N, K)
    assert len(pts) == 8 * 10 and (0, 0) in pts and (N - 1, K - 1) in pts
    for n, k in pts:
        c = wc.needle_case(N, K, M, n, k, 16)
        y = wc.ref_sum(c, 4)
        assert int((y != 0).sum()) == 1 and float(y[16, n]) == 3.0 * -1.5 * float(c.scale[n])
        slabs = wc.ref_slabs(c, 4)
        assert int((slabs[k // 256] != 0).sum()) == 1            # in the split that owns k*
    # a needle in k-block 0 / tile 0 moves under the layout mutants; a needle elsewhere does not
    c = wc.needle_case(N, K, M, 3, 5, 0)
    for mutant in ("kblock_swap", "tile_swap", "scale_next"):
        assert not wc.same_bits(wc.ref_sum(c), wc.ref_sum(c, mutant=mutant)), mutant
    c = wc.needle_case(N, K, M, 200, 700, 0)
    for mutant in ("kblock_swap", "tile_swap"):
        assert wc.same_bits(wc.ref_sum(c), wc.ref_sum(c, mutant=mutant)), mutant


def test_only_mixed_scales_see_the_scale_after_the_rounding():
    """A power of two commutes with a rounding: the mixed-scale grid is what rejects that mutant."""
    p2, mx = wc.grid_case(384, 1024, 17), wc.grid_case(384, 1024, 17, scales="mixed")
    assert wc.same_bits(wc.ref_bf16(p2), wc.ref_bf16(p2, mutant="scale_after_round"))
    assert not wc.same_bits(wc.ref_bf16(mx), wc.ref_bf16(mx, mutant="scale_after_round"))


def test_tiling_rules_are_the_bf16_ones():
    """The W8 ops import the bf16 tiling rules: same split, same n-block height, same NT rule."""
    assert gemm_w8.choose_split is gemm.choose_split and gemm_w8.partial_tiling is gemm.partial_tiling
    assert gemm_w8.down_kr is gemm.down_kr and gemm_w8.gate_up_split is gemm.gate_up_split
    small = gemm_w8.W8(torch.empty((4096, 4096), dtype=torch.uint8, device="meta"), torch.empty(4096), (4096, 4096))
    big = gemm_w8.W8(torch.empty((57344, 8192), dtype=torch.uint8, device="meta"), torch.empty(57344), (57344, 8192))
    assert gemm_w8._nt(small) == 0 and gemm_w8._nt(big) == gemm.NT_BIT
    assert gemm_w8.KERNEL_MAX_M == gemm.DECODE_MAX_M
