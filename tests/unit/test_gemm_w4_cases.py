"""The W4 (weight-only MXFP4) GEMM on the CPU: the packed layout round trip and its documented
positions, the quantiser against a brute-force float64 search, the interchange layout against
Hugging Face's dequantiser, the fp32 reference op against the float64 reference, and -- this
repository's convention -- proof that the inputs the GPU tests use can fail: the case set rejects
every mutant reference."""
import math

import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_w4
from polykey_service_amd.ops import reference as ref
from tests import gemm_w4_cases as wc


# --------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [256, 1024])
def test_pack_unpack_round_trip(N, K):
    g = torch.Generator().manual_seed(N + K)
    nib = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    xs = torch.randint(2, 253, (N, K // 32), generator=g, dtype=torch.uint8)
    p, x = gemm_w4.pack_w4(nib, xs)
    assert p.shape == nib.shape and x.shape == xs.shape and p.dtype == x.dtype == torch.uint8
    assert not torch.equal(p, nib) and not torch.equal(x, xs)
    n2, x2 = gemm_w4.unpack_w4(p, x)
    assert torch.equal(n2, nib) and torch.equal(x2, xs)
    assert torch.equal(torch.sort(p.view(-1)).values, torch.sort(nib.view(-1)).values)  # permutations
    assert torch.equal(torch.sort(x.view(-1)).values, torch.sort(xs.view(-1)).values)
    h = gemm_w4.W4.from_bytes(nib, xs)
    assert h.shape == (N, K) and h.nbytes == N * K // 2 + N * K // 32
    assert all(torch.equal(a, b) for a, b in zip(h.bytes_rowmajor(), (nib, xs)))


def test_packed_layout_is_the_one_the_kernel_reads():
    """Element (n, k) sits where the kernel's lane address finds it: n-block, 128-deep k-step, 16-row
    tile, lane 16 g + r, word s, byte b, nibble; its scale in byte s of word (n-block, k-step, tile, r)."""
    N, K = 256, 512
    codes = (torch.arange(N * K, dtype=torch.int64) * 7 // 3 % 16).view(N, K)
    xs = (2 + torch.arange(N * K // 32, dtype=torch.int64) % 251).to(torch.uint8).view(N, K // 32)
    p, x = gemm_w4.pack_w4(wc.pack_nibbles(codes), xs)
    p, x = p.view(-1), x.view(-1)
    for n, k in [(0, 0), (0, 1), (15, 7), (16, 8), (127, 31), (128, 32), (143, 127), (200, 128), (255, 511), (77, 300),
                 (1, 33), (130, 97)]:
        nb, tile, r = n // 128, (n % 128) // 16, n % 16
        ks, kk = k // 128, k % 128
        s, g, e = kk // 32, (kk % 32) // 8, kk % 8
        b, hi = e // 2, e % 2
        off = nb * 64 * K + ks * 8192 + tile * 1024 + (16 * g + r) * 16 + s * 4 + b
        assert (int(p[off]) >> (4 * hi)) & 15 == int(codes[n, k]), (n, k)
        word = ((nb * (K // 128) + ks) * 8 + tile) * 16 + r
        assert int(x[4 * word + s]) == int(xs[n, k // 32]), (n, k)


def test_pack_and_handle_reject_what_the_kernel_does_not_take():
    for shape in ((64, 256), (128, 128), (192, 256), (128, 384)):
        with pytest.raises(AssertionError):
            gemm_w4.pack_w4(torch.zeros((shape[0], shape[1] // 2), dtype=torch.uint8),
                            torch.full((shape[0], shape[1] // 32), 127, dtype=torch.uint8))
    nib = torch.zeros((128, 128), dtype=torch.uint8)
    for bad in (0, 1, 253, 254, 255):  # 255 is NaN in e8m0; the others leave bf16's normal range
        xs = torch.full((128, 8), 127, dtype=torch.uint8)
        xs[5, 3] = bad
        with pytest.raises(ValueError, match="scale bytes"):
            gemm_w4.W4.from_bytes(nib, xs)
    for ok in (2, 252):
        xs = torch.full((128, 8), ok, dtype=torch.uint8)
        d = gemm_w4.W4.from_bytes(torch.full((128, 128), 0x71, dtype=torch.uint8), xs).dequant()
        assert torch.equal(d.to(torch.bfloat16).float(), d) and bool((d.abs() >= 2.0 ** -126).all())  # normal bf16


# ------------------------------------------------------------------------------------- quantiser
MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def brute_force(block):
    """The OCP MX v1.0 rule for one block of 32 python floats (float64): (scale byte, 32 codes)."""
    amax = max(abs(v) for v in block)
    if amax == 0:
        X = 127
    else:
        m, e = math.frexp(amax)  # amax = m 2^e, 0.5 <= m < 1
        X = min(max(e - 1 - 2 + 127, 2), 252)
    codes = []
    for v in block:
        q = abs(v) * 2.0 ** (127 - X)  # exact: a power of two
        q = min(q, 8.0)                # (beyond 8 the nearest value is 6 all the same; keeps q - mag exact)
        best = None
        for code, mag in enumerate(MAGS):
            d = abs(q - mag)
            if best is None or d < best[0] or (d == best[0] and code % 2 == 0):
                best = (d, code)
        codes.append(best[1] + (8 if v < 0 and best[1] > 0 else 0))
    return X, codes


def check_blocks(w: torch.Tensor):
    nib, xs = ref.quantize_mxfp4_rows(w)
    codes = wc.codes_of(nib)
    for n in range(w.shape[0]):
        for kb in range(w.shape[1] // 32):
            X, want = brute_force([float(v) for v in w[n, 32 * kb:32 * kb + 32].double()])
            assert int(xs[n, kb]) == X, (n, kb, int(xs[n, kb]), X)
            assert codes[n, 32 * kb:32 * kb + 32].tolist() == want, (n, kb)
    return codes, xs


def test_quantiser_against_brute_force_on_every_tie_point():
    """Blocks whose amax is 4 * 2^e (scale 2^e): every tie point of the e2m1 grid, its two fp32
    neighbours and both signs; ties go to the even code."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    pos = []
    for t in ties:
        t32 = torch.tensor(t, dtype=torch.float32)
        lo, hi = torch.nextafter(t32, torch.tensor(0.0)), torch.nextafter(t32, torch.tensor(9.0))
        pos += [t, float(lo), float(hi)]
    assert len(pos) == 21
    rows = []
    for e in (-20, -3, 0, 5, 30):
        for chunk in (pos, [-v for v in pos]):
            rows.append(torch.tensor([4.0] + chunk + [0.0] * 10, dtype=torch.float32) * 2.0 ** e)
    w = torch.stack(rows)
    w = torch.cat([w] * 8, dim=1)  # [10, 256]
    codes, xs = check_blocks(w)
    assert xs[:, 0].tolist() == [107, 107, 124, 124, 127, 127, 132, 132, 157, 157]
    # spelled out: 0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, 1.75 -> 2.0, 2.5 -> 2.0, 3.5 -> 4.0, 5.0 -> 4.0
    assert [codes[4, 1 + 3 * i].item() for i in range(7)] == [0, 2, 2, 4, 4, 6, 6]
    assert [codes[5, 1 + 3 * i].item() for i in range(7)] == [0, 10, 10, 12, 12, 14, 14]   # (no negative zero)
    # and their neighbours fall to either side
    assert [codes[4, 2 + 3 * i].item() for i in range(7)] == [0, 1, 2, 3, 4, 5, 6]
    assert [codes[4, 3 + 3 * i].item() for i in range(7)] == [1, 2, 3, 4, 5, 6, 7]


def test_quantiser_scale_on_both_sides_of_every_power_of_two():
    """amax just below, at and just above 2^j for EVERY fp32 power of two, the subnormal ones included
    (j = -149 .. 127; below 2^-149 lies zero: an all-zero block), against the brute-force rule."""
    js = list(range(-149, 128))
    rows = []
    for j in js:
        p = torch.tensor(2.0 ** j, dtype=torch.float32)
        assert float(p) == 2.0 ** j
        below, above = torch.nextafter(p, torch.tensor(0.0)), torch.nextafter(p, torch.tensor(float("inf")))
        for amax in (below, p, above):
            rows.append(torch.linspace(-1.0, 1.0, 32, dtype=torch.float32) * amax)
    w = torch.stack(rows)
    w = torch.cat([w, w.flip(1), w * 0.5, -w], dim=1)  # [831, 128]
    codes, xs = check_blocks(w)
    i0 = 3 * js.index(0)
    assert xs[i0:i0 + 3, 0].tolist() == [124, 125, 125]            # amax just below 1 | 1 | just above 1
    # every exponent: X = j - 2 + 127 at and above 2^j, one less just below it, clamped into [2, 252]
    for i, j in enumerate(js):
        want = [min(max(j - 1 - 2 + 127, 2), 252)] + [min(max(j - 2 + 127, 2), 252)] * 2
        if j == -149:
            want[0] = 127                                            # the all-zero block
        assert xs[3 * i:3 * i + 3, 0].tolist() == want, j
    assert int(xs.min()) == 2 and int(xs.max()) == 252             # clamped at the low end, 2^127 reaches 252


def test_quantiser_saturation_zero_blocks_and_the_scale_clamp():
    w = torch.zeros((4, 256), dtype=torch.float64)
    # (6, 8) saturates: amax 7.75 gives scale 1, quotients 6.5, 7, 7.75 -> 6
    w[0, :6] = torch.tensor([7.75, 6.5, 7.0, -7.75, -6.5, 6.0], dtype=torch.float64)
    # block 1 of row 0 stays all zero: X = 127, nibbles 0
    # the clamp at the low end: amax 2^-140 (raw X = -15) -> X = 2, every quotient rounds to 0 or 0.5
    w[1, :3] = torch.tensor([2.0 ** -140, 2.0 ** -127, -(2.0 ** -126)], dtype=torch.float64)
    # the clamp at the high end: amax 2^200 (raw X = 325) -> X = 252, quotients saturate
    w[2, :4] = torch.tensor([2.0 ** 200, -(2.0 ** 130), 2.0 ** 125, 2.0 ** 124], dtype=torch.float64)
    codes, xs = check_blocks(w)
    assert int(xs[0, 0]) == 127 and codes[0, :6].tolist() == [7, 7, 7, 15, 15, 7]
    assert int(xs[0, 1]) == 127 and int(codes[0, 32:64].max()) == 0 and int(xs[3].min()) == int(xs[3].max()) == 127
    # (2^-127 = 0.25 * 2^-125 is the tie between 0 and 0.5: to the even code, 0)
    assert int(xs[1, 0]) == 2 and codes[1, :3].tolist() == [0, 0, 9]
    assert int(xs[2, 0]) == 252 and codes[2, :4].tolist() == [7, 15, 2, 1]
    # bf16 weights (the model's): the handle holds what the quantiser returns, dequant() is its value
    g = torch.Generator().manual_seed(5)
    wb = (torch.randn((128, 256), generator=g) * torch.logspace(-3, 2, 128)[:, None]).to(torch.bfloat16)
    wb[7] = 0
    h = gemm_w4.W4.from_weight(wb)
    nib, xq = ref.quantize_mxfp4_rows(wb)
    assert all(torch.equal(a, b) for a, b in zip(h.bytes_rowmajor(), (nib, xq)))
    c = wc.Case(torch.zeros((1, 256), dtype=torch.bfloat16), nib, xq)
    assert torch.equal(h.dequant().double(), wc.dequant64(c)) and h.dequant().dtype == torch.float32
    assert torch.equal(ref.dequantize_mxfp4(nib, xq, torch.float64), wc.dequant64(c))
    # error bound of the rule: the scale s = 2^(X - 127) lies in (amax / 8, amax / 4].  Unsaturated, the
    # error is at most half the largest grid step, 1 * s <= amax / 4; saturated, q = w / s in (6, 8)
    # loses (q - 6) s = |w| (1 - 6 / q) < amax / 4
    amax = wb.double().view(128, 8, 32).abs().amax(-1, keepdim=True)
    err = (wc.dequant64(c) - wb.double()).view(128, 8, 32).abs()
    assert bool((err <= amax / 4 + 1e-300).all())


def test_dequant_equals_the_hugging_face_dequantiser():
    """The interchange layout is the one ``transformers.integrations.mxfp4`` reads: its table, and
    ``convert_moe_packed_tensors`` (blocks [E, N, K/32, 16], scales [E, N, K/32]; its result is
    transposed to [E, K, N])."""
    mx = pytest.importorskip("transformers.integrations.mxfp4")
    assert [float(v) for v in mx.FP4_VALUES] == wc.E2M1 and [math.copysign(1, v) for v in mx.FP4_VALUES] == \
        [math.copysign(1, v) for v in wc.E2M1]
    c = wc.random_case(128, 256, 1)
    h = gemm_w4.W4.from_bytes(c.nib, c.xs)
    nib, xs = h.bytes_rowmajor()
    out = mx.convert_moe_packed_tensors(nib.view(1, 128, 8, 16), xs.view(1, 128, 8), dtype=torch.float32)
    assert out.shape == (1, 256, 128)
    assert torch.equal(out[0].t().contiguous(), h.dequant())


# --------------------------------------------------------------------------- fp32 reference op
@pytest.mark.parametrize("N,K", [(128, 256), (384, 1024), (256, 14336)])
def test_fp32_reference_is_exact_on_the_grid(N, K):
    c = wc.grid_case(N, K, 17)
    assert torch.equal(ref.w4_linear(c.x, c.nib, c.xs).double(), wc.ref_sum(c))
    assert torch.equal(ref.w4_linear(c.x, c.nib, c.xs, dtype=torch.float64), wc.ref_sum(c))
    rinv = torch.pow(2.0, -(torch.arange(17) % 5).float())
    assert torch.equal(ref.w4_linear(c.x, c.nib, c.xs, rinv).double(), wc.ref_sum(c, rinv=rinv))
    # the CPU ops are that reference plus the epilogue
    h = gemm_w4.W4.from_bytes(c.nib, c.xs)
    assert wc.same_bits(gemm_w4.linear(c.x, h), wc.ref_bf16(c))
    ws = torch.empty(16 * 17 * N)  # room for the largest split the GPU tiling could pick
    assert wc.same_bits(gemm_w4.linear_partial(c.x, h, ws).view().sum(0), wc.ref_sum(c))
    # SiLU: gate and up are exact, fp32 silu is not float64 silu (see tests/unit/test_gemm_w8_cases.py)
    got, want = gemm_w4.linear_silu(c.x, h).double(), wc.ref_silu(c).double()
    gate, up = (t.abs() for t in wc.split_gate_up(wc.ref_sum(c)))
    assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 2.0 ** -126 * (1 + gate) * (1 + up)).all())
    assert wc.same_bits(gemm_w4.widen(h), wc.dequant64(c)) and gemm_w4.widen(h).dtype == torch.bfloat16


def test_grid_exactness_figure():
    """max |sum| / quantum of the grid cases, from the data: below 2^24 with the narrower scale range
    at K = 14336, and the K <= 1024 range would NOT do there."""
    for N, K in wc.SHAPES:
        c = wc.grid_case(N, K, 200 if K <= 1024 else 17)
        assert wc.exactness(c) < 2.0 ** 24 and int(c.xs.max()) - int(c.xs.min()) == (7 if K <= 1024 else 3)
    c = wc.grid_case(256, 14336, 17)
    assert 48 * 14336 * 2 ** 7 > 2 ** 24   # the worst case of 8 scales at this K is not covered


def test_random_case_reference_within_its_bound():
    """The fp32 op against float64 on random values, within the bound the GPU tests use."""
    c = wc.random_case(384, 1024, 17)
    got = ref.w4_linear(c.x, c.nib, c.xs).to(torch.bfloat16).double()
    want = wc.ref_sum(c)
    bound = 2.0 ** -8 * want.abs() + c.K * 2.0 ** -23 * wc.abs_dot(c)
    assert bool(((got - want).abs() <= bound).all())


# --------------------------------------------------------------------------------------- mutants
def _case_set():
    """What the GPU tests run, at the sizes that keep this CPU test quick."""
    cases = [wc.grid_case(N, K, M) for (N, K) in wc.SHAPES[:4] for M in (1, 17)]
    cases += [wc.every_code_case(slice(0, 64)), wc.position_case()]
    return cases


def _views(c, mutant):
    """Every output the GPU tests compare, for one reference (mutant or not)."""
    S = 4 if c.K % 1024 == 0 else 2
    return [wc.ref_bf16(c, mutant=mutant), wc.ref_slabs(c, S, mutant=mutant), wc.ref_bf16(c, S, mutant=mutant),
            wc.ref_silu(c, mutant=mutant)]


@pytest.mark.parametrize("mutant", wc.MUTANTS)
def test_the_case_set_rejects_each_mutant(mutant):
    rejected = [c.name for c in _case_set()
                if any(not wc.same_bits(a, b) for a, b in zip(_views(c, None), _views(c, mutant)))]
    assert rejected, mutant
    # the grids alone reject every mutant too
    assert any(n.startswith("grid") for n in rejected), (mutant, rejected)


def test_every_code_and_position_cases_cover_what_they_claim():
    c = wc.every_code_case()
    codes = wc.codes_of(c.nib).view(256, 16, 32)
    pairs = {(int(x), int(v)) for n in range(256) for kb in range(16)
             for x in [c.xs[n, kb]] for v in codes[n, kb].unique()}
    assert pairs == {(x, v) for x in range(2, 253) for v in range(16)}
    want = wc.ref_sum(c)                                  # y[m, n] = w[n, m]: every weight, once
    assert torch.equal(want, wc.dequant64(c).t()) and torch.equal(want.float().to(torch.bfloat16).double(), want)
    assert float(want.abs().max()) == 6 * 2.0 ** 125 and float(want[want != 0].abs().min()) == 2.0 ** -126
    p = wc.position_case()
    assert len(p.xs.unique()) == 16 and not bool((wc.codes_of(p.nib) % 8 == 0).any())
    ks = wc.position_kstars(p.K)
    assert {0, 7, 8, 31, 32, 127, 128, 255, 256, 511, 512, 767, 768, 1023} <= set(ks) and p.M == len(ks)
    assert {0, 15, 16, 127, 128, 255} <= set(wc.position_rows(p.N))
    y = wc.ref_sum(p)
    for m, k in enumerate(ks):                            # every column carries its own block's scale
        assert torch.equal(y[m], wc.dequant64(p)[:, k])
        for mutant in ("scale_next_kblock", "scale_next_row", "scale_next_kstep"):
            assert not torch.equal(wc.ref_sum(p, mutant=mutant)[m], y[m]), (mutant, k)


def test_tiling_rules_are_the_bf16_ones():
    """The W4 ops import the bf16 tiling rules: same split, same n-block height; the NT rule counts
    the packed nibble bytes."""
    assert gemm_w4.choose_split is gemm.choose_split and gemm_w4.partial_tiling is gemm.partial_tiling
    assert gemm_w4.down_kr is gemm.down_kr and gemm_w4.gate_up_split is gemm.gate_up_split

    def meta(N, K):
        return gemm_w4.W4(torch.empty((N, K // 2), dtype=torch.uint8, device="meta"),
                          torch.empty((N, K // 32), dtype=torch.uint8, device="meta"), (N, K))
    assert gemm_w4._nt(meta(28672, 4096)) == 0 and gemm_w4._nt(meta(57344, 8192)) == gemm.NT_BIT
    assert gemm_w4.KERNEL_MAX_M == gemm.DECODE_MAX_M
