"""The W4 (weight-only MXFP4) kernels on the GPU: the decode GEMM in every instantiated mode against
the float64 reference (every nibble x every scale byte, position-coded scales, exact grid cases, NaN
sentinels), against the bf16 kernel of the same build where the epilogue is shared (row scale, SiLU),
random values within derived bounds, the widen kernel, the wide path, and a captured graph.  The
"equals the bf16 kernel" assertions rest on tests/kernels/test_gemm_exact.py, which pins that kernel
to float64.

tests/unit/test_gemm_w4_cases.py proves on the CPU that these inputs reject wrong kernels."""
import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_w4
from tests import gemm_w4_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def handle(c: wc.Case) -> gemm_w4.W4:
    return gemm_w4.W4.from_bytes(c.nib.to(DEV), c.xs.to(DEV))


def dequant_bf16(c: wc.Case):
    """The dequantised weight in bf16 (exact), row-major and block-packed, for the bf16 kernel."""
    w = wc.dequant64(c)
    wb = w.float().to(BF16)
    assert torch.equal(wb.double(), w)
    wb = wb.to(DEV)
    return wb, gemm.pack_weight(wb)


def splits(K: int):
    return [S for S in (1, 2, 4) if K % (256 * S) == 0]


def nan_ws(n: int) -> torch.Tensor:
    return torch.full((n + 64,), NAN, dtype=torch.float32, device=DEV)


def parts_for(M: int, nparts: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + M + nparts + seed)
    return (torch.rand((nparts, M), generator=g) * 300.0 + 1.0).to(DEV)


def check_bf16(c, h, x, nt=False):
    buf, out = wc.sentinel_out(c.M, c.N, DEV)
    if nt:
        gemm_w4._launch(gemm.MODE_BF16 | gemm.NT_BIT, x, h, 1, out=out)
    else:
        gemm_w4.linear(x, h, out=out)
    assert wc.outside_is_nan(buf, c.M, c.N) and wc.same_bits(out, wc.ref_bf16(c)), (c.name, nt)


def check_partial(c, h, x, S, half, want_slabs):
    M, N = c.M, c.N
    ws = nan_ws(S * M * N)
    p = gemm_w4.linear_partial(x, h, ws, S=S, half=half)
    assert (p.S, p.M, p.N) == (S, M, N)
    got = p.view().cpu()
    assert bool(ws[S * M * N:].isnan().all()) and not bool(got.isnan().any()), (c.name, S, half)
    assert wc.same_bits(got, want_slabs), (c.name, S, half)                   # every slab
    assert wc.same_bits(got.sum(0), want_slabs.sum(0)), (c.name, S, half)     # the slab sum (exact in fp32)
    # the existing reducer consumes the slabs unchanged
    assert wc.same_bits(gemm.reduce_partial(p), want_slabs.sum(0).float().to(BF16)), (c.name, S, half)


def test_every_nibble_times_every_scale_byte():
    """All 16 nibbles x every scale byte in [2, 252], one-hot activations of 1.0: the output is the
    weight itself, bit for bit -- the convert instruction's nibble order, its sign handling, its
    table and its whole scale range (2^-126 .. 6 * 2^125: every value a normal bf16 number).  Through
    the 64-row kernels (eight 64-row slices of the identity) and the 128-row one (all 512 rows)."""
    for rows in [slice(64 * i, 64 * i + 64) for i in range(8)] + [None]:
        c = wc.every_code_case(rows)
        h = handle(c)
        x = wc.sentinel_rows(c.x.to(DEV))
        want = wc.ref_sum(c)
        assert torch.equal(want.float().to(BF16).double(), want)
        check_bf16(c, h, x)
        check_partial(c, h, x, 2, False, wc.ref_slabs(c, 2))
    check_bf16(c, h, x, nt=True)  # (512 rows: the entry point drops the bit)
    c = wc.every_code_case(slice(448, 512))
    check_bf16(c, handle(c), wc.sentinel_rows(c.x.to(DEV)), nt=True)


def test_position_coded_scales():
    """Scale bytes that are a function of (row, k-block) with 16 distinct values, non-zero nibbles,
    one-hot activations at the edges of a word, a 16-byte load, a k-block, a k-step, a 256-deep LDS
    chunk and the splits: every output column carries its own block's scale."""
    c = wc.position_case()
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    w = wc.dequant64(c)
    check_bf16(c, h, x)
    check_bf16(c, h, x, nt=True)
    out = gemm_w4.linear(x, h).double().cpu()
    for m, k in enumerate(wc.position_kstars(c.K)):
        for n in wc.position_rows(c.N):
            assert float(out[m, n]) == float(w[n, k]), (n, k)
    for S in splits(c.K):
        for half in (False, True):
            check_partial(c, h, x, S, half, wc.ref_slabs(c, S))


@pytest.mark.parametrize("M", wc.ROWS)
@pytest.mark.parametrize("N,K", wc.SHAPES)
def test_grid_every_mode(N, K, M):
    """Grid inputs: bf16 out and the split-K slabs equal float64 bit for bit; the row-scaled slabs
    and the SiLU epilogues equal the bf16 kernel fed the dequantised weight bit for bit (the inputs
    are exact, so both kernels form the same acc and run the same epilogue).  Output and slab
    buffers are NaN-filled and larger than [M, N]; A's rows at and beyond M are NaN."""
    c = wc.grid_case(N, K, M)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    check_bf16(c, h, x)
    # the non-temporal instantiation (M <= 64; above, dispatch drops the bit for the row tiles)
    check_bf16(c, h, x, nt=True)
    # fp32 slabs: every split, 128- and 64-row n-blocks
    for S in splits(K):
        want = wc.ref_slabs(c, S)
        for half in (False, True):
            check_partial(c, h, x, S, half, want)
    # the shared epilogues against the bf16 kernel
    wb, wbp = dequant_bf16(c)
    buf, out = wc.sentinel_out(M, N // 2, DEV)
    ref_out = gemm.linear_silu(x, wb, packed=wbp, max_m=gemm.DECODE_MAX_M)
    gemm_w4._launch(gemm.MODE_SILU, x, h, 1, out=out)
    assert wc.outside_is_nan(buf, M, N // 2) and not bool(out.isnan().any())
    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), c.name
    buf, out = wc.sentinel_out(M, N // 2, DEV)
    gemm_w4._launch(gemm.MODE_SILU | gemm.NT_BIT, x, h, 1, out=out)
    assert wc.outside_is_nan(buf, M, N // 2)
    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, "NT")
    for nparts in (3, 20):
        rs = gemm.RowScale(parts_for(M, nparts), 1e-5)
        buf, out = wc.sentinel_out(M, N // 2, DEV)
        gemm_w4._launch(gemm.MODE_SILU, x, h, 1, out=out, rowscale=rs)
        ref_out = gemm.linear_silu(x, wb, packed=wbp, rowscale=rs)
        assert wc.outside_is_nan(buf, M, N // 2)
        assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, nparts)
        buf, out = wc.sentinel_out(M, N // 2, DEV)
        gemm_w4._launch(gemm.MODE_SILU | gemm.NT_BIT, x, h, 1, out=out, rowscale=rs)
        assert wc.outside_is_nan(buf, M, N // 2)
        assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, nparts, "NT")
        for S in splits(K):
            for half in (False, True):
                ws, ws2 = nan_ws(S * M * N), nan_ws(S * M * N)
                p = gemm_w4.linear_partial_rowscale(x, h, ws, rs, S=S, half=half)
                q = gemm.linear_partial_rowscale(x, wb, ws2, rs, S=S, packed=wbp, half=half)
                assert bool(ws[S * M * N:].isnan().all()) and not bool(p.view().isnan().any())
                assert torch.equal(p.view().view(torch.int32), q.view().view(torch.int32)), (c.name, nparts, S, half)


@pytest.mark.parametrize("M", [1, 64, 200])
def test_the_splits_the_ops_choose_at_the_real_width(M):
    """(1024, 14336), the 8B down projection's K: the tiling rules pick splits beyond 1, 2, 4 there
    (56 k-chunks: split 8, or 4 with 64-row n-blocks; 7-chunk k ranges, an odd count).  The
    slabs the ops produce when left to choose -- linear_partial with and without 64-row n-blocks, and
    linear_down, which the decode chain calls -- equal float64 bit for bit at the split they chose."""
    N, K = 1024, 14336
    c = wc.grid_case(N, K, M)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    chosen = set()
    for half in (False, True):
        S, _ = gemm.partial_tiling(N, K, M, h.packed, half)
        ws = nan_ws(S * M * N)
        p = gemm_w4.linear_partial(x, h, ws, half=half)
        assert p.S == S and bool(ws[S * M * N:].isnan().all())
        assert wc.same_bits(p.view(), wc.ref_slabs(c, S)), (M, S, half)
        assert wc.same_bits(gemm.reduce_partial(p), wc.ref_bf16(c)), (M, S, half)
        chosen.add(S)
    S = gemm.choose_split(N, K, M)
    ws = nan_ws(S * M * N)
    p = gemm_w4.linear_down(x, h, ws)
    assert p.S == S and bool(ws[S * M * N:].isnan().all())
    assert wc.same_bits(p.view(), wc.ref_slabs(c, S)), (M, S, "down")
    chosen.add(S)
    assert chosen == {8, 4}, chosen       # 8 is beyond what test_grid_every_mode sweeps
    # and every other split that divides the 56 k-chunks, set by hand
    for S in (7, 8, 14):
        for half in (False, True):
            check_partial(c, h, x, S, half, wc.ref_slabs(c, S))


# ------------------------------------------------------------------------------- random values
def bf16_bound(want: torch.Tensor, c: wc.Case) -> torch.Tensor:
    """|got - ref| <= 2^-8 |ref| + K 2^-23 sum_k |x||w|: one bf16 rounding (2^-9) and the fp32
    summation error (K 2^-24 of the absolute dot product), each with a factor-2 margin -- the bound
    of tests/kernels/test_gemm_w8.py (the weights are exact here too)."""
    return 2.0 ** -8 * want.abs() + c.K * 2.0 ** -23 * wc.abs_dot(c)


@pytest.mark.parametrize("M", [17, 200])
def test_random_values_within_derived_bounds(M):
    N, K = 384, 1024
    c = wc.random_case(N, K, M)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    want = wc.ref_sum(c)
    summ = c.K * 2.0 ** -23 * wc.abs_dot(c)
    got = gemm_w4.linear(x, h).double().cpu()
    assert bool(((got - want).abs() <= bf16_bound(want, c)).all())
    # slabs: fp32 sums (no bf16 rounding), then the reducer
    for half in (False, True):
        p = gemm_w4.linear_partial(x, h, nan_ws(4 * M * N), S=4, half=half)
        s = p.view().double().sum(0).cpu()
        assert bool(((s - want).abs() <= summ + 2.0 ** -22 * want.abs()).all())
        assert bool(((gemm.reduce_partial(p).double().cpu() - want).abs() <= bf16_bound(want, c)).all())
    # row scale: rinv is formed in fp32 from the parts (rsqrt: a few ulp), then one more fp32 product
    parts = parts_for(M, 3)
    rinv = torch.rsqrt(parts.double().cpu().sum(0) / K + 1e-5)
    p = gemm_w4.linear_partial_rowscale(x, h, nan_ws(4 * M * N), gemm.RowScale(parts, 1e-5), S=4)
    wr = want * rinv[:, None]
    assert bool(((p.view().double().sum(0).cpu() - wr).abs() <= (summ * rinv[:, None] + 2.0 ** -19 * wr.abs())).all())
    # SiLU-mul: the bound of tests/kernels/test_gemm_w8.py, derived there
    out = torch.empty((M, N // 2), dtype=BF16, device=DEV)
    gemm_w4._launch(gemm.MODE_SILU, x, h, 1, out=out)
    g, u = wc.split_gate_up(want)
    sg, su = wc.split_gate_up(summ)
    e_g, e_u = sg + 2.0 ** -8 * g.abs(), su + 2.0 ** -8 * u.abs()
    sil = g / (1.0 + torch.exp(-g))
    e_s = 1.1 * e_g + 2.0 ** -20 * sil.abs() + 2.0 ** -8 * (sil.abs() + 1.1 * e_g)
    e_p = e_s * u.abs() + e_u * sil.abs() + e_s * e_u
    bound = e_p + 2.0 ** -8 * ((sil * u).abs() + e_p)
    assert bool(((out.double().cpu() - sil * u).abs() <= bound).all())


# ------------------------------------------------------------------------------ prefill path
def test_widen_is_dequant_exactly():
    for c in (wc.every_code_case(slice(0, 1)), wc.position_case(384, 1024), wc.grid_case(128, 256, 1)):
        h = handle(c)
        N, K = c.N, c.K
        flat = torch.full((N * K + 64,), NAN, dtype=BF16, device=DEV)
        got = gemm_w4.widen(h, flat)
        want = h.dequant().cpu()
        assert torch.equal(want.double(), wc.dequant64(c))
        assert wc.same_bits(got, want) and bool(flat[N * K:].isnan().all()), c.name
        assert torch.equal(got.cpu().view(torch.int16) & 0x7fff, want.to(BF16).view(torch.int16) & 0x7fff)


def test_wide_path():
    """Above the kernel's row limit: widen into the scratch, library GEMM -- bit for bit the library
    GEMM on the dequantised weight (and, on the grid, float64)."""
    N, K, M = 384, 1024, 600
    assert M > gemm_w4.KERNEL_MAX_M
    for c in (wc.grid_case(N, K, M), wc.random_case(N, K, M)):
        h = handle(c)
        x = wc.sentinel_rows(c.x.to(DEV))
        got = gemm_w4.linear(x, h)
        wb, _ = dequant_bf16(c)
        want = torch.mm(x, wb.t())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), c.name
        h.scratch = torch.full((N * K + 64,), NAN, dtype=BF16, device=DEV)   # the model's shared scratch
        got = gemm_w4.linear(x, h)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool(h.scratch[N * K:].isnan().all())
    c = wc.grid_case(N, K, M)
    assert wc.same_bits(gemm_w4.linear(wc.sentinel_rows(c.x.to(DEV)), handle(c)), wc.ref_bf16(c))
    # a strided activation (a column slice) is not the kernel's: the wide path serves it
    c = wc.grid_case(N, K, 17)
    wide = torch.full((17 + 3, K + 8), NAN, dtype=BF16, device=DEV)
    wide[:17, 1:K + 1] = c.x.to(DEV)
    assert wc.same_bits(gemm_w4.linear(wide[:17, 1:K + 1], handle(c)), wc.ref_bf16(c))


def test_entry_point_rejects_what_it_does_not_tile():
    c = wc.grid_case(128, 256, 4)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    out = torch.empty((4, 128), dtype=BF16, device=DEV)
    from polykey_service_amd.ops import native
    for kw in (dict(S=2), dict(mode=gemm.MODE_BF16 | gemm.HALF_BIT), dict(mode=3), dict(mode=gemm.MODE_BF16 | 16)):
        with pytest.raises(native.KernelError):
            gemm_w4._launch(kw.get("mode", gemm.MODE_BF16), x, h, kw.get("S", 1), out=out)
    with pytest.raises(native.KernelError):  # K of the split not a multiple of 256
        gemm_w4._launch(gemm.MODE_PARTIAL, x, h, 2, ws=nan_ws(2 * 4 * 128))


def test_ops_take_the_non_temporal_kernels_by_the_byte_threshold(monkeypatch):
    """The ops set the non-temporal bit from gemm.NT_MIN_BYTES on the packed nibble bytes (read at
    the call, as the bf16 ops do)."""
    N, K, M = 384, 1024, 17
    sent = []
    real = gemm_w4.native.call

    def spy(name, *a):
        if name == "pk_w4_gemm":
            sent.append(a[11])
        return real(name, *a)
    monkeypatch.setattr(gemm_w4.native, "call", spy)
    c = wc.grid_case(N, K, M)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    base = gemm_w4.linear(x, h), gemm_w4.linear_silu(x, h)
    assert gemm_w4._nt(h) == 0 and not any(b & gemm.NT_BIT for b in sent)
    sent.clear()
    with monkeypatch.context() as mp:
        mp.setattr(gemm, "NT_MIN_BYTES", N * K // 2)
        assert gemm_w4._nt(h) == gemm.NT_BIT
        got = gemm_w4.linear(x, h), gemm_w4.linear_silu(x, h)
        mp.setattr(gemm, "NT_MIN_BYTES", N * K // 2 + 1)
        assert gemm_w4._nt(h) == 0
    assert sent == [gemm.MODE_BF16 | gemm.NT_BIT, gemm.MODE_SILU | gemm.NT_BIT], sent
    assert wc.same_bits(got[0], wc.ref_bf16(c)) and torch.equal(got[1].view(torch.int16), base[1].view(torch.int16))


def test_captured_graph_replays_after_the_activations_were_rewritten():
    N, K, M = 384, 1024, 17
    c, c2 = wc.grid_case(N, K, M), wc.grid_case(N, K, M, seed=1)
    h = handle(c)
    x = wc.sentinel_rows(c.x.to(DEV))
    out = torch.full((M, N), NAN, dtype=BF16, device=DEV)
    ws = nan_ws(4 * M * N)
    red = torch.full((M, N), NAN, dtype=BF16, device=DEV)

    def run():
        gemm_w4.linear(x, h, out=out)
        gemm.reduce_partial(gemm_w4.linear_partial(x, h, ws, S=4, half=True), out=red)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for acts in (c, c2, c):
        x.copy_(acts.x.to(DEV))
        want = wc.ref_bf16(wc.Case(acts.x, c.nib, c.xs))
        out.fill_(NAN)
        red.fill_(NAN)
        ws.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert wc.same_bits(out, want) and wc.same_bits(red, want)
    assert not wc.same_bits(wc.ref_bf16(c), wc.ref_bf16(wc.Case(c2.x, c.nib, c.xs)))
