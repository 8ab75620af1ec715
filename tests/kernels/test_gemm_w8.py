"""The W8 (weight-only FP8) kernels on the GPU: the decode GEMM in every instantiated mode against
the float64 reference (exact grid cases, needles, NaN sentinels), against the bf16 kernel of the
same build where the epilogue is shared (row scale, SiLU), random values within derived bounds,
the widen / column-scale kernels, the wide path, and a captured graph.  The "equals the bf16 kernel"
assertions rest on tests/kernels/test_gemm_exact.py, which pins that kernel to float64.

tests/unit/test_gemm_w8_cases.py proves on the CPU that these inputs reject wrong kernels."""
import functools

import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_w8
from tests import gemm_w8_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def handle(c: wc.Case) -> gemm_w8.W8:
    return gemm_w8.W8.from_bytes(c.b.view(torch.uint8).to(DEV), c.scale.to(DEV))


def dequant_bf16(c: wc.Case):
    """bf16(scale * widen(byte)) row-major and block-packed, for the bf16 kernel (exact: power-of-two scales)."""
    w = c.b.float() * c.scale[:, None]
    wb = w.to(BF16)
    assert torch.equal(wb.float(), w)
    wb = wb.to(DEV)
    return wb, gemm.pack_weight(wb)


def splits(K: int):
    return [S for S in (1, 2, 4) if K % (256 * S) == 0]


def nan_ws(n: int) -> torch.Tensor:
    return torch.full((n + 64,), NAN, dtype=torch.float32, device=DEV)


def parts_for(M: int, nparts: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + M + nparts + seed)
    return (torch.rand((nparts, M), generator=g) * 300.0 + 1.0).to(DEV)


def check_partial(c, h, x, S, half, want_slabs):
    M, N = c.M, c.N
    ws = nan_ws(S * M * N)
    p = gemm_w8.linear_partial(x, h, ws, S=S, half=half)
    assert (p.S, p.M, p.N) == (S, M, N)
    got = p.view().cpu()
    assert bool(ws[S * M * N:].isnan().all()) and not bool(got.isnan().any()), (c.name, S, half)
    assert wc.same_bits(got, want_slabs), (c.name, S, half)                   # every slab
    assert wc.same_bits(got.sum(0), want_slabs.sum(0)), (c.name, S, half)     # the slab sum (exact in fp32)
    # the existing reducer consumes the slabs unchanged
    assert wc.same_bits(gemm.reduce_partial(p), want_slabs.sum(0).float().to(BF16)), (c.name, S, half)


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
    # bf16 out
    buf, out = wc.sentinel_out(M, N, DEV)
    gemm_w8.linear(x, h, out=out)
    assert wc.outside_is_nan(buf, M, N) and wc.same_bits(out, wc.ref_bf16(c)), c.name
    # the non-temporal instantiation (M <= 64; above, dispatch drops the bit for the row tiles)
    buf, out = wc.sentinel_out(M, N, DEV)
    gemm_w8._launch(gemm.MODE_BF16 | gemm.NT_BIT, x, h, 1, out=out)
    assert wc.outside_is_nan(buf, M, N) and wc.same_bits(out, wc.ref_bf16(c)), (c.name, "NT")
    # fp32 slabs: every split, 128- and 64-row n-blocks
    for S in splits(K):
        want = wc.ref_slabs(c, S)
        for half in (False, True):
            check_partial(c, h, x, S, half, want)
    # the shared epilogues against the bf16 kernel
    wb, wbp = dequant_bf16(c)
    buf, out = wc.sentinel_out(M, N // 2, DEV)
    ref_out = gemm.linear_silu(x, wb, packed=wbp, max_m=gemm.DECODE_MAX_M)
    gemm_w8._launch(gemm.MODE_SILU, x, h, 1, out=out)
    assert wc.outside_is_nan(buf, M, N // 2) and not bool(out.isnan().any())
    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), c.name
    buf, out = wc.sentinel_out(M, N // 2, DEV)
    gemm_w8._launch(gemm.MODE_SILU | gemm.NT_BIT, x, h, 1, out=out)
    assert wc.outside_is_nan(buf, M, N // 2)
    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, "NT")
    for nparts in (3, 20):
        rs = gemm.RowScale(parts_for(M, nparts), 1e-5)
        buf, out = wc.sentinel_out(M, N // 2, DEV)
        gemm_w8._launch(gemm.MODE_SILU, x, h, 1, out=out, rowscale=rs)
        ref_out = gemm.linear_silu(x, wb, packed=wbp, rowscale=rs)
        assert wc.outside_is_nan(buf, M, N // 2)
        assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, nparts)
        buf, out = wc.sentinel_out(M, N // 2, DEV)
        gemm_w8._launch(gemm.MODE_SILU | gemm.NT_BIT, x, h, 1, out=out, rowscale=rs)
        assert wc.outside_is_nan(buf, M, N // 2)
        assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, nparts, "NT")
        for S in splits(K):
            for half in (False, True):
                ws, ws2 = nan_ws(S * M * N), nan_ws(S * M * N)
                p = gemm_w8.linear_partial_rowscale(x, h, ws, rs, S=S, half=half)
                q = gemm.linear_partial_rowscale(x, wb, ws2, rs, S=S, packed=wbp, half=half)
                assert bool(ws[S * M * N:].isnan().all()) and not bool(p.view().isnan().any())
                assert torch.equal(p.view().view(torch.int32), q.view().view(torch.int32)), (c.name, nparts, S, half)


@pytest.mark.parametrize("N,K", wc.SHAPES[:4])
def test_grid_mixed_scales(N, K):
    """Scales that are no powers of two (still exact in fp32): the scale is applied before the
    one bf16 rounding, in the kernel and in the reducer's input."""
    for M in (17, 200):
        c = wc.grid_case(N, K, M, scales="mixed")
        h = handle(c)
        x = wc.sentinel_rows(c.x.to(DEV))
        buf, out = wc.sentinel_out(M, N, DEV)
        gemm_w8.linear(x, h, out=out)
        assert wc.outside_is_nan(buf, M, N) and wc.same_bits(out, wc.ref_bf16(c)), c.name
        S = splits(K)[-1]
        check_partial(c, h, x, S, False, wc.ref_slabs(c, S))


@pytest.mark.parametrize("N,K", [(256, 512), (384, 1024)])
def test_needles(N, K):
    """One byte at (n*, k*), one activation at (m*, k*): exactly one output element, exact."""
    M = 17
    S = splits(K)[-1]
    for n, k in wc.needle_points(N, K):
        for m in (0, M - 1):
            c = wc.needle_case(N, K, M, n, k, m)
            h = handle(c)
            x = wc.sentinel_rows(c.x.to(DEV))
            want = wc.ref_sum(c)
            assert int((want != 0).sum()) == 1
            buf, out = wc.sentinel_out(M, N, DEV)
            gemm_w8.linear(x, h, out=out)
            assert wc.outside_is_nan(buf, M, N) and wc.same_bits(out, want), c.name
            for half in (False, True):
                check_partial(c, h, x, S, half, wc.ref_slabs(c, S))
            # non-temporal loads read the same bytes
            buf, out = wc.sentinel_out(M, N, DEV)
            gemm_w8._launch(gemm.MODE_BF16 | gemm.NT_BIT, x, h, 1, out=out)
            assert wc.outside_is_nan(buf, M, N) and wc.same_bits(out, want), (c.name, "NT")
            # the row scale, every split and n-block height: bit for bit the bf16 kernel on the
            # dequantised weight, and still exactly one non-zero element
            wb, wbp = dequant_bf16(c)
            rs = gemm.RowScale(parts_for(M, 3), 1e-5)
            for Sr in splits(K):
                for half in (False, True):
                    ws, ws2 = nan_ws(Sr * M * N), nan_ws(Sr * M * N)
                    p = gemm_w8.linear_partial_rowscale(x, h, ws, rs, S=Sr, half=half)
                    q = gemm.linear_partial_rowscale(x, wb, ws2, rs, S=Sr, packed=wbp, half=half)
                    assert torch.equal(p.view().view(torch.int32), q.view().view(torch.int32)), (c.name, Sr, half)
                    got = p.view().sum(0)
                    assert int((got != 0).sum()) == 1 and float(got[m, n]) != 0, (c.name, Sr, half)
            # SiLU (a lone gate or up byte: silu(gate) * up is zero everywhere), plain and non-temporal,
            # with and without the row scale: bit for bit the bf16 kernel
            for r in (None, rs):
                ref_out = gemm.linear_silu(x, wb, packed=wbp, rowscale=r, max_m=gemm.DECODE_MAX_M)
                for nt in (0, gemm.NT_BIT):
                    buf, out = wc.sentinel_out(M, N // 2, DEV)
                    gemm_w8._launch(gemm.MODE_SILU | nt, x, h, 1, out=out, rowscale=r)
                    assert wc.outside_is_nan(buf, M, N // 2) and bool((out == 0).all()), c.name
                    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (c.name, nt)


def test_needle_pairs_through_the_silu():
    """A gate byte and an up byte of the same column: one non-zero SiLU output, at column n / 2."""
    N, K, M = 384, 1024, 17
    for gate_row, k in ((0, 0), (15, 255), (128 + 5, 256), (N - 32, K - 1)):
        c = wc.needle_case(N, K, M, gate_row, k, M - 1, xv=2.0, wv=4.0)
        c.b = c.b.float()
        c.b[gate_row + 16, k] = -1.5
        c.b = c.b.to(wc.FP8)
        h = handle(c)
        buf, out = wc.sentinel_out(M, N // 2, DEV)
        gemm_w8._launch(gemm.MODE_SILU, wc.sentinel_rows(c.x.to(DEV)), h, 1, out=out)
        want = wc.ref_silu(c).double()
        col = (gate_row // 32) * 16 + gate_row % 16
        assert int((want != 0).sum()) == 1 and float(want[M - 1, col]) != 0
        got = out.double().cpu()
        assert wc.outside_is_nan(buf, M, N // 2) and int((got != 0).sum()) == 1 and float(got[M - 1, col]) != 0
        # one bf16 rounding of silu (2^-8 with the kernel's fast exp inside it) and one of the product
        assert abs(float(got[M - 1, col]) - float(want[M - 1, col])) <= 2.0 ** -7 * abs(float(want[M - 1, col]))
        # and bit for bit the bf16 kernel on the dequantised weight, non-temporal loads and row scale included
        wb, wbp = dequant_bf16(c)
        x = c.x.to(DEV)
        for r in (None, gemm.RowScale(parts_for(M, 3), 1e-5)):
            ref_out = gemm.linear_silu(x, wb, packed=wbp, rowscale=r, max_m=gemm.DECODE_MAX_M)
            for nt in (0, gemm.NT_BIT):
                o2 = torch.empty((M, N // 2), dtype=BF16, device=DEV)
                gemm_w8._launch(gemm.MODE_SILU | nt, x, h, 1, out=o2, rowscale=r)
                assert torch.equal(o2.view(torch.int16), ref_out.view(torch.int16)), (gate_row, k, nt)
                assert int((o2 != 0).sum()) == 1


# ------------------------------------------------------------------------------- random values
def bf16_bound(want: torch.Tensor, c: wc.Case) -> torch.Tensor:
    """|got - ref| <= 2^-8 |ref| + K 2^-23 scale[n] sum_k |x||w|: one bf16 rounding (2^-9) and the
    fp32 summation error (K 2^-24 of the absolute dot product), each with a factor-2 margin."""
    return 2.0 ** -8 * want.abs() + c.K * 2.0 ** -23 * wc.abs_dot(c)


@pytest.mark.parametrize("M", [17, 200])
def test_random_values_within_derived_bounds(M):
    N, K = 384, 1024
    c = wc.random_case(N, K, M)
    h = handle(c)
    x = c.x.to(DEV)
    want = wc.ref_sum(c)
    summ = c.K * 2.0 ** -23 * wc.abs_dot(c)
    # bf16 out
    got = gemm_w8.linear(x, h).double().cpu()
    assert bool(((got - want).abs() <= bf16_bound(want, c)).all())
    # slabs: fp32 sums (no bf16 rounding; the scale is one more fp32 rounding), then the reducer
    for half in (False, True):
        p = gemm_w8.linear_partial(x, h, nan_ws(4 * M * N), S=4, half=half)
        s = p.view().double().sum(0).cpu()
        assert bool(((s - want).abs() <= summ + 2.0 ** -22 * want.abs()).all())
        assert bool(((gemm.reduce_partial(p).double().cpu() - want).abs() <= bf16_bound(want, c)).all())
    # row scale: rinv is formed in fp32 from the parts (rsqrt: a few ulp), then one more fp32 product
    parts = parts_for(M, 3)
    rinv = torch.rsqrt(parts.double().cpu().sum(0) / K + 1e-5)
    p = gemm_w8.linear_partial_rowscale(x, h, nan_ws(4 * M * N), gemm.RowScale(parts, 1e-5), S=4)
    wr = want * rinv[:, None]
    assert bool(((p.view().double().sum(0).cpu() - wr).abs() <= (summ * rinv[:, None] + 2.0 ** -19 * wr.abs())).all())
    # SiLU-mul.  gate, up: computed values within e = summ + 2^-8 |.| of the reference (as above).
    # silu is 1.1-Lipschitz, the kernel's fast exp adds 2^-20 relative, then one bf16 rounding:
    #   e_s = 1.1 e_g + 2^-20 |silu g| + 2^-8 (|silu g| + 1.1 e_g)
    # the product of the two rounded values, then the final rounding:
    #   e_p = e_s |u| + e_u |silu g| + e_s e_u;   bound = e_p + 2^-8 (|silu g * u| + e_p)
    out = torch.empty((M, N // 2), dtype=BF16, device=DEV)
    gemm_w8._launch(gemm.MODE_SILU, x, h, 1, out=out)
    g, u = wc.split_gate_up(want)
    sg, su = wc.split_gate_up(summ)
    e_g, e_u = sg + 2.0 ** -8 * g.abs(), su + 2.0 ** -8 * u.abs()
    sil = g / (1.0 + torch.exp(-g))
    e_s = 1.1 * e_g + 2.0 ** -20 * sil.abs() + 2.0 ** -8 * (sil.abs() + 1.1 * e_g)
    e_p = e_s * u.abs() + e_u * sil.abs() + e_s * e_u
    bound = e_p + 2.0 ** -8 * ((sil * u).abs() + e_p)
    assert bool(((out.double().cpu() - sil * u).abs() <= bound).all())


# ------------------------------------------------------------------------------ prefill path
def all_bytes_case(N: int, K: int) -> wc.Case:
    """Every finite e4m3 byte, in an order that puts different bytes at every layout position."""
    idx = (torch.arange(N * K, dtype=torch.int64) * 131 + torch.arange(N * K, dtype=torch.int64) // K) % 256
    byte = torch.where((idx & 0x7F) == 0x7F, idx & 0x80, idx).to(torch.uint8).view(N, K)
    return wc.Case(torch.zeros((1, K), dtype=BF16), byte.view(wc.FP8), wc.channel_scales(N), "all-bytes")


@pytest.mark.parametrize("N,K", [(128, 256), (384, 1024)])
def test_widen_is_the_cpu_widen_exactly(N, K):
    c = all_bytes_case(N, K)
    h = handle(c)
    flat = torch.full((N * K + 64,), NAN, dtype=BF16, device=DEV)
    got = gemm_w8.widen(h, flat)
    want = gemm_w8.unpack_w8(h.packed.cpu()).view(wc.FP8).to(BF16)
    assert torch.equal(want.float(), c.b.float())
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and bool(flat[N * K:].isnan().all())


@pytest.mark.parametrize("M,N", [(1, 128), (37, 384), (600, 1024)])
def test_col_scale_is_the_fp32_formula_exactly(M, N):
    g = torch.Generator().manual_seed(M + N)
    y = (torch.randn((M, N), generator=g) * 50).to(BF16)
    scale = (torch.rand(N, generator=g) * 3 + 2.0 ** -9).float()
    buf, out = wc.sentinel_out(M, N, DEV)
    out.copy_(y)
    gemm_w8.col_scale(out, scale.to(DEV))
    want = (y.float() * scale[None, :]).to(BF16)
    assert wc.outside_is_nan(buf, M, N) and torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_wide_path():
    """Above the kernel's row limit: widen into the scratch, library GEMM, column scale.  On the
    grid the GEMM's bf16 rounding commutes with the power-of-two scale: bit-exact.  On random
    values it rounds twice: 2^-7 |ref| plus the summation term."""
    N, K, M = 384, 1024, 600
    assert M > gemm_w8.KERNEL_MAX_M
    c = wc.grid_case(N, K, M)
    got = gemm_w8.linear(c.x.to(DEV), handle(c))
    assert wc.same_bits(got, wc.ref_bf16(c))
    c = wc.random_case(N, K, M)
    got = gemm_w8.linear(c.x.to(DEV), handle(c)).double().cpu()
    want = wc.ref_sum(c)
    assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + c.K * 2.0 ** -23 * wc.abs_dot(c)).all())
    # a strided activation (a column slice) is not the kernel's: the wide path serves it
    c = wc.grid_case(N, K, 17)
    wide = torch.zeros((17, K + 8), dtype=BF16, device=DEV)
    wide[:, 1:K + 1] = c.x.to(DEV)
    assert wc.same_bits(gemm_w8.linear(wide[:, 1:K + 1], handle(c)), wc.ref_bf16(c))


def test_entry_point_rejects_what_it_does_not_tile():
    c = wc.grid_case(128, 256, 4)
    h = handle(c)
    x = c.x.to(DEV)
    out = torch.empty((4, 128), dtype=BF16, device=DEV)
    from polykey_service_amd.ops import native
    for kw in (dict(S=2), dict(mode=gemm.MODE_BF16 | gemm.HALF_BIT), dict(mode=3), dict(mode=gemm.MODE_BF16 | 16)):
        with pytest.raises(native.KernelError):
            gemm_w8._launch(kw.get("mode", gemm.MODE_BF16), x, h, kw.get("S", 1), out=out)
    with pytest.raises(native.KernelError):  # K of the split not a multiple of 256
        gemm_w8._launch(gemm.MODE_PARTIAL, x, h, 2, ws=nan_ws(2 * 4 * 128))


def test_ops_take_the_non_temporal_kernels_by_the_byte_threshold(monkeypatch):
    """The ops set the non-temporal bit from gemm.NT_MIN_BYTES (read at the call, as the bf16 ops
    do): with the threshold lowered, linear and linear_silu launch the NT kernels, to the same bits;
    above 64 rows the entry point drops the bit, to the same bits again."""
    N, K = 384, 1024
    sent = []
    real = gemm_w8.native.call

    def spy(name, *a):
        if name == "pk_w8_gemm":
            sent.append(a[11])
        return real(name, *a)
    monkeypatch.setattr(gemm_w8.native, "call", spy)
    for M in (17, 64, 200):
        c = wc.grid_case(N, K, M)
        h = handle(c)
        x = c.x.to(DEV)
        base = gemm_w8.linear(x, h), gemm_w8.linear_silu(x, h)
        assert gemm_w8._nt(h) == 0 and not any(b & gemm.NT_BIT for b in sent)
        sent.clear()
        with monkeypatch.context() as mp:
            mp.setattr(gemm, "NT_MIN_BYTES", 1 << 10)
            assert gemm_w8._nt(h) == gemm.NT_BIT
            got = gemm_w8.linear(x, h), gemm_w8.linear_silu(x, h)
        assert sent == [gemm.MODE_BF16 | gemm.NT_BIT, gemm.MODE_SILU | gemm.NT_BIT], sent
        sent.clear()
        assert wc.same_bits(got[0], wc.ref_bf16(c)) and torch.equal(got[0].view(torch.int16), base[0].view(torch.int16))
        assert torch.equal(got[1].view(torch.int16), base[1].view(torch.int16)), M


def test_captured_graph_replays_to_the_same_bits():
    N, K, M = 384, 1024, 17
    c = wc.grid_case(N, K, M)
    h = handle(c)
    x = c.x.to(DEV)
    out = torch.full((M, N), NAN, dtype=BF16, device=DEV)
    ws = nan_ws(4 * M * N)
    red = torch.full((M, N), NAN, dtype=BF16, device=DEV)

    def run():
        gemm_w8.linear(x, h, out=out)
        gemm.reduce_partial(gemm_w8.linear_partial(x, h, ws, S=4, half=True), out=red)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    want = wc.ref_bf16(c)
    for _ in range(3):
        out.fill_(NAN)
        red.fill_(NAN)
        ws.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert wc.same_bits(out, want) and wc.same_bits(red, want)
