"""The dense bf16 GEMMs and their split-K consumers against float64, in every mode.

tests/gemm_cases.py builds the inputs (integer grids that are exact in fp32 in any summation order,
needles at the corners of the tilings, NaN sentinels around everything a kernel may write), the
float64 references with the documented roundings, and the criteria: bit-exact wherever the
arithmetic is exact, and an interval criterion derived from the fp32 operation count where it is
not (row scale, SiLU, the sums of squares of large residuals).  No element is exempt.
tests/unit/test_gemm_cases.py shows on the CPU that every wrong reference (swapped k-blocks,
k-steps, chunks, row tiles or half blocks, a lost or shifted split, a leaking row, a wrong gate / up
pairing, one rounding instead of two, parts of the wrong residual or row, a wrong rinv, a shifted
norm weight, every RoPE / cache slip) fails them.

Derived bounds and the largest observed ``|got - ref| / (delta |ref|)`` on MI355X per family (the
observed value is a record; the bound is the derived one, u = 2^-24):

    family                                      delta                  largest observed ratio
    row scale, fp32 slabs                       5 u                    0.54
    "rounding"-class parts, 128 / 64 columns    n u  (n = 128, 64)     0.036
    "rounding"-class parts, 512 columns         512 u                  0.0036
    SiLU (bf16 output, interval criterion)      (8 + 2 |g|) u          40196 of 11550272 outputs differ
                                                                       from the delta = 0 reference
    fused MLP slabs (one element of h each)     the interval of h      all inside

The SiLU error is only visible after the bf16 rounding, so its record is the number of outputs that
differ from the float64 reference evaluated without any slack (0.35 %, every one inside its interval).
``pytest -s`` prints the running figures as RECORD lines.
"""
import functools

import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm, gemm_prefill, reference
from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
I32 = torch.int32
ALL_ROWS = gc.ROWS + gc.ROWS_TILED
D = gemm.DECODE_MAX_M

grid = functools.lru_cache(maxsize=None)(gc.grid_case)
silu_grid = functools.lru_cache(maxsize=None)(gc.silu_case)

RECORD = {"rowscale": 0.0, "parts": 0.0, "parts512": 0.0, "silu_off": 0, "silu_n": 0}


def record(key, value):
    RECORD[key] = max(RECORD[key], value)
    print(f"RECORD {key} {RECORD[key]:.4g}")


def dev_x(c: gc.Case) -> torch.Tensor:
    """A on the device: row stride K + 8, NaN rows at and beyond M."""
    return gc.sentinel_rows(c.x.to(DEV))


def weights(c: gc.Case, packed: bool):
    w = c.w.to(DEV)
    return w, (gemm.pack_weight(w) if packed else None)


def dev_parts(parts: torch.Tensor) -> torch.Tensor:
    """[nparts, M] parts at the head of a NaN buffer."""
    buf = gc.sentinel_flat(parts.numel(), DEV)
    buf[: parts.numel()] = parts.reshape(-1).to(DEV)
    return buf[: parts.numel()].view(parts.shape)


def silu_mid(acc):
    """The float64 reference without any slack (gates below the __expf overflow give 0)."""
    g, u = gc.split_gate_up(acc)
    s = gc.silu64(gc.bf(g))
    s = torch.where(s.abs() < gc.SILU_ABS, torch.zeros_like(s), s)
    return gc.bf(gc.bf(s) * gc.bf(u))


def check_silu(out, acc, err=0.0, what=""):
    iv = gc.ref_silu(acc, err)
    assert gc.inside(out, iv), what
    off = int((out.double().cpu() != silu_mid(acc)).sum())
    RECORD["silu_off"] += off
    RECORD["silu_n"] += out.numel()
    print(f"RECORD silu_off {RECORD['silu_off']} of {RECORD['silu_n']}")


# ------------------------------------------------------------------------------ decode GEMM, bf16 out
@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_bf16(N, K, monkeypatch):
    """bf16 out: row-major W, packed W (the 64-row n-blocks the wrapper picks below 192 n-blocks),
    packed W as 128-row n-blocks, and both with the non-temporal bit."""
    for M in ALL_ROWS:
        c = grid(N, K, M)
        want = gc.expect_buf(gc.ref_bf16(c))
        x = dev_x(c)
        for packed, half, nt in ((False, False, False), (True, True, False), (True, False, False),
                                 (True, True, True), (True, False, True)):
            with monkeypatch.context() as mp:
                mp.setattr(gemm, "_TARGET_WGS", 192 if half else 0)
                mp.setattr(gemm, "NT_MIN_BYTES", 1 if nt else 160 << 20)
                w, wp = weights(c, packed)
                assert bool(gemm._wmode(wp) & gemm.NT_BIT) == nt
                buf, out = gc.sentinel_out(M, N, DEV)
                gemm.linear(x, w, out=out, packed=wp, max_m=D)
                assert gc.same_bits(buf, want), (c.name, packed, half, nt)


@pytest.mark.parametrize("M", [1, 64])
def test_long_k(M):
    """K = 14336: bf16 out and the slabs of every split."""
    N, K = gc.LONG_SHAPE
    c = grid(N, K, M)
    x = dev_x(c)
    for packed in (False, True):
        w, wp = weights(c, packed)
        buf, out = gc.sentinel_out(M, N, DEV)
        gemm.linear(x, w, out=out, packed=wp)
        assert gc.same_bits(buf, gc.expect_buf(gc.ref_bf16(c))), (c.name, packed)
        for S in gc.splits(K):
            for half in (False, True):
                check_partial(c, x, w, wp, S, half)


def check_partial(c, x, w, wp, S, half):
    M, N = c.M, c.N
    ws = gc.sentinel_flat(S * M * N, DEV)
    p = gemm.linear_partial(x, w, ws, S, packed=wp, half=half)
    assert (p.S, p.M, p.N) == (S, M, N)
    assert gc.same_bits(p.view(), gc.ref_slabs(c, S)), (c.name, S, wp is not None, half)
    assert bool(ws[S * M * N:].isnan().all()), (c.name, S, half)


@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_partial(N, K):
    """fp32 slabs: every slab equals its float64 slab bit for bit, the NaN tail is intact."""
    for M in ALL_ROWS:
        c = grid(N, K, M)
        x = dev_x(c)
        for packed in (False, True):
            w, wp = weights(c, packed)
            for S in gc.splits(K):
                for half in (False, True):
                    check_partial(c, x, w, wp, S, half)


# -------------------------------------------------------------------------------------------- SiLU
@pytest.mark.parametrize("cls", ["small", "rounding"])
@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_silu_unsplit(N, K, cls, monkeypatch):
    for M in ALL_ROWS:
        c = silu_grid(N, K, M, 0, cls)
        acc = gc.ref_acc(c)
        x = dev_x(c)
        for packed, nt in ((False, False), (True, False), (True, True)):
            with monkeypatch.context() as mp:
                mp.setattr(gemm, "NT_MIN_BYTES", 1 if nt else 160 << 20)
                w, wp = weights(c, packed)
                y = gemm.linear_silu(x, w, None, packed=wp, max_m=D)
                check_silu(y, acc, what=(c.name, packed, nt))
                assert bool((y[:, 16:32] == 0).all())  # the zero-gate anchor
                # the same launch into a sentinel buffer
                buf, out = gc.sentinel_out(M, N // 2, DEV)
                gemm._launch_ex(gemm.MODE_SILU, x, w, wp, 1, out=out)
                assert gc.inside(buf, gc.iv_pad(gc.ref_silu(acc))), (c.name, packed, nt)


@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_silu_split(N, K):
    """Split over K, then pk_splitk_reduce: exact slabs, SiLU of their sum."""
    for M in gc.ROWS:
        S = gemm.choose_split(N, K, M)
        assert S == {256: 1, 512: 2, 1024: 4, 2048: 8}[K]
        c = silu_grid(N, K, M)
        x = dev_x(c)
        for packed in (False, True):
            w, wp = weights(c, packed)
            ws = gc.sentinel_flat(S * M * N, DEV)
            y = gemm.linear_silu(x, w, ws, packed=wp)
            check_silu(y, gc.ref_acc(c), what=(c.name, packed))
            if S > 1:
                assert gc.same_bits(ws[: S * M * N].view(S, M, N), gc.ref_slabs(c, S)), c.name
            assert bool(ws[S * M * N:].isnan().all())


@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_silu_norm_in(N, K):
    """The RMSNorm prologue with per-row power-of-two rinv: bit-exact activations, SiLU interval."""
    for M in gc.ROWS:
        for i, nparts in enumerate(gc.NPARTS):
            c, nw, parts = gc.norm_case(N, K, M, 0, nparts)
            acc = gc.ref_acc(c, x=gc.ref_norm_in(c.x, gc.ref_rinv(parts, K), nw))
            w, wp = weights(c, packed=bool((i + M) % 2))
            y = gemm.linear_silu(dev_x(c), w, packed=wp, norm=gemm.NormIn(dev_parts(parts), nw.to(DEV), gc.EPS))
            check_silu(y, acc, what=c.name)


@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_silu_rowscale(N, K):
    """Folded norm: unsplit (row tiles above 64 rows: 128 rows up to 16 parts, else 64) and split +
    reduce, under the interval criterion."""
    for M in ALL_ROWS:
        for nparts in gc.NPARTS:
            c = silu_grid(N, K, M, 0, "small" if nparts % 2 else "rounding")
            parts = gc.int_parts(M, nparts)
            rinv = gc.ref_rinv(parts, K)
            rs = gemm.RowScale(dev_parts(parts), gc.EPS)
            x = dev_x(c)
            w, wp = weights(c, True)
            s1 = gc.ref_slabs(c, 1)
            y = gemm.linear_silu(x, w, packed=wp, rowscale=rs)
            check_silu(y, s1[0] * rinv[:, None], gc.rowscale_err(s1, rinv), (c.name, nparts))
            S = gemm.gate_up_split(N, K, M) if M <= gemm.FUSED_MAX_M else 1
            if S > 1:
                ws = gc.sentinel_flat(S * M * N, DEV)
                y = gemm.linear_silu(x, w, ws, packed=wp, rowscale=rs)
                sl = gc.ref_slabs(c, S)
                check_silu(y, gc.ref_acc(c) * rinv[:, None], gc.rowscale_err(sl, rinv), (c.name, nparts, S))
                check_rowscale_slabs(ws[: S * M * N].view(S, M, N), sl, rinv, (c.name, nparts, S))
                assert bool(ws[S * M * N:].isnan().all())


def check_rowscale_slabs(got, slabs, rinv, what):
    ref = slabs * rinv[None, :, None]
    err = gc.DELTA_R * ref.abs()
    assert gc.within_rel(got, ref, err), what
    record("rowscale", gc.worst_ratio(got, ref, err))


@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_partial_rowscale(N, K):
    for M in ALL_ROWS:
        c = grid(N, K, M)
        x = dev_x(c)
        w, wp = weights(c, True)
        for nparts in gc.NPARTS:
            parts = gc.int_parts(M, nparts, 1)
            rinv = gc.ref_rinv(parts, K)
            rs = gemm.RowScale(dev_parts(parts), gc.EPS)
            for S in gc.splits(K):
                for half in (False, True):
                    ws = gc.sentinel_flat(S * M * N, DEV)
                    p = gemm.linear_partial_rowscale(x, w, ws, rs, S=S, packed=wp, half=half)
                    assert (p.S, p.M, p.N) == (S, M, N)
                    check_rowscale_slabs(p.view(), gc.ref_slabs(c, S), rinv, (c.name, nparts, S, half))
                    assert bool(ws[S * M * N:].isnan().all())


# --------------------------------------------------------------------------------- residual update
@pytest.mark.parametrize("cls", ["small", "rounding"])
@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_linear_add_residual(N, K, cls):
    """In-launch split-K reduction + residual update + parts, twice on the same counters with
    different inputs: residual exact, parts exact ("small") or within n u ref ("rounding"), the
    slabs exact, every sentinel intact, the counters zero afterwards."""
    ctr = torch.zeros(64, dtype=I32, device=DEV)
    for M in gc.ROWS:
        for half in (False, True):
            nblk = 64 if half else 128
            for packed in (False, True):
                for S in gc.splits(K):
                    for seed in (0, 1):
                        c, r = gc.residual_case(N, K, M, seed, cls, nblk)
                        new, parts = gc.ref_add_residual(gc.ref_acc(c), r, nblk)
                        w, wp = weights(c, packed)
                        rbuf, res = gc.sentinel_out(M, N, DEV, pad_cols=0)
                        res.copy_(r.to(BF16))
                        ws = gc.sentinel_flat(S * M * N, DEV)
                        pbuf = gc.sentinel_flat(N // nblk * M, DEV)
                        got = gemm.linear_add_residual(dev_x(c), w, ws, ctr, res, pbuf, S, packed=wp, half=half)
                        what = (c.name, half, packed, S)
                        assert gc.same_bits(rbuf, gc.expect_buf(new, pad_cols=0)), what
                        err = gc.parts_err(parts, nblk, cls)
                        assert got.shape == parts.shape and gc.within_rel(got, parts, err), what
                        if cls == "rounding":
                            record("parts", gc.worst_ratio(got, parts, err))
                        assert gc.same_bits(ws[: S * M * N].view(S, M, N), gc.ref_slabs(c, S)), what
                        assert bool(ws[S * M * N:].isnan().all()) and bool(pbuf[N // nblk * M:].isnan().all()), what
    assert int(ctr.abs().sum()) == 0


def test_add_residual_refuses_row_tiles():
    """M = 96 is still refused: the per-n-block tickets are not per row tile."""
    c, r = gc.residual_case(256, 512, 96)
    ws = torch.empty(2 * 96 * 256, dtype=F32, device=DEV)
    ctr = torch.zeros(64, dtype=I32, device=DEV)
    with pytest.raises(RuntimeError):
        gemm.linear_add_residual(c.x.to(DEV), c.w.to(DEV), ws, ctr, r.to(BF16).to(DEV),
                                 torch.empty(2 * 96, device=DEV), 2)
    assert int(ctr.abs().sum()) == 0


# ------------------------------------------------------------------------------------- QKV + RoPE
def dev_caches(nb, nkv, bs):
    kc = torch.full((nb, nkv, bs, 128), gc.POISON, dtype=BF16, device=DEV)
    vc = torch.full((nb, nkv, 128, bs), gc.POISON, dtype=BF16, device=DEV)
    return kc, vc


def check_caches(kc, vc, want_k, want_v, what):
    assert gc.same_bits(reference.k_cache_logical(kc), want_k), what
    assert gc.same_bits(reference.v_cache_logical(vc), want_v), what


@pytest.mark.parametrize("use_norm", [False, True])
@pytest.mark.parametrize("nq,nkv,bs", gc.QKV_HEADS)
def test_linear_qkv_rope(nq, nkv, bs, use_norm):
    """Mode 4 against the float64 reference (not A.rope_and_cache): poisoned caches, one row with
    slot -1, slots across a block boundary, two launches with different inputs on the same caches
    and counters."""
    K = 1024
    N = (nq + 2 * nkv) * 128
    cs = gc.rope_table()
    cs_d = cs.to(DEV)
    ctr = torch.zeros(64, dtype=I32, device=DEV)
    for M in gc.ROWS:
        pos = gc.rope_positions(M)
        slots, nb = gc.cache_slots(M, bs)
        for S in (1, 2, 4):
            for packed in (False, True):
                kc, vc = dev_caches(nb, nkv, bs)
                want_k = want_v = None
                for seed in (0, 1):
                    if use_norm:
                        c, nw, parts = gc.norm_case(N, K, M, seed, 1 + 2 * seed)
                        acc = gc.ref_acc(c, x=gc.ref_norm_in(c.x, gc.ref_rinv(parts, K), nw))
                        norm = gemm.NormIn(dev_parts(parts), nw.to(DEV), gc.EPS)
                    else:
                        c, norm = gc.qkv_case(nq, nkv, K, M, seed), None
                        acc = gc.ref_acc(c)
                    w, wp = weights(c, packed)
                    ws = gc.sentinel_flat(S * M * N, DEV)
                    q = gemm.linear_qkv_rope(dev_x(c), w, ws, ctr, pos.to(DEV), cs_d, kc, vc, slots.to(DEV), nq, nkv,
                                             S, packed=wp, norm=norm)
                    want_q, want_k, want_v = gc.ref_qkv(acc, pos, cs, slots, nq, nkv, bs, nb, want_k, want_v)
                    what = (c.name, S, packed, seed)
                    assert gc.same_bits(q, want_q), what
                    check_caches(kc, vc, want_k, want_v, what)
                    assert bool(ws[S * M * N:].isnan().all()), what
    assert int(ctr.abs().sum()) == 0


# ----------------------------------------------------------------------------------------- needles
NEEDLE = (256, 2048, 64)
NEEDLE_VALUE = -4.5  # 3 * -1.5


def needle_buffers():
    N, K, M = NEEDLE
    return torch.zeros((M, K), dtype=BF16, device=DEV), torch.zeros((N, K), dtype=BF16, device=DEV)


def set_needle(x, w, n, k, m, on=True):
    x[m, k] = 3.0 if on else 0.0
    w[n, k] = -1.5 if on else 0.0


def one_nonzero(t, idx, what):
    assert int(t.count_nonzero()) == 1 and float(t[idx]) == NEEDLE_VALUE, what


@pytest.mark.parametrize("packed", [False, True])
def test_needles_linear(packed):
    N, K, M = NEEDLE
    x, w = needle_buffers()
    for (n, k, m) in gc.decode_needle_points(N, K, M):
        set_needle(x, w, n, k, m)
        out = gemm.linear(x, w, packed=gemm.pack_weight(w) if packed else None)
        one_nonzero(out, (m, n), (n, k, m))
        set_needle(x, w, n, k, m, False)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("S", [1, 2, 4, 8])
def test_needles_partial(S, half):
    N, K, M = NEEDLE
    x, w = needle_buffers()
    ws = torch.empty(S * M * N, dtype=F32, device=DEV)
    for (n, k, m) in gc.decode_needle_points(N, K, M, S):
        set_needle(x, w, n, k, m)
        ws.fill_(float("nan"))
        p = gemm.linear_partial(x, w, ws, S, packed=gemm.pack_weight(w), half=half)
        one_nonzero(p.view(), (k // (K // S), m, n), (n, k, m))
        set_needle(x, w, n, k, m, False)


@pytest.mark.parametrize("half", [False, True])
def test_needles_add_residual(half):
    N, K, M = NEEDLE
    S = 2
    x, w = needle_buffers()
    ws = torch.empty(S * M * N, dtype=F32, device=DEV)
    ctr = torch.zeros(64, dtype=I32, device=DEV)
    nblk = 64 if half else 128
    for i, (n, k, m) in enumerate(gc.decode_needle_points(N, K, M, S)):
        set_needle(x, w, n, k, m)
        res = torch.zeros((M, N), dtype=BF16, device=DEV)
        pbuf = torch.full((N // nblk * M,), float("nan"), device=DEV)
        parts = gemm.linear_add_residual(x, w, ws, ctr, res, pbuf, S, packed=gemm.pack_weight(w) if i % 2 else None,
                                         half=half)
        one_nonzero(res, (m, n), (n, k, m))
        assert int(parts.count_nonzero()) == 1 and float(parts[n // nblk, m]) == NEEDLE_VALUE ** 2, (n, k, m)
        set_needle(x, w, n, k, m, False)
    assert int(ctr.abs().sum()) == 0


# ------------------------------------------------------------------------------- split-K consumers
def dev_partial(slabs: torch.Tensor) -> gemm.Partial:
    S, M, N = slabs.shape
    buf = gc.sentinel_flat(slabs.numel(), DEV)
    buf[: slabs.numel()] = slabs.reshape(-1).to(DEV)
    return gemm.Partial(buf, S, M, N)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8, 16])
def test_reduce_partial_and_silu_reduce(S):
    """pk_splitk_reduce on synthetic integer slabs (templated and generic S), plain and SiLU, into
    an output whose row stride exceeds N."""
    N = 1056  # 33 blocks of 32: more than one workgroup per row, no multiple of 128
    for M in (1, 17, 64):
        slabs = gc.int_slabs(S, M, N, 0, mag=40)
        slabs[:, :, 32:48] = 0  # the zero-gate anchor
        acc = slabs.double().sum(0)
        p = dev_partial(slabs)
        buf, out = gc.sentinel_out(M, N, DEV)
        gemm.reduce_partial(p, out)
        assert gc.same_bits(buf, gc.expect_buf(gc.bf(acc))), (S, M)
        buf, out = gc.sentinel_out(M, N // 2, DEV)
        gemm.silu_reduce(p, out)
        assert gc.inside(buf, gc.iv_pad(gc.ref_silu(acc))), (S, M)
        check_silu(out, acc, what=(S, M))
        assert bool((out[:, 16:32] == 0).all())


@pytest.mark.parametrize("H", [512, 1536])
@pytest.mark.parametrize("S", [0, 1, 2, 4, 8])
def test_residual_parts(S, H):
    for M in (1, 17, 64):
        for mag, cls in ((8, "small"), (300, "rounding")):
            r = torch.randint(-8, 9, (M, H), generator=torch.Generator().manual_seed(S + H + M)).double()
            slabs = gc.int_slabs(max(S, 1), M, H, 1, mag)
            acc = slabs.double().sum(0) if S else torch.zeros((M, H), dtype=torch.float64)
            new, parts = gc.ref_add_residual(acc, r, 512)
            assert cls == "rounding" or float(parts.max()) < 2 ** 24
            rbuf, res = gc.sentinel_out(M, H, DEV, pad_cols=0)
            res.copy_(r.to(BF16))
            pbuf = gc.sentinel_flat(H // 512 * M, DEV)
            got = gemm.residual_parts(dev_partial(slabs) if S else None, res, pbuf)
            err = gc.parts_err(parts, 512, cls)
            assert gc.same_bits(rbuf, gc.expect_buf(new, pad_cols=0)), (S, H, M, cls)
            assert gc.within_rel(got, parts, err) and bool(pbuf[H // 512 * M:].isnan().all()), (S, H, M, cls)
            if cls == "rounding":
                record("parts512", gc.worst_ratio(got, parts, err))


@pytest.mark.parametrize("S", [1, 2, 4, 8])
@pytest.mark.parametrize("H", [1024, 3072, 8192])
def test_partial_add_rms_norm(H, S):
    """Residual exact; the row's own sum of squares is H 4^j, so rinv is a power of two and x exact."""
    M = 17
    slabs, r, nw, new, want_x = gc.addnorm_case(M, H, S)
    rbuf, res = gc.sentinel_out(M, H, DEV, pad_cols=0)
    res.copy_(r)
    xbuf, x = gc.sentinel_out(M, H, DEV, pad_cols=0)
    gemm.partial_add_rms_norm(dev_partial(slabs), res, nw.to(DEV), gc.EPS, out=x)
    assert gc.same_bits(rbuf, gc.expect_buf(new, pad_cols=0)), (H, S)
    assert gc.same_bits(xbuf, gc.expect_buf(want_x, pad_cols=0)), (H, S)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("nq,nkv,bs", gc.QKV_HEADS)
def test_qkv_reduce_rope_cache(nq, nkv, bs, S):
    N = (nq + 2 * nkv) * 128
    cs = gc.rope_table()
    for M in (1, 17, 64):
        slabs = gc.int_slabs(S, M, N, 2, mag=20)
        pos = gc.rope_positions(M)
        slots, nb = gc.cache_slots(M, bs)
        kc, vc = dev_caches(nb, nkv, bs)
        q = gemm.qkv_reduce_rope_cache(dev_partial(slabs), pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), nq, nkv)
        want_q, want_k, want_v = gc.ref_qkv(slabs.double().sum(0), pos, cs, slots, nq, nkv, bs, nb)
        assert gc.same_bits(q, want_q), (S, M)
        check_caches(kc, vc, want_k, want_v, (S, M))


@pytest.mark.parametrize("nq,nkv,bs", gc.QKV_HEADS)
def test_rope_and_cache_exact(nq, nkv, bs):
    """A.rope_and_cache itself on the exact table (it has been the oracle of the other two writers):
    32 tokens filling an aligned 32-slot run (the gathered V path), then scattered ones."""
    cs = gc.rope_table()
    N = (nq + 2 * nkv) * 128
    for T in (1, 17, 32, 72):
        g = torch.Generator().manual_seed(T)
        qkv = torch.randint(-256, 257, (T, N), generator=g).double()
        pos = gc.rope_positions(T)
        tail, nb = gc.cache_slots(max(T - 32, 1), bs)
        if T >= 32:  # tokens 0..31 -> an aligned run in a block of its own, the rest as cache_slots
            slots = torch.cat([nb * bs + torch.arange(32, dtype=I32), tail[: T - 32]])
            nb += 2
        else:
            slots, nb = gc.cache_slots(T, bs)
        kc, vc = dev_caches(nb, nkv, bs)
        buf = torch.full((T, N + 128), float("nan"), dtype=BF16, device=DEV)  # row stride above N
        x = buf[:, :N]
        x.copy_(qkv.to(BF16))
        A.rope_and_cache(x, pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), nq, nkv)
        want_q, want_k, want_v = gc.ref_qkv(qkv, pos, cs, slots, nq, nkv, bs, nb)
        rot = gc.ref_rope(qkv.view(T, -1, 128)[:, : nq + nkv], pos, cs)
        assert gc.same_bits(x.view(T, -1, 128)[:, :nq], want_q), T
        assert gc.same_bits(x.view(T, -1, 128)[:, : nq + nkv], rot), T       # k rotated in place
        assert gc.same_bits(x.view(T, -1, 128)[:, nq + nkv:], qkv.view(T, -1, 128)[:, nq + nkv:]), T
        assert bool(buf[:, N:].isnan().all())
        check_caches(kc, vc, want_k, want_v, T)


@pytest.mark.parametrize("H", [1024, 4096])
def test_norm_apply(H):
    for M in (1, 17, 64):
        for nparts in (1, 3, 8):
            g = torch.Generator().manual_seed(H + M + nparts)
            res = torch.randint(-256, 257, (M, H), generator=g).double()
            nw = (torch.randint(1, 4, (H,), generator=g) * (2 * torch.randint(0, 2, (H,), generator=g) - 1)).double()
            parts = gc.pow2_parts(M, nparts, H)
            want = gc.ref_norm_in(res, gc.ref_rinv(parts, H), nw)
            exact = gc.bf(res * (2.0 ** -(torch.arange(M) % 4).double())[:, None] * nw[None, :])
            assert gc.same_bits(want, exact)  # the construction: rinv acts as 2^-j
            y = gemm.norm_apply(res.to(BF16).to(DEV), dev_parts(parts), nw.to(BF16).to(DEV), gc.EPS)
            assert gc.same_bits(y, want), (H, M, nparts)


# ----------------------------------------------------------------------------------- fused launch
@functools.lru_cache(maxsize=None)
def mlp_weights(H, I, S):
    g = torch.Generator().manual_seed(41)
    wgu = torch.randint(-2, 3, (2 * I, H), generator=g).to(BF16)
    wgu[32:48] = 0
    wd, k, v = gc.select_down(H, I, S)
    return wgu, gemm.pack_weight(wgu.to(DEV)), gemm.pack_weight(wd.to(DEV)), k, v


@pytest.mark.parametrize("M", [5, 100])
def test_mlp_fused_anchor(M):
    """gemm.mlp_fused against the float64 reference of the chain: h = SiLU of the row-scaled gate_up
    under the interval criterion, and a down weight with one non-zero per (column, split), so that
    every slab element is exactly +-1 or +-2 times one element of h, in any summation order.  Two
    launches with different inputs on the same flow words, which are zero afterwards."""
    H, I = 1024, 12288
    S = gemm.choose_split(H, I, M)
    assert S == 16 and gemm.gate_up_split(2 * I, H, M) == 1
    wgu, gup, dp, k, v = mlp_weights(H, I, S)
    assert H * 1 * 2 < 2 ** 24  # sum_k |x| |w|: the gate_up sums are exact
    flow = torch.zeros(gemm.FLOW_WORDS, dtype=I32, device=DEV)
    nparts = H // gemm.PART_COLS
    assert gemm.mlp_fused_ok(torch.empty((M, H), dtype=BF16, device=DEV), gup, dp, nparts)
    for seed in (0, 1):
        x = torch.randint(-1, 2, (M, H), generator=torch.Generator().manual_seed(seed + M)).to(BF16)
        parts = gc.int_parts(M, nparts, seed)
        rinv = gc.ref_rinv(parts, H)
        acc = x.double() @ wgu.double().t()
        sl = acc[None]
        h_lo, h_hi = gc.ref_silu(acc * rinv[:, None], gc.rowscale_err(sl, rinv))
        assert bool((h_lo[:, 16:32] == 0).all()) and bool((h_hi[:, 16:32] == 0).all())
        ws = gc.sentinel_flat(S * M * H, DEV)
        p = gemm.mlp_fused(gc.sentinel_rows(x.to(DEV)), gup, dp, gemm.RowScale(dev_parts(parts), gc.EPS), ws, flow)
        a, b = h_lo[:, k] * v[None], h_hi[:, k] * v[None]          # [M, S, H]
        lo, hi = torch.minimum(a, b).permute(1, 0, 2), torch.maximum(a, b).permute(1, 0, 2)
        assert (p.S, p.M, p.N) == (S, M, H)
        assert gc.inside(p.view(), (lo.contiguous(), hi.contiguous())), (M, seed)
        assert bool(ws[S * M * H:].isnan().all())
    torch.cuda.synchronize()
    gemm.check_fused()
    assert int(flow.abs().sum()) == 0


# ---------------------------------------------------------------------------------------- prefill
def prefill_variants(K):
    return [(4, False), (6, False)] + ([(5, True), (7, True)] if K % 128 == 0 else [])


@pytest.mark.parametrize("K", gc.PREFILL_K)
@pytest.mark.parametrize("N", gc.PREFILL_N)
def test_prefill_grid(N, K):
    """gemm_prefill.linear, dense: variants 4 and 6 on row-major W (6 falls back to 4 where
    K % 128 != 0), 5 and 7 on packed W; strided A and C, NaN rows of A beyond M, NaN around C."""
    for M in gc.PREFILL_M:
        c = silu_grid(N, K, M)
        acc = gc.ref_acc(c)
        want = gc.expect_buf(gc.bf(acc))
        want_silu = gc.iv_pad(gc.ref_silu(acc))
        x = dev_x(c)
        for variant, packed in prefill_variants(K):
            w, wp = weights(c, packed)
            buf, out = gc.sentinel_out(M, N, DEV)
            gemm_prefill.linear(x, w, out=out, variant=variant, packed=wp)
            assert gc.same_bits(buf, want), (c.name, variant)
            buf, out = gc.sentinel_out(M, N // 2, DEV)
            gemm_prefill.linear(x, w, out=out, silu=True, variant=variant, packed=wp)
            assert gc.inside(buf, want_silu), (c.name, variant)
            check_silu(out, acc, what=(c.name, variant))
            assert bool((out[:, 16:32] == 0).all())


@pytest.mark.parametrize("M,N,K", [(513, 512, 1024), (257, 256, 192)])
def test_prefill_needles(M, N, K):
    x = torch.zeros((M, K), dtype=BF16, device=DEV)
    w = torch.zeros((N, K), dtype=BF16, device=DEV)
    for (n, k, m) in gc.prefill_needle_points(M, N, K):
        set_needle(x, w, n, k, m)
        for variant, packed in prefill_variants(K):
            out = gemm_prefill.linear(x, w, variant=variant, packed=gemm.pack_weight(w) if packed else None)
            one_nonzero(out, (m, n), (n, k, m, variant))
        set_needle(x, w, n, k, m, False)
