"""RMSNorm, fused add + RMSNorm, SiLU-and-mul (split and interleaved), the embedding gather and the
staging copy against float64, at every vector-per-thread width and every edge of their loops.

tests/rowwise_cases.py builds the inputs (power-of-four rows that make the norm bit-exact, integer
rows whose sum of squares is exact, rows below eps, Gaussian rows, sums that round on the way into
the residual; every bf16 bit pattern as SiLU gate; random 16-bit patterns as embedding table; NaN
or sentinel words around everything a kernel may write), the float64 references with the documented
roundings, and the criteria: bit-exact wherever the arithmetic is exact, the interval criterion of
tests/gemm_cases.py where it is not.  No element is exempt.  tests/unit/test_rowwise_cases.py shows
on the CPU that every wrong reference (eps dropped or misplaced, a lost wave or vector in the sum, a
weight indexed by thread or shifted, one rounding instead of two, the scale of another row, a wrong
stride, a sum of squares of the wrong or the unrounded residual; gate / up exchanged or mispaired,
a wrong interleave, an unrounded SiLU, a lost workgroup; every mask, stride and tail slip of the
gather) fails them.

The outputs are bf16, so an error inside the derived bound (u = 2^-24) is visible only where it
moves a rounding: the record per family is the number of outputs that differ from the float64
reference evaluated without any slack (every one of them inside its interval).  On MI355X:

    family                                      bound on r or silu     outputs off the zero-slack reference
    pow4 rows (same_bits)                       exact                  0 of 3784704 (plain), 0 of 3784704 (fused)
    integer rows                                5 u                    0 of 1892352, 0 of 1892352
    rows below eps                              5 u                    0 of 1892352, 0 of 1892352
    Gaussian rows                               (H / 2 + 5) u          0 of 1892352, 0 of 1892352
    rounding rows (fused)                       5 u                    0 of 1892352
    SiLU, Gaussian gates and the full sweep     (8 + 2 |g|) u          15366 of 758144 (2.0 %)

so the largest observed |got - ref| / bound is 0 for every norm family (the kernel's tree reduction
is far more accurate than the any-order bound of the Gaussian rows), and for SiLU every one of the
15366 outputs lies inside its interval.  ``pytest -s`` prints the running figures as RECORD lines.
The 43 tests of this file take about 4 s together on one MI355X, none more than 0.4 s.

A scratch build with six in-bounds numeric errors (eps dropped in rmsnorm_kernel, g[threadIdx.x] in
its second pass, ss of the unrounded sum in the fused kernel, an unrounded SiLU in the split kernel,
gate and up exchanged in the interleaved kernel, ``local > 0`` in the embedding mask) turned 31 of
these tests red (every norm, SiLU and embedding test that launches) and none of the numeric tests
of tests/kernels/test_norm_act.py.
"""
import functools

import pytest
import torch

from polykey_service_amd import ops
from polykey_service_amd.ops import gemm, native
from tests import gemm_cases as gc
from tests import rowwise_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
I16 = torch.int16
I32 = torch.int32
NAN = float("nan")

norm_case = functools.lru_cache(maxsize=None)(rc.norm_case)
embed_table = functools.lru_cache(maxsize=None)(rc.embed_table)

RECORD = {}


def record(key, off, n):
    a, b = RECORD.get(key, (0, 0))
    RECORD[key] = (a + off, b + n)
    print(f"RECORD {key} {RECORD[key][0]} of {RECORD[key][1]} outputs off the zero-slack reference")


def flat_nan(n, tail=64, dtype=BF16):
    return torch.full((n + tail,), NAN, dtype=dtype, device=DEV)


def check_norm(got, c, iv, what):
    if c.exact:
        assert gc.same_bits(got, iv[0]), (c.name, what)
    assert gc.inside(got, iv), (c.name, what)


def families(H, fused):
    for T in rc.NORM_T:
        for fam in (rc.FUSED_FAMILIES if fused else rc.FAMILIES):
            for eps in (rc.NORM_EPS if fam == "pow4" else [1e-5]):
                yield norm_case(fam, T, H, eps, fused)


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("H", list(rc.WIDTHS))
def test_rms_norm(H):
    """Contiguous rows, then a column slice of a wider NaN tensor into an ``out=`` slice of another:
    every family, T in {1, 3, 17}; nothing outside [T, H] is written and the input is left alone."""
    for c in families(H, False):
        T = c.T
        w = c.w.to(BF16).to(DEV)
        iv, _ = rc.ref_norm(c)
        x = c.a.to(BF16).to(DEV)
        y = ops.rms_norm(x, w, c.eps)
        assert y.shape == (T, H) and y.is_contiguous()
        check_norm(y, c, iv, "contiguous")
        record(c.family, rc.count_off(y, rc.norm_mid(c)), y.numel())
        xbuf, xv = rc.sliced(x, rc.IN_GEOM)
        obuf, ov = rc.sliced(torch.full((T, H), NAN, dtype=BF16, device=DEV), rc.OUT_GEOM)
        assert xv.stride(0) == H + 24 and ov.stride(0) == H + 16 and xv.data_ptr() % 16 == 0 == ov.data_ptr() % 16
        before = xbuf.clone()
        y2 = ops.rms_norm(xv, w, c.eps, out=ov)
        assert y2.data_ptr() == ov.data_ptr()
        want = rc.ref_norm_sliced(c)
        if c.exact:
            assert gc.same_bits(obuf, want[0]), (c.name, "sliced")
        assert gc.inside(obuf, want), (c.name, "sliced")
        assert gc.same_bits(xbuf, before) and gc.same_bits(y2, y), (c.name, "sliced")


@pytest.mark.parametrize("H", list(rc.WIDTHS))
def test_fused_add_rms_norm(H):
    """The new residual bit for bit (a = -b and the sums that round included), x by the family's
    criterion; the words behind both buffers stay NaN."""
    for c in families(H, True):
        T = c.T
        iv, new = rc.ref_norm(c)
        xb, rb = flat_nan(T * H), flat_nan(T * H)
        x, r = xb[:T * H].view(T, H), rb[:T * H].view(T, H)
        x.copy_(c.a.to(BF16))
        r.copy_(c.b.to(BF16))
        gx, gr = ops.fused_add_rms_norm(x, r, c.w.to(BF16).to(DEV), c.eps)
        assert gx.data_ptr() == x.data_ptr() and gr.data_ptr() == r.data_ptr()
        assert gc.same_bits(r, new), (c.name, "residual")
        check_norm(x, c, iv, "x")
        assert bool(xb[T * H:].isnan().all()) and bool(rb[T * H:].isnan().all()), c.name
        record("fused-" + c.family, rc.count_off(x, rc.norm_mid(c)), x.numel())


def test_rms_norm_refuses_what_the_vectors_cannot_take():
    """A row stride that is no multiple of 8, a base that is not 16-byte aligned, on either side:
    refused ahead of any launch (the destination keeps its NaN)."""
    H = 512
    w = torch.ones(H, dtype=BF16, device=DEV)
    good = torch.ones((4, H + 16), dtype=BF16, device=DEV)
    odd = torch.ones((4, H + 4), dtype=BF16, device=DEV)
    out = torch.full((4, H + 16), NAN, dtype=BF16, device=DEV)
    oout = torch.full((4, H + 4), NAN, dtype=BF16, device=DEV)
    for x, o in ((good[:, 4:4 + H], out[:, :H]), (odd[:, :H], out[:, :H]), (good[:, :H], out[:, 4:4 + H]),
                 (good[:, :H], oout[:, :H]), (good[:, :H], out[:3, :H]), (good[:, :H], out[:, :2 * H:2])):
        with pytest.raises((AssertionError, ValueError)):
            ops.rms_norm(x, w, 1e-5, out=o)
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(oout.isnan().all())


# ------------------------------------------------------------------------------------------- SiLU
def run_silu(x, il, what):
    """x: bf16 [T, 2I] on the CPU.  Into a NaN-padded flat buffer; the whole buffer is compared."""
    T, I = x.shape[0], x.shape[1] // 2
    buf = flat_nan(T * I)
    out = buf[:T * I].view(T, I)
    fn = gemm.silu_and_mul_interleaved if il else ops.silu_and_mul
    got = fn(x.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    iv = rc.ref_silu_mul(x.double(), il)
    assert gc.inside(buf, iv), what
    fresh = fn(x.to(DEV))
    assert fresh.shape == (T, I) and gc.same_bits(fresh, out), what
    mid = rc.ref_silu_mul(x.double(), il, slack=False)[0]
    record("silu", rc.count_off(buf, mid), T * I)


@pytest.mark.parametrize("il", [False, True])
def test_silu_sweep(il):
    """Every bf16 bit pattern as gate against up = 1, -1, 1.5 and 0: exactly g from 18 up, a zero
    from -89 down, exactly 0 at a zero gate, NaN exactly where float64 gives NaN."""
    run_silu(rc.silu_sweep(il), il, "sweep")


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("I", rc.SILU_I)
def test_silu_gauss(I, il):
    for T in rc.SILU_T:
        x = rc.silu_gauss(T, I).to(BF16)
        if il and I % 16:
            buf = flat_nan(T * I)
            with pytest.raises(native.KernelError):
                gemm.silu_and_mul_interleaved(x.to(DEV), out=buf[:T * I].view(T, I))
            assert bool(buf.isnan().all())
        else:
            run_silu(x, il, (T, I))


def test_silu_refusals():
    """I % 8 != 0 is refused by the launcher, a strided or short destination by the wrapper; the
    buffer is untouched."""
    x = torch.ones((3, 24), dtype=BF16, device=DEV)
    buf = flat_nan(3 * 24)
    with pytest.raises(native.KernelError):
        ops.silu_and_mul(x, out=buf[:36].view(3, 12))
    x = torch.ones((3, 32), dtype=BF16, device=DEV)
    for fn in (ops.silu_and_mul, gemm.silu_and_mul_interleaved):
        for out in (buf[:72].view(3, 24)[:, :16], buf[:96:2].view(3, 16), buf[:32].view(2, 16)):
            with pytest.raises(AssertionError):
                fn(x, out=out)
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())


# -------------------------------------------------------------------------------------- embedding
def launch_embedding(table, ids, start, local):
    """Through native.call into a NaN-padded buffer -> int16 on the CPU."""
    T, H = ids.numel(), table.shape[1]
    out = flat_nan(T * H)
    dt, di = table.to(DEV), ids.to(I32).to(DEV)
    native.call("pk_embedding", out.data_ptr(), dt.data_ptr(), di.data_ptr(), T, H, start, local, native.stream_ptr())
    return out.view(I16).cpu()


@pytest.mark.parametrize("H", rc.EMBED_H)
def test_embedding(H):
    """A bit copy of random 16-bit patterns, 0x0000 for the rows of other shards, NaN behind the
    last row: the shard edges as ids, alone (T = 1) and among 77, as int32, int64 and 2-D ids."""
    for (start, local, holds) in rc.EMBED_SHARDS:
        table = embed_table(local, H)
        what = (H, start, local)
        for sp in rc.embed_special_ids(start, local, holds):
            one = torch.tensor([sp])
            assert torch.equal(launch_embedding(table, one, start, local), rc.ref_embedding(table, one, start, local)), (what, sp)
        ids = rc.embed_ids(77, start, local, holds)
        want = rc.ref_embedding(table, ids, start, local)
        assert torch.equal(launch_embedding(table, ids, start, local), want), what
        tb = table.view(BF16).to(DEV)
        for v in (ids.to(I32), ids, ids.view(7, 11), ids.to(I32).view(11, 7)):
            got = ops.embedding(v.to(DEV), tb, start, local)
            assert got.shape == v.shape + (H,) and got.dtype == BF16
            assert torch.equal(got.reshape(-1).view(I16).cpu(), want[:-64]), (what, v.dtype, v.shape)


# ----------------------------------------------------------------------------------- staging copy
@pytest.mark.parametrize("nbytes", rc.COPY_BYTES)
def test_copy_from_host(nbytes):
    """From a pinned int32 buffer, as the model runner stages a step: the first ``nbytes`` bytes
    arrive, the sentinel behind them stays."""
    n = nbytes // 4
    src = rc.copy_source(nbytes, pin=True)
    assert src.is_pinned() and src.numel() == n + 16
    dst = torch.full((n + 16,), rc.COPY_SENTINEL, dtype=I32, device=DEV)
    native.call("pk_copy_from_host", dst.data_ptr(), src.data_ptr(), nbytes, native.stream_ptr())
    got = dst.cpu()
    assert torch.equal(got[:n], src[:n]) and bool((got[n:] == rc.COPY_SENTINEL).all())


def test_copy_from_host_refusals():
    src = rc.copy_source(64, pin=True)
    dst = torch.full((32,), rc.COPY_SENTINEL, dtype=I32, device=DEV)
    for bad in (8, 24, 63):
        with pytest.raises(native.KernelError):
            native.call("pk_copy_from_host", dst.data_ptr(), src.data_ptr(), bad, native.stream_ptr())
    native.call("pk_copy_from_host", dst.data_ptr(), src.data_ptr(), 0, native.stream_ptr())
    assert bool((dst.cpu() == rc.COPY_SENTINEL).all())
