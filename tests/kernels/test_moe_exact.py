"""MoE kernels against the float64 references of tests/moe_cases.py: routing, align, permute and the
three combines, the three grouped GEMMs and ``fused_moe`` end to end.

Inputs are chosen so that the expected value is known exactly wherever the arithmetic allows it:
grid logits (ids must match on every row), integer GEMM operands and integer combine data (outputs
bit-equal to the integers), NaN poison in everything a kernel must not read and a finite sentinel in
everything it must not write.  Where bf16 rounding or a transcendental is involved the criteria are
those of tests/moe_cases.py: u = 2^-8, combine u |ref| + k 2^-23 sum |w y|, RMSNorm and SiLU
2.25 u |ref|, end to end 4.25 u sum_j w_j sum_i |h w2|.  tests/unit/test_moe_cases.py shows on the
CPU that every one of these checks rejects the mutants of the references.

The exports are called through ``native.call`` with sentinel-filled buffers, as ops/moe.py calls them,
so rows that must stay untouched can be inspected; the wrappers are then checked against that.

Each test prints ``ratio <name> <largest error / bound>`` (run with -s to see it).
"""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_prefill, moe, native
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


def sent(shape, dtype=BF):
    return torch.full(shape, mc.SENT_I if dtype == torch.int32 else mc.SENT, dtype=dtype, device=DEV)


def report(name, ratio):
    print(f"ratio {name} {ratio:.4g}")


# ------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("T,E,k", mc.ROUTE_CASES)
def test_topk_softmax_grid(T, E, k, renorm):
    lg = mc.grid_logits(T, E, k, seed=T + E)
    view = mc.strided(lg).to(DEV)[:, 2:2 + E]
    assert view.stride(0) > E
    ids, w = sent((T + 2, k), torch.int32), sent((T + 2, k), torch.float32)
    native.call("pk_moe_topk_softmax", ids.data_ptr(), w.data_ptr(), view.data_ptr(), T, E, k, view.stride(0),
                int(renorm), native.stream_ptr())
    assert bool((ids[T:] == mc.SENT_I).all()) and bool((w[T:] == mc.SENT).all()), "written past row T"
    report("route_weights_rel", mc.check_route(ids[:T].cpu(), w[:T].cpu(), lg, k, renorm))
    ids2, w2 = moe.topk_softmax(view, k, renorm)   # the wrapper passes the stride on
    assert torch.equal(ids2, ids[:T]) and torch.equal(w2, w[:T])


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("T,E,k", mc.ROUTE_CASES)
def test_add_rmsnorm_route_exact_logits(T, E, k, renorm):
    """The norm kernel that also routes: exact integer logits (ties included), so the new residual
    and x are bit-exact and ids and weights are judged by route64 of the kernel's own logits,
    F.linear(x, router) (exact in bf16), on every row: with exact logits no row is a near-tie that
    would have to be set aside, and exact ties must go to the lower expert id."""
    S = 2 if T % 2 else 4
    slabs, res, nw, router, v, x_ref, logits = mc.route_norm_case(T, E, T + E + k, S)
    H = res.shape[1]
    p = gemm.Partial(slabs.reshape(-1).to(DEV), S, T, H)
    x, r, ids, w = gemm.partial_add_rms_norm_route(p, res.to(DEV), nw.to(DEV), 0.0, router.to(DEV), k, renorm)
    mc.check_exact(r.cpu(), v, "residual")
    mc.check_exact(x.cpu(), x_ref, "x")
    own = torch.nn.functional.linear(x.cpu().double(), router.double()).to(BF)
    assert torch.equal(own, logits)
    report("route_norm_weights_rel", mc.check_route(ids.cpu(), w.cpu(), own, k, renorm))


# --------------------------------------------------------------------------------------- align
def run_align(ids_np, E, lo, hi):
    n, El = len(ids_np), hi - lo
    ids = torch.from_numpy(ids_np).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    off, srt, inv = sent((El + 3,), torch.int32), sent((max(n, 1) + 2,), torch.int32), sent((max(n, 1) + 2,), torch.int32)
    native.call("pk_moe_align", ids.data_ptr(), off.data_ptr(), srt.data_ptr(), inv.data_ptr(), n, E, lo, hi,
                native.stream_ptr())
    assert bool((off[El + 1:] == mc.SENT_I).all()) and bool((srt[n:] == mc.SENT_I).all()) and bool((inv[n:] == mc.SENT_I).all())
    return off[:El + 1], srt[:n], inv[:n]


@pytest.mark.parametrize("case", mc.ALIGN_CASES, ids=lambda c: c.name)
def test_align(case):
    ids = case.ids()
    off, srt, inv = run_align(ids, case.E, case.e_lo, case.e_hi)
    mc.check_align(off.cpu().numpy(), srt.cpu().numpy(), inv.cpu().numpy(), ids, case.e_lo, case.e_hi)
    if case.n:
        o2, s2, i2 = moe.align(torch.from_numpy(ids).to(DEV), case.E, case.e_lo, case.e_hi)
        m = int(off[-1])
        assert torch.equal(o2, off) and torch.equal(s2[:m], srt[:m]) and torch.equal(i2, inv)


# --------------------------------------------------------------------------- permute / combine
@pytest.mark.parametrize("H", [8, 1024, 2056])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_permute(H, k):
    T, E, lo, hi = 9, 8, 2, 6
    g = np.random.default_rng(H + k)
    ids = np.stack([g.permutation(E)[:k] for _ in range(T)]).astype(np.int32)
    ids[1] = 0   # a token with no local slot
    off, srt, inv = mc.align_ref(ids, lo, hi)
    m, n = int(off[-1]), T * k
    assert 0 < m < n
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(H)).to(BF)
    s_full = np.full(n, mc.SENT_I, dtype=np.int32)
    s_full[:m] = srt
    out = sent((n + 1, H))
    xd, sd, od = x.to(DEV), torch.from_numpy(s_full).to(DEV), torch.from_numpy(off.astype(np.int32)).to(DEV)
    native.call("pk_moe_permute", out.data_ptr(), xd.data_ptr(), sd.data_ptr(), od.data_ptr(), n, hi - lo, k, H,
                native.stream_ptr())
    ref = torch.full((n + 1, H), mc.SENT, dtype=BF)
    ref[:m] = mc.permute_ref(x, srt, k)
    mc.check_exact(out.cpu(), ref, "permute")
    got = moe.permute(xd, sd, od, k)
    assert torch.equal(got[:m].cpu(), ref[:m])


@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("H", [8, 1024, 2056])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_unpermute(k, H, integer):
    T = 5
    y, inv, w = mc.combine_case(T, k, H, integer, seed=T + k + H)
    ref, mag = mc.combine64(y, inv, w, T, k)
    out = sent((T + 1, H))
    yd, invd, wd = y.to(DEV), inv.to(DEV), w.to(DEV)
    native.call("pk_moe_unpermute", out.data_ptr(), yd.data_ptr(), invd.data_ptr(), wd.data_ptr(), T, k, H,
                native.stream_ptr())
    assert bool((out[T] == mc.SENT).all())
    o = out[:T].cpu()
    assert bool((o[1] == 0).all()), "a token without a local slot is not exactly zero"
    if integer:
        mc.check_exact(o, ref, "unpermute")
    else:
        report("combine", mc.check_combine(o, ref, mag, k))
    assert torch.equal(moe.unpermute(yd, invd, wd, T, k).cpu(), o)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("H", [8, 1024, 2056])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_unpermute_partial(k, H, S):
    """Combine from fp32 split-K slabs == unpermute of the bf16-rounded slab sum, bit for bit."""
    T = 5
    y, inv, w = mc.combine_case(T, k, H, True, seed=T + k + H + S)
    R = y.shape[0]
    assert R > T * k
    g = torch.Generator().manual_seed(S)
    slabs = torch.randint(-64, 65, (S, R, H), generator=g).float()
    slabs[S - 1] = y.float() - slabs[: S - 1].sum(0)
    assert torch.equal(slabs.sum(0).to(BF), y)
    ref, _ = mc.combine64(y, inv, w, T, k)
    out = sent((T + 1, H))
    sd, yd, invd, wd = slabs.to(DEV), y.to(DEV), inv.to(DEV), w.to(DEV)
    native.call("pk_moe_unpermute_partial", out.data_ptr(), sd.data_ptr(), S, R, invd.data_ptr(), wd.data_ptr(), T, k,
                H, native.stream_ptr())
    assert bool((out[T] == mc.SENT).all())
    mc.check_exact(out[:T].cpu(), ref, "unpermute_partial")
    assert torch.equal(out[:T], moe.unpermute(yd, invd, wd, T, k))
    # randn slabs: the sum is rounded to bf16 before the weighted combine
    yr = torch.randn(S, R, H, generator=g)
    ysum = yr[0].clone()
    for s in range(1, S):
        ysum += yr[s]   # fp32, in slab order, as the kernel adds them
    ref, mag = mc.combine64(ysum.to(BF), inv, w, T, k)
    sd = yr.to(DEV)
    native.call("pk_moe_unpermute_partial", out.data_ptr(), sd.data_ptr(), S, R, invd.data_ptr(), wd.data_ptr(), T, k,
                H, native.stream_ptr())
    report("combine_partial", mc.check_combine(out[:T].cpu(), ref, mag, k))


@pytest.mark.parametrize("H", [1024, 2048, 4096, 8192])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_combine_add_rms_norm(k, H):
    T, eps = 3, 1e-5
    g = torch.Generator().manual_seed(H + k)
    nw = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    for integer in (True, False):
        y, inv, w = mc.combine_case(T, k, H, integer, seed=H + k)
        if integer:
            res = (torch.randint(-64, 65, (T, H), generator=g).float() / 8).to(BF)
        else:
            res = torch.randn(T, H, generator=g).to(BF)
        comb, mag = mc.combine64(y, inv, w, T, k)
        x, r = sent((T + 1, H)), torch.cat([res, torch.full((1, H), mc.SENT, dtype=BF)]).to(DEV)
        yd, invd, wd, nwd = y.to(DEV), inv.to(DEV), w.to(DEV), nw.to(DEV)
        native.call("pk_moe_combine_add_rmsnorm", x.data_ptr(), r.data_ptr(), yd.data_ptr(), invd.data_ptr(),
                    wd.data_ptr(), nwd.data_ptr(), T, k, H, eps, native.stream_ptr())
        assert bool((x[T] == mc.SENT).all()) and bool((r[T] == mc.SENT).all())
        rc, xc = r[:T].cpu(), x[:T].cpu()
        if integer:
            mc.check_exact(rc, comb + res.double(), "residual")
            assert torch.equal(rc[1], res[1]), "a token without a local slot changed its residual"
        else:
            # bf16(bf16(combine) + residual): the combine criterion, then one more rounding, of the sum
            total = comb + res.double()
            err, bound = (rc.double() - total).abs(), mc.U * comb.abs() + k * 2.0 ** -23 * mag + mc.U * total.abs()
            assert bool((err <= bound).all()), float((err - bound).max())
            report("combine_fused", float((err / bound.clamp_min(1e-300)).max()))
        report("norm_x", mc.check_rel(xc, mc.rmsnorm64(rc, nw, eps), 2.25, "x"))
        # the wrapper
        pend = moe.PendingCombine(yd, invd, wd, T, k)
        x2, r2 = moe.combine_add_rms_norm(pend, res.to(DEV), nwd, eps)
        assert torch.equal(x2, x[:T]) and torch.equal(r2, r[:T])


# --------------------------------------------------------------------------------- grouped GEMM
def expect(case, A, W, offs):
    full = mc.grouped64(A, W, offs)
    return full, mc.with_sentinel(full), mc.with_sentinel(mc.silu_ref(full))


@pytest.mark.parametrize("case", mc.MOE_GEMM_CASES, ids=lambda c: c.id)
def test_moe_gemm(case):
    """pk_moe_gemm, the grouped GEMM of shapes the weight-streaming kernel does not take."""
    A, W, offs = case.build()
    full, ref, sref = expect(case, A, W, offs)
    R, G, N, K = A.shape[0], len(case.sizes), case.N, case.K
    Ad, Wd, od = A.to(DEV), W.to(DEV), offs.to(DEV)
    for mode, n_out in ((0, N), (2, N // 2)):
        out = sent((R, n_out))
        native.call("pk_moe_gemm", out.data_ptr(), Ad.data_ptr(), Wd.data_ptr(), od.data_ptr(), case.max_rows, N, K,
                    out.stride(0), G, mode, native.stream_ptr())
        if mode == 0:
            mc.check_exact(out.cpu(), ref, "bf16")
        else:
            report("silu_moe_gemm", mc.check_rel(out.cpu(), sref, 2.25, "silu"))
        # moe.grouped_gemm sends N % 128 != 0 to this kernel
        m = int(offs[-1])
        got = moe.grouped_gemm(Ad, Wd, od, case.max_rows, silu=mode == 2)
        assert torch.equal(got[:m], out[:m])


def launch_grouped(mode, a, w, offsets, max_rows, packed, S, out, ws, **extra):
    """gemm.grouped_linear's launch with caller-owned (sentinel-filled) outputs."""
    G, N, K = w.shape
    gemm._launch_ex(mode, a, w.view(G * N, K), None if packed is None else packed.view(G * N, K), S, out=out,
                    ws=ws, row_offsets=offsets, w_stride=N * K, groups=G, max_group_rows=max_rows, **extra)


@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("case", mc.SKINNY_CASES, ids=lambda c: c.id)
def test_grouped_linear(case, packed):
    A, W, offs = case.build()
    full, ref, sref = expect(case, A, W, offs)
    R, G, N, K = A.shape[0], len(case.sizes), case.N, case.K
    m = int(offs[-1])
    Ad, Wd, od = A.to(DEV), W.to(DEV), offs.to(DEV)
    Wp = gemm.pack_weight(Wd.view(G * N, K)).view(G, N, K) if packed else None
    out = sent((R, N))
    launch_grouped(gemm.MODE_BF16, Ad, Wd, od, case.max_rows, Wp, 1, out, None)
    mc.check_exact(out.cpu(), ref, "bf16")
    assert torch.equal(gemm.grouped_linear(Ad, Wd, od, case.max_rows, False, packed=Wp)[:m], out[:m])
    h = sent((R, N // 2))
    launch_grouped(gemm.MODE_SILU, Ad, Wd, od, case.max_rows, Wp, 1, h, None)
    report("silu_skinny", mc.check_rel(h.cpu(), sref, 2.25, "silu"))
    assert torch.equal(gemm.grouped_linear(Ad, Wd, od, case.max_rows, True, packed=Wp)[:m], h[:m])
    S = K // 256
    if S > 1:   # slab s is exactly the integer sum over k in [s K/S, (s+1) K/S)
        ws = sent((S * R * N + 64,), torch.float32)
        launch_grouped(gemm.MODE_PARTIAL, Ad, Wd, od, case.max_rows, Wp, S, None, ws)
        assert bool((ws[S * R * N:] == mc.SENT).all())
        mc.check_exact(ws[: S * R * N].view(S, R, N).cpu(), mc.with_sentinel(mc.slab_refs(A, W, offs, S)), "slabs")
        ws2 = sent((S * R * N,), torch.float32)
        assert gemm.grouped_linear(Ad, Wd, od, case.max_rows, False, packed=Wp, ws=ws2, S=S) is ws2
        assert torch.equal(ws2, ws[: S * R * N])


@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("T,k,N,K", [(24, k, N, K) for k in (1, 2, 4) for N, K in ((128, 256), (256, 512))])
def test_grouped_linear_gathered(T, k, N, K, packed):
    """The MoE permute folded into the A staging: a_rows = sorted, a_row_div = k, n_rows = T k."""
    x, W, ids, offs, srt, A = mc.gather_case(T, k, 6, 1, 5, N, K, seed=T + k + N)
    G, m, n = W.shape[0], int(offs[-1]), T * k
    full = mc.grouped64(A, W, offs)
    ref, sref = mc.with_sentinel(full), mc.with_sentinel(mc.silu_ref(full))
    xd, Wd, od, Ad = x.to(DEV), W.to(DEV), offs.to(DEV), A.to(DEV)
    Wp = gemm.pack_weight(Wd.view(G * N, K)).view(G, N, K) if packed else None
    s_full = sent((n,), torch.int32)
    s_full[:m] = srt.to(DEV)
    gather = dict(a_rows=s_full, a_row_div=k, m_override=n)
    for mode, n_out, want in ((gemm.MODE_BF16, N, ref), (gemm.MODE_SILU, N // 2, sref)):
        out, perm = sent((n, n_out)), sent((n, n_out))
        launch_grouped(mode, xd, Wd, od, T, Wp, 1, out, None, **gather)
        launch_grouped(mode, Ad, Wd, od, T, Wp, 1, perm, None)
        assert torch.equal(out, perm), "gathered form differs from the permuted form"
        if mode == gemm.MODE_BF16:
            mc.check_exact(out.cpu(), want, "bf16")
        else:
            report("silu_gathered", mc.check_rel(out.cpu(), want, 2.25, "silu"))
        got = gemm.grouped_linear(xd, Wd, od, T, mode == gemm.MODE_SILU, packed=Wp, a_rows=s_full, a_row_div=k, n_rows=n)
        assert torch.equal(got[:m], out[:m])


@pytest.mark.parametrize("silu", [False, True], ids=["bf16", "silu"])
@pytest.mark.parametrize("variant", [4, 6])
@pytest.mark.parametrize("case", mc.PREFILL_CASES, ids=lambda c: c.id)
def test_prefill_grouped_linear(case, variant, silu):
    A, W, offs = case.build()
    full, ref, sref = expect(case, A, W, offs)
    out = sent((A.shape[0], case.N // 2 if silu else case.N))
    gemm_prefill.grouped_linear(A.to(DEV), W.to(DEV), offs.to(DEV), silu=silu, out=out, variant=variant)
    if silu:
        report("silu_prefill", mc.check_rel(out.cpu(), sref, 2.25, "silu"))
    else:
        mc.check_exact(out.cpu(), ref, "bf16")


# ---------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("defer", [False, True], ids=["combine", "defer"])
@pytest.mark.parametrize("ep", mc.EP_RANGES)
@pytest.mark.parametrize("case", mc.MOE_CASES, ids=lambda c: c.name)
def test_fused_moe(case, ep, defer):
    """Plumbing of the three routes of fused_moe: the decode path (gathered w13 GEMM), the path of
    more than 64 tokens (permute, 128-row tiles) and shapes the weight-streaming GEMM does not take
    (pk_moe_gemm)."""
    lo, hi = ep
    x, router, w13, w2 = case.build(lo, hi)
    ref, B = mc.moe64(x, router, w13, w2, case.k, lo, hi)
    y = moe.fused_moe(x.to(DEV), router.to(DEV), w13.to(DEV), w2.to(DEV), case.k, lo, hi, defer_combine=defer)
    decode = case.T <= 64 and (2 * case.I) % 128 == 0
    assert isinstance(y, moe.PendingCombine) == (defer and decode)
    if isinstance(y, moe.PendingCombine):
        y = y.combine()
    report("moe", mc.check_moe(y.cpu(), ref, B))
