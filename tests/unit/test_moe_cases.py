"""CPU proof that the exact MoE tests (tests/kernels/test_moe_exact.py) can fail: the float64
references of tests/moe_cases.py agree with the CPU fallbacks of ops/moe.py, every input table meets
what its docstring promises, and for every case of the GPU tables the unmutated reference passes the
criterion the GPU test applies while every mutant of it is rejected.

A mutant that cannot differ from the reference on a case is skipped there by a rule stated next to
it (a tie mutant needs k < E or two tied ids inside the top k, a renormalisation mutant needs k < E
because the weights of all experts already sum to 1, and so on); every mutant is rejected on at least
one case of its table."""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import gemm, gemm_prefill, moe
from tests import moe_cases as mc

BF = torch.bfloat16


def rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("T,E,k", mc.ROUTE_CASES)
def test_grid_logits_and_route_mutants(T, E, k):
    lg = mc.grid_logits(T, E, k, seed=T + E)
    v = lg.double()
    fin = torch.isfinite(v)
    assert bool(fin.any(-1).all()), "a row without a finite logit"
    assert bool((v[fin] * 8 == torch.round(v[fin] * 8)).all()) and float(v[fin].abs().max()) <= 16
    assert torch.equal(lg.double().to(BF), lg)
    if T >= 5:
        assert bool((~fin).any())
    # the planted tie of row 0 sits across the k-th place (k == E: inside the top k)
    top = torch.sort(v[0], descending=True).values
    a = min(k, E - 1)
    assert top[a] == top[a - 1]
    for renorm in (True, False):
        ids, w = mc.route64(lg, k, renorm)
        assert mc.check_route(ids, w.float(), lg, k, renorm) <= 2.0 ** -24
        rejects(mc.check_route, *mc.route64(lg, k, renorm, tie_high=True), lg, k, renorm)
        if k < E:  # over all E experts the weights sum to 1 with or without renormalisation
            rejects(mc.check_route, *mc.route64(lg, k, not renorm), lg, k, renorm)
        bad = ids.clone()
        bad[0, 0] = bad[0, -1] if k > 1 else (bad[0, 0] + 1) % E
        rejects(mc.check_route, bad, w, lg, k, renorm)
        if k >= 2:
            rejects(mc.check_route, ids, w[:, [1, 0] + list(range(2, k))], lg, k, renorm)
        rejects(mc.check_route, ids, w * (1 + 2 * mc.W_RTOL), lg, k, renorm)
        # the CPU fallback of ops/moe.py is the same function
        ids_o, w_o = moe.topk_softmax(lg, k, renorm)
        mc.check_route(ids_o, w_o, lg, k, renorm, rtol=1e-5)
    # a kernel that ignored the stride would read the +16 padding
    buf = mc.strided(lg)
    assert buf.stride(0) > E and torch.equal(buf[:, 2:2 + E], lg)
    flat = buf.reshape(-1)[2:2 + T * E].reshape(T, E)
    if T > 1:
        rejects(mc.check_route, *mc.route64(flat, k, True), lg, k, True)


def test_w_rtol_is_below_the_old_ceiling():
    assert mc.W_RTOL <= 1e-5


@pytest.mark.parametrize("T,E,k", mc.ROUTE_CASES)
def test_route_norm_case_is_exact(T, E, k):
    S = 2 if T % 2 else 4
    slabs, res, nw, router, v, x, logits = mc.route_norm_case(T, E, T + E + k, S)
    r = (slabs.double().sum(0).to(BF).double() + res.double()).to(BF)
    assert torch.equal(r, v)
    assert torch.equal(mc.rmsnorm64(r, nw, 0.0).to(BF), x)
    lg64 = x.double() @ router.double().t()
    assert torch.equal(lg64.to(BF).double(), lg64) and torch.equal(lg64.to(BF), logits)
    # fp32 in another order gives the same integers
    assert torch.equal((x.float().flip(-1) @ router.float().flip(-1).t()).double(), lg64)
    ids, w = mc.route64(logits, k, True)
    mc.check_route(ids, w, logits, k, True)
    if E > 8 or T > 8:
        assert bool((torch.sort(lg64, -1).values.diff(dim=-1) == 0).any()), "no tied logits in the case"
        rejects(mc.check_route, *mc.route64(logits, k, True, tie_high=True), logits, k, True)


# --------------------------------------------------------------------------------------- align
@pytest.mark.parametrize("case", mc.ALIGN_CASES, ids=lambda c: c.name)
def test_align_cases_and_mutants(case):
    ids = case.ids()
    n, lo, hi = case.n, case.e_lo, case.e_hi
    off, srt, inv = mc.align_ref(ids, lo, hi)
    m = int(off[-1])
    full = np.full(n, mc.SENT_I, dtype=np.int64)
    full[:m] = srt
    mc.check_align(off, full, inv, ids, lo, hi)
    o2, s2, i2 = moe.align(torch.from_numpy(ids), case.E, lo, hi)
    assert np.array_equal(o2.numpy(), off) and np.array_equal(s2.numpy(), srt) and np.array_equal(i2.numpy(), inv)
    local = (ids >= lo) & (ids < hi)
    if case.kind == "mixed" and n > 100:
        assert (ids == -1).any() and (ids == case.E + 3).any()
    if case.kind == "one":
        assert m == n
    if case.kind == "none":
        assert m == 0 and n > 0
    if n and np.bincount(ids[local] - lo, minlength=1).max(initial=0) >= 2:   # an expert with two slots
        o, s, i = mc.align_ref(ids, lo, hi, unstable=True)
        f = full.copy()
        f[:m] = s
        rejects(mc.check_align, o, f, i, ids, lo, hi)
    if (~local).any():
        o, s, i = mc.align_ref(ids, lo, hi, keep_nonlocal=True)
        rejects(mc.check_align, o, s, i, ids, lo, hi)
    if m < n:
        f = full.copy()
        f[m] = 0
        rejects(mc.check_align, off, f, inv, ids, lo, hi)


def test_align_table_covers_the_edges():
    assert {c.n for c in mc.ALIGN_CASES} >= {0, 1, 1023, 1024, 1025, 2049}
    assert {c.e_hi - c.e_lo for c in mc.ALIGN_CASES} >= {1, 8, 64}
    assert any(c.e_lo > 0 for c in mc.ALIGN_CASES) and {c.kind for c in mc.ALIGN_CASES} == {"mixed", "one", "none"}


# --------------------------------------------------------------------------- permute / combine
COMBINE_SHAPES = [(5, k, H) for k in (1, 2, 4) for H in (8, 1024, 2056)]


@pytest.mark.parametrize("T,k,H", COMBINE_SHAPES)
@pytest.mark.parametrize("integer", [True, False])
def test_combine_reference_and_mutants(T, k, H, integer):
    y, inv, w = mc.combine_case(T, k, H, integer, seed=T + k + H)
    assert bool((inv == -1).any()) and bool((inv.view(T, k)[1] == -1).all())
    ref, mag = mc.combine64(y, inv, w, T, k)
    assert bool((ref[1] == 0).all())
    out = moe.unpermute(y, inv, w, T, k)   # the CPU fallback: fp32 accumulate, one bf16 rounding
    if integer:
        assert float(ref.abs().max()) <= 16 and torch.equal(ref.to(BF).double(), ref)
        mc.check_exact(out, ref)
        judge = lambda o: mc.check_exact(o.to(BF), ref)
    else:
        assert mc.check_combine(out, ref, mag, k) <= 1.0
        judge = lambda o: mc.check_combine(o.to(BF), ref, mag, k)
    judge(ref)
    if k >= 2:
        rejects(judge, mc.combine64(y, inv, w, T, k, swap=True)[0])
    rejects(judge, mc.combine64(y, inv, w, T, k, keep_nonlocal=True)[0])
    rejects(judge, mc.combine64(y, inv, w, T, k, shift=True)[0])


def test_permute_reference():
    x = torch.arange(7 * 8, dtype=torch.float32).view(7, 8).to(BF)
    ids = np.array([[0, 3], [2, 9], [3, 1], [-1, 2], [0, 2], [9, 9], [1, 0]], dtype=np.int32)
    off, srt, inv = mc.align_ref(ids, 0, 3)
    got = moe.permute(x, torch.from_numpy(srt).int(), torch.from_numpy(off).int(), 2)
    assert torch.equal(got, mc.permute_ref(x, srt, 2))
    assert torch.equal(mc.permute_ref(x, srt, 2)[:, 0].float() / 8, torch.tensor([0., 4, 6, 2, 6, 1, 3, 4]))


def test_rmsnorm64():
    r = torch.tensor([[3.0, -4.0, 0.0, 0.0]])
    assert torch.allclose(mc.rmsnorm64(r, torch.tensor([1.0, 2.0, 1.0, 1.0]), 0.0),
                          torch.tensor([[1.2, -3.2, 0.0, 0.0]], dtype=torch.float64))


# --------------------------------------------------------------------------------- grouped GEMM
ALL_GEMM = mc.MOE_GEMM_CASES + mc.SKINNY_CASES + mc.PREFILL_CASES


def test_gemm_tables_hold_the_named_group_sizes():
    assert {s for c in mc.MOE_GEMM_CASES for s in c.sizes} >= {0, 1, 16, 17, 32, 48, 64}
    assert {c.max_rows for c in mc.MOE_GEMM_CASES} == {16, 32, 48, 64} and {c.K for c in mc.MOE_GEMM_CASES} == {128, 384}
    assert {s for c in mc.SKINNY_CASES for s in c.sizes} >= {0, 1, 15, 16, 17, 64, 65, 128}
    assert {(c.N, c.K) for c in mc.SKINNY_CASES} == {(N, 256 * S) for N in (128, 256) for S in (1, 2, 4)}
    assert all(c.sizes == (255, 0, 256, 257, 1) and c.tail == 5 for c in mc.PREFILL_CASES)
    assert {c.K for c in mc.PREFILL_CASES} == {64, 192, 128, 512}
    assert all(max(c.sizes) <= c.max_rows for c in ALL_GEMM)


def test_interleave_matches_the_package():
    g = torch.arange(64 * 4, dtype=torch.float32).view(64, 4)
    u = -g
    assert torch.equal(mc.interleave(g, u), gemm.interleave_gate_up(g, u))
    gg, uu = mc.deinterleave(mc.interleave(g, u).t().contiguous())
    assert torch.equal(gg, g.t()) and torch.equal(uu, u.t())


@pytest.mark.parametrize("case", ALL_GEMM, ids=lambda c: c.id)
def test_gemm_case_is_exact_and_mutants_are_rejected(case):
    A, W, offs = case.build()   # asserts |sum| <= 256 and gate sums >= -80
    R, m = A.shape[0], int(offs[-1])
    assert bool(torch.isnan(A[m:]).all()) and A.shape[0] - m == case.tail
    assert all(bool(torch.isnan(W[e]).all()) == (s == 0) for e, s in enumerate(case.sizes))
    full = mc.grouped64(A, W, offs)
    ref = mc.with_sentinel(full)
    assert torch.equal(torch.nan_to_num(full).to(BF).double(), torch.nan_to_num(full)), "not exact in bf16"
    mc.check_exact(ref.to(BF), ref)
    sref = mc.with_sentinel(mc.silu_ref(full))
    live = sref != mc.SENT
    assert float(sref[live].abs().min()) == 0 or float(sref[live & (sref != 0)].abs().min()) > 1e-30

    def judge_silu(o):
        return mc.check_rel(o.to(BF), sref, 2.25, "silu")

    # the bf16 emulation of the epilogue passes, with room: bf16(bf16(silu(g)) * u)
    g, u = mc.deinterleave(full)
    emu = mc.with_sentinel(mc.bf(mc.bf(mc.silu64(g)) * u))
    assert mc.check_rel(emu, sref, 2.25, "silu") <= 2.0
    for name, mut in mc.gemm_mutants(case, A, W, offs).items():
        rejects(mc.check_exact, mc.with_sentinel(mut).to(BF), ref, name)
        rejects(judge_silu, mc.with_sentinel(mc.silu_ref(mut)))
    rejects(judge_silu, mc.with_sentinel(mc.silu_ref(full, swap=True)))
    rejects(judge_silu, mc.with_sentinel(mc.silu_ref(full, block=8)))
    # a row outside every group written, a row of a group left at the sentinel
    bad = ref.clone()
    bad[m:] = 1.0
    rejects(mc.check_exact, bad, ref)
    if case in mc.SKINNY_CASES and case.K > 256:
        S = case.K // 256
        slabs = mc.slab_refs(A, W, offs, S)
        assert torch.equal(torch.nan_to_num(slabs.sum(0)), torch.nan_to_num(full))
        sl = mc.with_sentinel(slabs)
        mc.check_exact(sl.float(), sl)
        rejects(mc.check_exact, mc.with_sentinel(mc.slab_refs(A, W, offs, S, shift=8)).float(), sl)
    if case in mc.PREFILL_CASES:   # the CPU fallback of the prefill GEMM
        a0, w0 = torch.nan_to_num(A), torch.nan_to_num(W)
        y = gemm_prefill.grouped_linear(a0, w0, offs)
        assert torch.equal(y[:m].double(), full[:m])
        h = gemm_prefill.grouped_linear(a0, w0, offs, silu=True)
        mc.check_rel(h[:m], mc.silu_ref(full)[:m], 2.25, "silu")


GATHER_SHAPES = [(24, k, N, K) for k in (1, 2, 4) for N, K in ((128, 256), (256, 512))]


@pytest.mark.parametrize("T,k,N,K", GATHER_SHAPES)
def test_gather_case(T, k, N, K):
    x, W, ids, offs, srt, A = mc.gather_case(T, k, 6, 1, 5, N, K, seed=T + k + N)
    m = int(offs[-1])
    assert 0 < m < T * k and A.shape[0] == T * k
    assert torch.equal(torch.nan_to_num(mc.permute_ref(x, srt, k)), torch.nan_to_num(A[:m]))
    used = set((srt.long() // k).tolist())
    assert all(bool(torch.isnan(x[t]).all()) != (t in used) for t in range(T))
    if k == 1:
        assert len(used) < T, "every token is read by a local slot"
    full = mc.grouped64(A, W, offs)
    # reading row sorted[p] instead of sorted[p] // k, or rows in slot order, changes the integers
    if k > 1:
        wrong = torch.cat([torch.nan_to_num(x)[srt.long() % T], A[m:]])
        rejects(mc.check_exact, mc.with_sentinel(mc.grouped64(wrong, W, offs)).to(BF), mc.with_sentinel(full))


# ---------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", mc.MOE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("ep", mc.EP_RANGES)
def test_moe_case_and_mutants(case, ep):
    lo, hi = ep
    x, router, w13, w2 = case.build(lo, hi)
    E, k = case.E, case.k
    lg = x[:, :E].double()
    assert torch.equal(x.double() @ router.double().t(), lg)
    top = torch.sort(lg, -1, descending=True).values
    assert bool((top[:, 0] - top[:, 1] >= 1).all()) and bool((top.diff(dim=-1) <= -0.125).all())
    assert bool((torch.nan_to_num(w13)[:, :, :E] == 0).all())
    ref, B = mc.moe64(x, router, w13, w2, k, lo, hi)
    ids, wts = mc.route64(lg, k, True)
    none_local = ~((ids >= lo) & (ids < hi)).any(-1)
    assert bool((B[none_local] == 0).all()) and (hi - lo == E or bool(none_local.any()))
    # the package's reference with the kernels' rounding points (NaN experts are never routed to)
    pk = moe.fused_moe_reference(x, router, torch.nan_to_num(w13), torch.nan_to_num(w2), k, lo, hi)
    ratio = mc.check_moe(pk.to(BF), ref, B)
    assert ratio <= 4.25
    local_tokens = ~none_local

    def every_local_token_over(mut):
        err = (mut.to(BF).double() - ref).abs()
        return bool(((err > 4.25 * mc.U * B).any(-1) | ~local_tokens).all())

    for kw in ("renorm", "swap"):
        mut = mc.moe64(x, router, w13, w2, k, lo, hi, **({"renorm": False} if kw == "renorm" else {"swap": True}))[0]
        rejects(mc.check_moe, mut.to(BF), ref, B)
        assert every_local_token_over(mut), kw
    if hi - lo > 1:
        rejects(mc.check_moe, mc.moe64(x, router, w13, w2, k, lo, hi, next_expert=True)[0].to(BF), ref, B)
    rejects(mc.check_moe, mc.moe64(x, router, w13, w2, k, lo, hi, gate_up_swap=True)[0].to(BF), ref, B)
    rejects(mc.check_moe, mc.moe64(x, router, w13, w2, k, lo, hi, shift=True)[0].to(BF), ref, B)
    if hi - lo < E:
        rejects(mc.check_moe, mc.moe64(x, router, w13, w2, k, lo, hi, keep_nonlocal=True)[0].to(BF), ref, B)
