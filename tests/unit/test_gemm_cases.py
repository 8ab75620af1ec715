"""The dense GEMM cases (tests/gemm_cases.py) on the CPU: every builder keeps its exactness budget,
every reference satisfies its own criterion, every mutant -- a reference with one of the bugs a
kernel could have -- is rejected by at least one case of the set tests/kernels/test_gemm_exact.py
runs on the GPU, and the CPU paths of ``ops`` agree with the references."""
import pytest
import torch

from tests import gemm_cases as gc

BF16 = torch.bfloat16
ROWS_CPU = [1, 17, 64]  # a subset of gc.ROWS: what rejects here is rejected on the GPU too


# ------------------------------------------------------------------------------------- budgets
@pytest.mark.parametrize("cls", ["small", "rounding"])
@pytest.mark.parametrize("N,K", gc.SHAPES)
def test_grid_budgets(N, K, cls):
    for M in gc.ROWS + gc.ROWS_TILED:
        for make in (gc.grid_case, gc.silu_case):
            c = make(N, K, M, 0, cls)  # asserts integrality, sum |x||w| < 2^24 and its class
            acc = gc.ref_acc(c)
            assert float(acc.abs().max()) < 2 ** 24 and bool((acc == acc.round()).all())
            for S in gc.splits(K):
                assert gc.same_bits(gc.ref_slabs(c, S).sum(0), acc)
        if M <= 64:
            for half in (False, True):
                for seed in (0, 1):
                    gc.residual_case(N, K, M, seed, cls, 64 if half else 128)


def test_long_k_budget():
    N, K = gc.LONG_SHAPE
    for M in (1, 64):
        c = gc.grid_case(N, K, M)
        acc = gc.ref_acc(c)
        assert 256 < float(acc.abs().max()) < 2 ** 24
        # the budget stated with the case family: x, w in [-4, 4] at K = 14336 stays far below 2^24
        assert float((c.x.double().abs() @ c.w.double().abs().t()).max()) <= 16 * K


def test_small_class_budget():
    """x in {-1, 0, 1}, w in [-2, 2], K = 1024, residual in [-8, 8]: a new residual of magnitude
    <= 256 + 8 whose 128-column sums of squares are integers below 2^24."""
    c, r = gc.residual_case(384, 1024, 64, 0, "small")
    new, parts = gc.ref_add_residual(gc.ref_acc(c), r, 128)
    assert float(new.abs().max()) <= 264 and float(parts.max()) < 2 ** 24
    assert bool((parts == parts.round()).all()) and gc.is_bf16(new)


@pytest.mark.parametrize("nparts", gc.NPARTS)
def test_norm_budgets(nparts):
    for (N, K) in gc.SHAPES:
        for M in gc.ROWS:
            c, nw, parts = gc.norm_case(N, K, M, 0, nparts)  # asserts the power-of-two prologue
            assert int((parts != 0).sum()) == M and parts.shape == (nparts, M)
            rinv = gc.ref_rinv(parts, K)
            j = (torch.arange(M) % 4).double()
            assert bool(((rinv * 2.0 ** j - 1.0).abs() < 2.0 ** -17).all())
    for M in (1, 64, 200):
        p = gc.int_parts(M, nparts)
        assert bool((p == p.round()).all()) and float(p.sum(0).max()) < 2 ** 24


def test_rope_table_is_exact():
    cs = gc.rope_table()
    pairs = {(float(c), float(s)) for c, s in zip(cs[:, :64].reshape(-1), cs[:, 64:].reshape(-1))}
    assert pairs == set(gc.ROPE_PAIRS)
    # varies per position and per dimension
    assert all(not torch.equal(cs[p], cs[p + 1]) for p in range(64))
    assert all(not torch.equal(cs[:, d], cs[:, d + 1]) for d in range(63))
    # integer pre-activations: every product and both sums are exact in fp32, contracted or not
    v = torch.randint(-256, 257, (64, 3, 128), generator=torch.Generator().manual_seed(1)).double()
    pos = gc.rope_positions(64)
    assert len(set(pos.tolist())) == 64
    t = cs.double()[pos.long()]
    a, b, co, si = v[..., :64], v[..., 64:], t[:, None, :64], t[:, None, 64:]
    for e in (a * co, b * si, a * co - b * si, b * co + a * si):
        assert bool((e.float().double() == e).all())
    assert gc.same_bits(gc.ref_rope(v, pos, cs), gc.bf(torch.cat([a * co - b * si, b * co + a * si], -1)))


@pytest.mark.parametrize("H", [1024, 3072, 8192])
def test_addnorm_budget(H):
    for S in (1, 2, 4, 8):
        slabs, r, nw, new, x = gc.addnorm_case(17, H, S)  # asserts the construction
        assert gc.is_bf16(new) and gc.is_bf16(x) and float(slabs.abs().max()) <= 8


def test_select_down():
    w, k, v = gc.select_down(1024, 12288, 16)
    assert int((w != 0).sum()) == 16 * 1024
    h = torch.randint(-50, 51, (5, 12288), generator=torch.Generator().manual_seed(3)).double()
    c = gc.Case(h.to(BF16), w)
    slabs = gc.ref_slabs(c, 16)
    for s in (0, 7, 15):
        assert bool((k[s] // 768 == s).all())
        assert gc.same_bits(slabs[s], h[:, k[s]] * v[s][None, :])


# -------------------------------------------------------------- references meet their own criteria
def test_references_satisfy_their_criteria():
    c = gc.silu_case(256, 512, 17)
    acc = gc.ref_acc(c)
    assert gc.same_bits(gc.ref_bf16(c), gc.bf(acc)) and gc.is_bf16(gc.ref_bf16(c))
    iv = gc.ref_silu(acc)
    g, u = gc.split_gate_up(acc)
    mid = gc.bf(gc.bf(gc.silu64(gc.bf(g))) * gc.bf(u))
    assert gc.inside(mid, iv) and gc.is_bf16(iv[0]) and gc.is_bf16(iv[1])
    assert bool((iv[0][:, 16:32] == 0).all()) and bool((iv[1][:, 16:32] == 0).all())  # the anchor
    # the intervals are tight: at most neighbouring bf16 values
    width = (iv[1] - iv[0]).abs()
    assert bool((width <= 2.0 ** -7 * torch.maximum(iv[0].abs(), iv[1].abs()) + 1e-30).all())
    # row scale
    parts = gc.int_parts(17, 3)
    rinv = gc.ref_rinv(parts, c.K)
    slabs = gc.ref_slabs(c, 2)
    ref = acc * rinv[:, None]
    err = gc.rowscale_err(slabs, rinv)
    assert gc.within_rel(ref.float(), ref, err + 0.5 * gc.U * ref.abs())  # fp32 storage alone
    assert gc.inside(gc.bf(gc.bf(gc.silu64(gc.bf(gc.split_gate_up(ref)[0]))) * gc.bf(gc.split_gate_up(ref)[1])),
                     gc.ref_silu(ref, err))
    # residual update and parts
    for cls in ("small", "rounding"):
        cr, r = gc.residual_case(256, 512, 17, 0, cls)
        new, p = gc.ref_add_residual(gc.ref_acc(cr), r, 128)
        assert gc.is_bf16(new) and gc.within_rel(p, p, gc.parts_err(p, 128, cls))
        assert gc.within_rel(new.float().view(17, 2, 128).pow(2).sum(-1).t(), p, gc.parts_err(p, 128, cls))


def test_silu_overflow_floor():
    """Gate values where __expf overflows (the kernel returns -0) and a zero gate."""
    g = torch.tensor([[-120.0, -100.0, -89.0, 0.0, 30.0, -1.25, -1.3125]]).double()
    lo, hi = gc.iv_bf(gc.iv_silu((g, g)))
    assert bool((lo[0, :3] <= 0).all()) and bool((hi[0, :3] >= 0).all())   # -0 is accepted
    assert float(lo[0, 3]) == 0.0 and float(hi[0, 3]) == 0.0                 # exactly 0
    assert float(lo[0, 4]) == 30.0 and float(hi[0, 4]) == 30.0
    # an interval straddling the minimum of silu contains the minimum
    lo2, hi2 = gc.iv_silu((torch.tensor([-1.3125]).double(), torch.tensor([-1.25]).double()))
    assert float(lo2) <= float(gc.silu64(torch.tensor(gc.SILU_ARGMIN).double())) <= float(hi2)


# -------------------------------------------------------------------------------------- mutants
def _gemm_rejects(mutant: str) -> bool:
    """Some grid case of the GPU set at which the mutant's slabs differ from the reference's."""
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU:
            c = gc.grid_case(N, K, M)
            for S in gc.splits(K):
                if not gc.same_bits(gc.ref_slabs(c, S, mutant), gc.ref_slabs(c, S)):
                    return True
    return False


def _bf16_rejects(mutant: str) -> bool:
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU:
            c = gc.grid_case(N, K, M)
            if not gc.same_bits(gc.expect_buf(gc.ref_bf16(c, 1, mutant), mutant=mutant), gc.expect_buf(gc.ref_bf16(c))):
                return True
    return False


def _needle_rejects(mutant: str) -> bool:
    N, K, M = 256, 2048, 17
    for S in gc.splits(K):
        for (n, k, m) in gc.decode_needle_points(N, K, M, S):
            c = gc.needle_case(N, K, M, n, k, m)
            if not gc.same_bits(gc.ref_slabs(c, S, mutant), gc.ref_slabs(c, S)):
                return True
    return False


@pytest.mark.parametrize("mutant", ["kblock_swap", "kstep_swap", "kchunk_swap", "tile16_swap", "half64_swap"])
def test_layout_mutants_rejected(mutant):
    assert mutant in gc.MUTANTS
    assert _gemm_rejects(mutant) and _bf16_rejects(mutant) and _needle_rejects(mutant)


@pytest.mark.parametrize("mutant", ["drop_last_split", "split_shift"])
def test_split_mutants_rejected(mutant):
    assert mutant in gc.MUTANTS
    assert _gemm_rejects(mutant) and _needle_rejects(mutant)
    # a shifted boundary keeps the sum: only the slab-by-slab comparison sees it
    c = gc.grid_case(256, 2048, 17)
    assert gc.same_bits(gc.ref_acc(c, 4, "split_shift"), gc.ref_acc(c, 4))


def test_row_leak_rejected():
    assert _bf16_rejects("row_leak")
    c = gc.silu_case(256, 512, 17)
    iv = gc.ref_silu(gc.ref_acc(c))
    leak = gc.iv_pad(iv, mutant="row_leak")
    assert not gc.inside(leak[0], gc.iv_pad(iv))


@pytest.mark.parametrize("mutant", ["gate_up_swap", "gate_next_up"])
@pytest.mark.parametrize("cls", ["small", "rounding"])
def test_silu_mutants_rejected(mutant, cls):
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU:
            acc = gc.ref_acc(gc.silu_case(N, K, M, 0, cls))
            assert gc.disjoint(gc.ref_silu(acc, mutant=mutant), gc.ref_silu(acc)), (N, K, M)


def test_residual_mutants_rejected():
    hit = {"round_once": False, "parts_old": False, "parts_next_row": False}
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU:
            for nblk in (128, 64):
                for cls in ("small", "rounding"):
                    c, r = gc.residual_case(N, K, M, 0, cls, nblk)
                    acc = gc.ref_acc(c)
                    new, parts = gc.ref_add_residual(acc, r, nblk)
                    err = gc.parts_err(parts, nblk, cls)
                    for mutant in hit:
                        n2, p2 = gc.ref_add_residual(acc, r, nblk, mutant)
                        bad = not gc.same_bits(n2, new) or not gc.within_rel(p2, parts, err)
                        hit[mutant] |= bad
                        if mutant == "round_once":
                            assert bad == (cls == "rounding"), (N, K, M, cls)  # only that class can tell
                        if mutant == "parts_old" or (mutant == "parts_next_row" and M > 1):
                            assert bad, (mutant, N, K, M, cls)
    assert all(hit.values()), hit


@pytest.mark.parametrize("mutant", ["rinv_div_n", "rinv_next_row", "normw_shift8"])
def test_norm_in_mutants_rejected(mutant):
    hit = False
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU:
            for nparts in (1, 3):
                c, nw, parts = gc.norm_case(N, K, M, 0, nparts)
                good = gc.ref_acc(c, x=gc.ref_norm_in(c.x, gc.ref_rinv(parts, K), nw))
                rinv = gc.ref_rinv(parts, K, mutant=mutant, N=N)
                bad = gc.ref_acc(c, x=gc.ref_norm_in(c.x, rinv, nw, mutant))
                rejected = not gc.same_bits(gc.bf(bad), gc.bf(good))
                hit |= rejected
                if mutant == "normw_shift8" or (mutant == "rinv_next_row" and M > 1) or (mutant == "rinv_div_n" and N != K):
                    assert rejected, (N, K, M, nparts)
    assert hit


@pytest.mark.parametrize("mutant", ["rinv_div_n", "rinv_next_row"])
def test_rowscale_mutants_rejected(mutant):
    hit = False
    for (N, K) in gc.SHAPES:
        for M in ROWS_CPU + [200]:
            for nparts in (1, 16, 64):
                c = gc.grid_case(N, K, M, 0, "small")
                parts = gc.int_parts(M, nparts)
                for S in gc.splits(K):
                    slabs = gc.ref_slabs(c, S)
                    good, bad = gc.ref_rinv(parts, K), gc.ref_rinv(parts, K, mutant=mutant, N=N)
                    err = gc.DELTA_R * (slabs * good[None, :, None]).abs()
                    rejected = not gc.within_rel(slabs * bad[None, :, None], slabs * good[None, :, None], err)
                    hit |= rejected
                    if (mutant == "rinv_next_row" and M > 1) or (mutant == "rinv_div_n" and N != K):
                        assert rejected, (N, K, M, nparts, S)
    assert hit


ROPE_MUTANTS = ["rope_halves_swapped", "sin_flip", "pos_next_row", "khead_next", "v_untransposed", "slot_neg_cached"]


@pytest.mark.parametrize("mutant", ROPE_MUTANTS)
def test_qkv_mutants_rejected(mutant):
    assert mutant in gc.MUTANTS
    cs = gc.rope_table()
    hit = False
    for (nq, nkv, bs) in gc.QKV_HEADS:
        for M in ROWS_CPU:
            c = gc.qkv_case(nq, nkv, 256, M)
            acc = gc.ref_acc(c)
            pos = gc.rope_positions(M)
            slots, nb = gc.cache_slots(M, bs)
            assert 0 not in slots.tolist() and (M == 1 or -1 in slots.tolist())
            assert M == 1 or len({int(s) // bs for s in slots if s >= 0}) > 1  # crosses a block
            good = gc.ref_qkv(acc, pos, cs, slots, nq, nkv, bs, nb)
            bad = gc.ref_qkv(acc, pos, cs, slots, nq, nkv, bs, nb, mutant=mutant)
            rejected = any(not gc.same_bits(a, b) for a, b in zip(good, bad))
            hit |= rejected
            trivial = ((mutant == "khead_next" and nkv == 1) or (mutant in ("pos_next_row", "slot_neg_cached") and M == 1))
            assert rejected or trivial, (nq, nkv, bs, M)
    assert hit


def test_every_mutant_has_a_test():
    covered = {"kblock_swap", "kstep_swap", "kchunk_swap", "tile16_swap", "half64_swap", "drop_last_split",
               "split_shift", "row_leak", "gate_up_swap", "gate_next_up", "round_once", "parts_old", "parts_next_row",
               "rinv_div_n", "rinv_next_row", "normw_shift8"} | set(ROPE_MUTANTS)
    assert covered == set(gc.MUTANTS)


def test_needle_points_cover_the_corners():
    pts = gc.decode_needle_points(256, 2048, 64, 4)
    assert {p[0] for p in pts} == {0, 15, 16, 63, 64, 127, 128, 255}
    assert {p[1] for p in pts} == {0, 7, 8, 31, 32, 127, 128, 255, 256, 511, 512, 2047}
    assert {p[2] for p in pts} == {0, 15, 16, 63}
    pts = gc.prefill_needle_points(513, 512, 1024)
    assert {p[2] for p in pts} == {0, 15, 16, 127, 128, 255, 256, 512}
    assert {p[0] for p in pts} == {0, 15, 16, 127, 128, 255, 256, 511}
    assert {p[1] for p in pts} == {0, 7, 8, 63, 64, 127, 128, 1023}
    for (n, k, m) in pts[:5]:
        c = gc.needle_case(512, 1024, 513, n, k, m)
        acc = gc.ref_acc(c)
        assert int((acc != 0).sum()) == 1 and float(acc[m, n]) == -4.5


# ------------------------------------------------------------------------ the CPU paths of ``ops``
@pytest.mark.parametrize("S", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("H", [512, 1536])
def test_ops_residual_parts_cpu(S, H):
    from polykey_service_amd.ops import gemm
    M = 17
    r = torch.randint(-8, 9, (M, H), generator=torch.Generator().manual_seed(S + H)).double()
    slabs = gc.int_slabs(max(S, 1), M, H, 0, mag=40)
    acc = slabs.double().sum(0) if S else torch.zeros((M, H), dtype=torch.float64)
    new, parts = gc.ref_add_residual(acc, r, 512)
    res = r.to(BF16)
    buf = torch.full((H // 512 * M + 8,), float("nan"))
    got = gemm.residual_parts(gemm.Partial(slabs.reshape(-1), S, M, H) if S else None, res, buf)
    assert gc.same_bits(res, new) and gc.same_bits(got, parts) and bool(buf[H // 512 * M:].isnan().all())


@pytest.mark.parametrize("packed", [False, True])
def test_ops_prefill_linear_cpu(packed):
    from polykey_service_amd.ops import gemm, gemm_prefill
    c = gc.silu_case(256, 320 if not packed else 384, 37)
    wp = gemm.pack_weight(c.w) if packed else None
    assert gc.same_bits(gemm_prefill.linear(c.x, c.w, packed=wp), gc.ref_bf16(c))
    assert gc.inside(gemm_prefill.linear(c.x, c.w, silu=True, packed=wp), gc.ref_silu(gc.ref_acc(c)))
