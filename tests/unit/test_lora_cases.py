"""The LoRA kernel cases (tests/lora_cases.py) on the CPU: they are exact, asymmetric, reject every
mutant of the contract, and the fp32 reference ops (ops/reference.py, the CPU branch of ops/lora.py)
pass them bit for bit -- so a GPU kernel that passes them computes the contract."""
import pytest
import torch

from polykey_service_amd.ops import lora as lora_ops
from polykey_service_amd.ops.gemm import RowScale
from tests import lora_cases as lc

FORMS = ("slab", "bf16")


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality of values, NaN == NaN."""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=-12345.0),
                                              torch.nan_to_num(b.double(), nan=-12345.0))


def run_ops(c: lc.Case, form: str, init: torch.Tensor):
    """shrink + expand through ops/lora.py (here: its CPU branch) -> (t, buffer)."""
    t = torch.full((c.M * c.R + 16,), float("nan"), dtype=torch.bfloat16)
    rs = None if c.parts is None else RowScale(c.parts, c.eps)
    tv = lora_ops.shrink(c.x, c.A, c.idx, t, c.seg_r, ranks=c.ranks, rowscale=rs)
    out = init.clone()
    lora_ops.expand(out[0] if form == "slab" else out, tv, c.B, c.scale, c.idx, lora_ops.Segments(*c.seg),
                    ranks=c.ranks)
    return tv, out


SUBSET = [(kind, K, r) for kind in lc.KINDS for K in lc.KS for r in lc.RANKS]


@pytest.mark.parametrize("kind,K,r", SUBSET)
def test_grid_cases_are_exact_and_the_reference_ops_pass_them(kind, K, r):
    for c in lc.grid_cases(kind, K, r)[1::2] + lc.grid_cases(kind, K, r)[:1]:
        valid = c.idx >= 0
        sig = lc.sums_f64(c, c.idx)[valid]
        assert sig.numel() == 0 or sig.abs().max() < 2 ** 24  # integers: exact in fp32 in any order
        t = lc.reference_t(c)
        assert torch.isnan(t[~valid]).all() and not torch.isnan(t[valid]).any()
        if c.parts is None:
            assert torch.equal(t[valid], sig), "t must be exactly representable in bf16"
        elif c.M >= 16:
            assert not torch.equal(t[valid], (sig.float() * lc.rinv_fp32(c)[valid][:, None]).double()), \
                "the row-scale cases must need the rounding"
        # expand sums: multiples of 2^-3 (t: 2^-2 with a row scale, B: 2^-1) below 2^24 such units
        cols = lc.col_segments(c.N, c.seg)[:, None] * c.seg_r + torch.arange(c.seg_r)[None, :]
        for m in torch.nonzero(valid).flatten().tolist():
            tot = (c.B[int(c.idx[m])].double().abs() * t[m].abs()[cols]).sum(-1).max()
            assert tot * 8 + 8 * 8 < 2 ** 24
        assert torch.equal((t[valid] * 4).round(), t[valid] * 4)
        for form in FORMS:
            init = lc.initial_out(c, form)
            want = lc.reference_out(c, form, init)
            tv, got = run_ops(c, form, init)
            assert _same(tv, t.to(torch.bfloat16)), c.name
            assert _same(got, want), (c.name, form)
            # rows without a slot and (slab form) slab 1 are untouched
            keep = got[0] if form == "slab" else got
            assert torch.equal(keep[~valid], (init[0] if form == "slab" else init)[~valid])
            if form == "slab":
                assert torch.equal(got[1], init[1])


def test_cases_are_asymmetric():
    for kind in lc.KINDS:
        c = lc.grid_case(kind, 512, 16, 17, rowscale=True)
        assert (c.idx[:8].tolist()) == [-1, 0, 2, 1, -1, 0, 2, 1]  # no uniform row tile
        assert torch.isnan(c.x[c.idx < 0]).all()
        assert c.x.stride(0) == c.K + 8
        rk = [int(v) for v in c.ranks]
        for s in range(lc.SLOTS):
            for sg in range(c.nseg):
                a = c.A[s, sg * c.seg_r: sg * c.seg_r + rk[s]].float()
                assert len({tuple(row.tolist()) for row in a}) == rk[s], "A rows alike"
                assert (c.A[s, sg * c.seg_r + rk[s]:(sg + 1) * c.seg_r] == 0).all()  # zero, NaN-free padding
                assert a[-1, 0] != 0 and a[-1, -1] != 0  # the first and the last k column count
            assert (c.B[s, :, rk[s]:] == 0).all() and (c.B[s, :, rk[s] - 1] != 0).all()
        # slots differ, and so do the sub-projections' blocks of one slot
        assert not torch.equal(c.A[0], c.A[1]) and not torch.equal(c.A[0], c.A[2]) and not torch.equal(c.A[1], c.A[2])
        assert not torch.equal(c.B[0], c.B[1]) and not torch.equal(c.B[1], c.B[2])
        for sg in range(1, c.nseg):
            assert not torch.equal(c.A[1, :c.seg_r], c.A[1, sg * c.seg_r:(sg + 1) * c.seg_r])
        assert len(set(c.scale.tolist())) == lc.SLOTS and all(v != 1.0 for v in c.scale.tolist())


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    kinds = ["gate_up"] if mutant in ("gate_up_swapped", "deinterleave_wrong") else ["qkv"]
    forms = ("slab",) if mutant == "slab1" else FORMS
    for kind in kinds:
        for form in forms:
            rejected = 0
            cases = [lc.grid_case(kind, 512, r, M, rowscale=True) for r in (8, 24) for M in (3, 17)]
            for c in cases:
                init = lc.initial_out(c, form)
                good = lc.reference_out(c, form, init)
                bad = lc.reference_out(c, form, init, mutant)
                rejected += not _same(good, bad)
            assert rejected >= len(cases) // 2, (mutant, kind, form, rejected)


def test_a_wrong_t_is_seen_through_the_expand():
    """The GPU test compares t as well; still, every rank column of t reaches some output."""
    c = lc.grid_case("qkv", 512, 8, 3)
    init = lc.initial_out(c, "slab")
    good = lc.reference_out(c, "slab", init)
    t = lc.reference_t(c)
    for sg in range(c.nseg):
        t2 = t.clone()
        t2[1, sg * c.seg_r + int(c.ranks[0]) - 1] += 1.0
        assert not _same(good, lc.reference_out(c, "slab", init, t=t2))


RANDOM = [("qkv", 512, 768, (16, 64, 32), 17), ("gate_up", 2048, 2048, (32, 16, 64), 5)]


@pytest.mark.parametrize("kind,K,N,ranks,M", RANDOM)
def test_random_cases_sit_inside_the_bound_on_the_reference_ops(kind, K, N, ranks, M):
    """The stated bound takes 2^-9 |t| for the rounding of t (bf16's half ulp is 2^-9 of the
    binade's upper end, 2^-8 of its lower end), so it is a bound on sums of at least 16 terms, not
    on a single one: the random cases use ranks >= 16 and are checked here to sit inside 0.9 of it
    with the reference ops, whose only difference to a GPU kernel is the order of the fp32 sums."""
    c = lc.random_case(kind, K, N, ranks, M)
    for form in FORMS:
        init = lc.initial_out(c, form)
        _, got = run_ops(c, form, init)
        got = (got[0] if form == "slab" else got).double()
        err = (got - lc.true_out(c, form, init)).abs()
        bound = lc.error_bound(c, form, init)
        assert (err <= 0.9 * bound).all(), (form, float((err / bound.clamp_min(1e-30)).max()))
        assert (err[c.idx < 0] == 0).all()
