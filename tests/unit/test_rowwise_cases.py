"""The row-wise cases (tests/rowwise_cases.py) on the CPU: every builder keeps its budget, every
reference satisfies its own criterion, every mutant -- a reference with one of the bugs a kernel
could have -- is rejected by at least one case of the set tests/kernels/test_rowwise_exact.py runs
on the GPU (``pytest -s`` prints the rejecting case per mutant), and the CPU paths of ``ops`` agree
with the references."""
import re
from pathlib import Path

import pytest
import torch

from tests import gemm_cases as gc
from tests import rowwise_cases as rc

BF16 = torch.bfloat16
ROOT = Path(__file__).resolve().parents[2]


# ------------------------------------------------------------------------------ widths, budgets
def test_width_table_matches_the_launcher():
    """The table of the cases against pick_vpt, and pick_vpt here against the launcher's source."""
    for H, want in rc.WIDTHS.items():
        assert rc.pick_vpt(H) == want, H
    assert {v for v, _ in rc.WIDTHS.values()} == {1, 2, 4, 8}
    assert rc.pick_vpt(9216 - 8)[0] == -1 and all(rc.pick_vpt(H)[0] == 1 for H in range(512, 8193, 512))
    src = (ROOT / "csrc/kernels/norm_act.hip").read_text()
    cond = re.search(r"for \(int vpt : \{1, 2, 4, 8\}\) \{\s*if \((.*?)\) \{", src, re.S).group(1)
    assert cond == "vecs % vpt == 0 && vecs / vpt <= 1024 && (vecs / vpt) % 64 == 0"


@pytest.mark.parametrize("H", list(rc.WIDTHS))
def test_norm_budgets(H):
    """Every builder asserts its own budget; the exact family and the integer family are points."""
    for T in rc.NORM_T:
        for fused in (False, True):
            for fam in (rc.FUSED_FAMILIES if fused else rc.FAMILIES):
                for eps in (rc.NORM_EPS if fam == "pow4" else [1e-5]):
                    c = rc.norm_case(fam, T, H, eps, fused)
                    (lo, hi), new = rc.ref_norm(c)
                    assert gc.is_bf16(lo) and gc.is_bf16(hi) and bool((lo <= hi).all()), c.name
                    mid = rc.norm_mid(c)
                    assert gc.inside(mid, (lo, hi)), c.name
                    if c.exact:
                        assert gc.same_bits(lo, hi)
                    # the intervals are tight: each of the two roundings splits by at most one bf16 step
                    tight = bool(((hi - lo).abs() <= 2.0 ** -6 * torch.maximum(lo.abs(), hi.abs())).all())
                    assert tight, c.name
                    assert fused == (new is not None)


def test_integer_rows_tell_one_rounding_from_two():
    c = rc.norm_case("int", 3, 5120)
    good, bad = rc.ref_norm(c)[0], rc.ref_norm(c, "round_once")[0]
    assert float((good[0] == good[1]).double().mean()) > 0.99     # a single point almost everywhere
    assert float(((bad[1] < good[0]) | (bad[0] > good[1])).double().mean()) > 0.1


def test_silu_tightening():
    g = rc.all_gates().double()
    lo, hi = rc.iv_silu_gate(g)            # asserts that float64 agrees with both derivations
    big, neg = g >= 18, (g <= -89) & g.isfinite()
    assert bool((lo[big] == g[big]).all()) and bool((hi[big] == g[big]).all())
    assert bool((lo[neg] == 0).all()) and bool((hi[neg] == 0).all())
    nan = lo.isnan()
    assert bool((nan == (g.isnan() | (g == -float("inf")))).all()) and bool((hi.isnan() == nan).all())
    assert float(lo[g == 0].abs().max()) == 0 and float(hi[g == 0].abs().max()) == 0
    # the derivations: e^-18 (1 + 30 u) < 2^-25;  89 log2(e) >= 128
    assert torch.exp(torch.tensor(-18.0, dtype=torch.float64)) * (1 + 30 * gc.U) < 2.0 ** -25
    assert 89.0 * 1.4426950408889634 >= 128.0
    # NaN exactly where the float64 formula gives NaN, for every up value
    for il in (False, True):
        x = rc.silu_sweep(il).double()
        lo, hi = rc.ref_silu_mul(x, il)
        gg, uu = rc.silu_operands(x, il)
        f64 = gc.silu64(gg) * uu
        assert bool((lo[:-64].isnan() == f64.reshape(-1).isnan()).all()) and bool(lo[-64:].isnan().all())
        assert gc.inside(rc.ref_silu_mul(x, il, slack=False)[0], (lo, hi))


def test_silu_il_is_gemm_cases_ref_silu():
    """For Gaussian gates the interleaved reference is gemm_cases.ref_silu as it stands."""
    x = rc.silu_gauss(5, 2064)
    lo, hi = rc.ref_silu_mul(x, True)
    a, b = gc.ref_silu(x)
    assert gc.same_bits(lo[:-64].view(5, 2064), a) and gc.same_bits(hi[:-64].view(5, 2064), b)
    assert gc.same_bits(rc.join_gate_up(*gc.split_gate_up(x)), x)


def test_copy_sizes_cover_the_launcher():
    """One workgroup, the n16 / 256 + 1 rounding (an idle second workgroup at exactly 256 vectors), the
    cap of 64 at exactly one pass, a second pass of one vector, and several passes with a remainder."""
    assert [rc.copy_grid(b) for b in rc.COPY_BYTES] == [(1, 1), (1, 1), (2, 1), (2, 1), (64, 1), (64, 2), (64, 5)]
    src = rc.copy_source(4112)
    assert src.numel() == 1028 + 16 and len(set(src.tolist())) == src.numel()


def test_embed_ids():
    for (start, local, holds) in rc.EMBED_SHARDS:
        sp = rc.embed_special_ids(start, local, holds)
        ids = rc.embed_ids(77, start, local, holds)            # asserts its own properties
        hit = ((ids >= start) & (ids < start + local)).any()
        assert bool(hit) == holds and {0, rc.EMBED_V - 1} <= set(sp) <= set(ids.tolist())
    assert rc.embed_special_ids(250, 300, True) == [249, 250, 549, 550, 0, 999]
    assert rc.EMBED_SHARDS[3][0] + rc.EMBED_SHARDS[3][1] == rc.EMBED_V and rc.EMBED_SHARDS[2][1] == 1


# -------------------------------------------------------------------------------------- mutants
def _norm_cases(fused: bool):
    """The GPU set, cheapest first."""
    for H in rc.WIDTHS:
        for T in (3, 1, 17):
            for fam in (rc.FUSED_FAMILIES if fused else rc.FAMILIES):
                yield rc.norm_case(fam, T, H, 1e-5, fused)


@pytest.mark.parametrize("mutant,fused", [(m, f) for f in (False, True) for m in rc.NORM_MUTANTS
                                          if not (f and "stride" in m)])  # the fused kernel takes no strides
def test_norm_mutants_rejected(mutant, fused):
    hit = None
    for c in _norm_cases(fused):
        if "stride" in mutant:
            bad = rc.misses(rc.ref_norm_sliced(c, mutant), rc.ref_norm_sliced(c))
        else:
            bad = rc.misses(rc.ref_norm(c, mutant)[0], rc.ref_norm(c)[0])
        if bad:
            hit = c.name
            break
    print(f"MUTANT {mutant} rejected by {hit}")
    assert hit is not None


@pytest.mark.parametrize("mutant", rc.FUSED_MUTANTS)
def test_fused_mutants_rejected(mutant):
    hit = None
    for c in _norm_cases(True):
        if rc.misses(rc.ref_norm(c, mutant)[0], rc.ref_norm(c)[0]):
            hit = c.name
            break
    print(f"MUTANT {mutant} rejected by {hit}")
    assert hit is not None


def test_norm_mutants_where_they_must_show():
    """Beyond "somewhere": the family built for a mutant rejects it at every width."""
    for H, (vpt, _) in rc.WIDTHS.items():
        e = rc.norm_case("eps", 3, H)
        for m in ("eps_dropped", "eps_outside_rsqrt"):
            assert rc.misses(rc.ref_norm(e, m)[0], rc.ref_norm(e)[0]), (m, H)
        i = rc.norm_case("int", 3, H)
        p = rc.norm_case("pow4", 3, H)
        for m in ("round_once", "weight_shift8", "rinv_next_row", "mean_over_h_minus_512"):
            assert rc.misses(rc.ref_norm(i, m)[0], rc.ref_norm(i)[0]), (m, H)
        for m in ("weight_shift8", "rinv_next_row", "mean_over_h_minus_512"):
            assert rc.misses(rc.ref_norm(p, m)[0], rc.ref_norm(p)[0]), (m, H)
        for m in ("first_vector_only", "weight_by_thread"):          # only VPT > 1 can tell
            for c in (i, p):
                assert rc.misses(rc.ref_norm(c, m)[0], rc.ref_norm(c)[0]) == (vpt > 1), (m, H)
        for m in ("in_stride_is_h", "out_stride_is_in_stride"):
            assert rc.misses(rc.ref_norm_sliced(p, m), rc.ref_norm_sliced(p)), (m, H)
        r = rc.norm_case("rounding", 3, H, fused=True)                # asserts ss_unrounded, norm_of_unrounded
        g = rc.norm_case("gauss", 3, H, fused=True)
        for m in ("ss_from_x_only", "ss_from_old_residual"):
            for c in (r, g):
                assert rc.misses(rc.ref_norm(c, m)[0], rc.ref_norm(c)[0]), (m, H)
    # the sliced reference keeps NaN everywhere outside [T, H]
    lo, _ = rc.ref_norm_sliced(p)
    row0, col0 = rc.OUT_GEOM[:2]
    inner = torch.zeros_like(lo, dtype=torch.bool)
    inner[row0:row0 + p.T, col0:col0 + p.H] = True
    assert bool(lo[~inner].isnan().all()) and not bool(lo[inner].isnan().any())


def _silu_inputs():
    for I in rc.SILU_I:
        for T in (5, 1):
            yield f"gauss-T{T}-I{I}", rc.silu_gauss(T, I)
    yield "sweep", None


@pytest.mark.parametrize("mutant", rc.SILU_MUTANTS)
def test_silu_mutants_rejected(mutant):
    for il in (False, True):
        if (il and mutant == "up_offset_2i") or (not il and mutant.startswith("il_")):
            continue                         # a slip of the other layout
        hit = None
        for name, x in _silu_inputs():
            if il and x is not None and x.shape[1] % 32:
                continue
            x = rc.silu_sweep(il).double() if x is None else x
            if rc.misses(rc.ref_silu_mul(x, il, mutant), rc.ref_silu_mul(x, il)):
                hit = name
                break
        print(f"MUTANT {mutant} ({'interleaved' if il else 'split'}) rejected by {hit}")
        assert hit is not None
    # the sweep alone sees a gate / up exchange in both layouts
    for il in (False, True):
        x = rc.silu_sweep(il).double()
        assert rc.misses(rc.ref_silu_mul(x, il, "gate_up_swap"), rc.ref_silu_mul(x, il))


@pytest.mark.parametrize("mutant", rc.EMBED_MUTANTS)
def test_embedding_mutants_rejected(mutant):
    hit = None
    for H in rc.EMBED_H:
        for (start, local, holds) in rc.EMBED_SHARDS:
            table = rc.embed_table(local, H)
            ids = rc.embed_ids(77, start, local, holds)
            if not torch.equal(rc.ref_embedding(table, ids, start, local, mutant), rc.ref_embedding(table, ids, start, local)):
                hit = hit or f"H{H}-shard({start},{local})"
                if mutant in ("first_row_dropped", "mask_off_by_one_low"):
                    # the single-id cases see it too
                    one = torch.tensor([start if mutant == "first_row_dropped" else start - 1])
                    assert not torch.equal(rc.ref_embedding(table, one, start, local, mutant),
                                           rc.ref_embedding(table, one, start, local))
    print(f"MUTANT {mutant} rejected by {hit}")
    assert hit is not None


def test_every_mutant_is_listed():
    assert set(rc.NORM_MUTANTS) == {"eps_dropped", "eps_outside_rsqrt", "mean_over_h_minus_512", "first_vector_only",
                                    "weight_by_thread", "weight_shift8", "round_once", "rinv_next_row",
                                    "in_stride_is_h", "out_stride_is_in_stride"}
    assert set(rc.FUSED_MUTANTS) == {"ss_from_x_only", "ss_from_old_residual", "ss_unrounded", "norm_of_unrounded"}
    assert set(rc.SILU_MUTANTS) == {"gate_up_swap", "up_offset_2i", "il_block8", "il_half_swap", "silu_unrounded",
                                    "last_group_dropped"}
    assert set(rc.EMBED_MUTANTS) == {"first_row_dropped", "mask_off_by_one_low", "start_ignored",
                                     "tail_vector_dropped", "row_stride_2048"}


# ------------------------------------------------------------------------ the CPU paths of ``ops``
@pytest.mark.parametrize("H", [512, 1536, 9216])
def test_ops_norm_cpu(H):
    from polykey_service_amd import ops
    for fam in rc.FUSED_FAMILIES:
        for fused in (False, True):
            if fam == "rounding" and not fused:
                continue
            c = rc.norm_case(fam, 3, H, 1e-5, fused)
            iv, new = rc.ref_norm(c)
            if not fused:
                assert gc.inside(ops.rms_norm(c.a.to(BF16), c.w.to(BF16), c.eps), iv), c.name
                buf, out = rc.sliced(torch.zeros((3, H), dtype=BF16), rc.OUT_GEOM)
                ops.rms_norm(c.a.to(BF16), c.w.to(BF16), c.eps, out=out)
                assert gc.inside(buf, rc.ref_norm_sliced(c)), c.name
            else:
                x, r = c.a.to(BF16), c.b.to(BF16)
                ops.fused_add_rms_norm(x, r, c.w.to(BF16), c.eps)
                assert gc.same_bits(r, new) and gc.inside(x, iv), c.name


def test_ops_silu_cpu():
    from polykey_service_amd import ops
    from polykey_service_amd.ops import gemm
    for il, fn in ((False, ops.silu_and_mul), (True, gemm.silu_and_mul_interleaved)):
        for x in (rc.silu_gauss(5, 2064), rc.silu_sweep(il).double()):
            T, I = x.shape[0], x.shape[1] // 2
            iv = rc.ref_silu_mul(x, il)
            assert gc.inside(fn(x.to(BF16)).reshape(-1), (iv[0][:-64], iv[1][:-64]))
            buf = torch.full((T * I + 64,), float("nan"), dtype=BF16)
            fn(x.to(BF16), out=buf[:T * I].view(T, I))
            assert gc.inside(buf, iv)


def test_ops_embedding_cpu():
    """The CPU path is the same bit copy: zeros for masked rows even where row 0 holds NaN or inf."""
    from polykey_service_amd import ops
    for (start, local, holds) in rc.EMBED_SHARDS:
        table = rc.embed_table(local, 40)
        table[0, :4] = torch.tensor([0x7FC0, 0x7F80, -128, -1], dtype=torch.int16)   # NaN, inf, -inf, NaN
        for ids in (rc.embed_ids(77, start, local, holds), rc.embed_ids(77, start, local, holds).to(torch.int32),
                    rc.embed_ids(78, start, local, holds).view(2, 39)):
            got = ops.embedding(ids, table.view(BF16), start, local)
            assert got.shape == ids.shape + (40,)
            assert torch.equal(got.reshape(-1).view(torch.int16), rc.ref_embedding(table, ids, start, local)[:-64])


def test_ops_refusals_cpu():
    """The checks ops.rms_norm makes ahead of a launch, on tensors no kernel ever sees."""
    from polykey_service_amd.ops import norm
    buf = torch.zeros((4, 1040), dtype=BF16)
    norm.check_rows(buf[:, 8:520], "ok")
    norm.check_rows(buf[:1, 8:520], "ok")
    for bad in (buf[:, 4:516],                                  # base 8 bytes off
                torch.zeros((4, 516), dtype=BF16)[:, :512],     # row stride 516
                buf[:, 0:1024:2],                               # column stride 2
                buf.view(2, 2, 1040)):                          # not 2-D
        with pytest.raises((AssertionError, ValueError)):
            norm.check_rows(bad, "bad")
