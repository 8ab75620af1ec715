"""The exact attention tests can fail: on the CPU, for every case the GPU tests use
(tests/attention_cases.py), the needles carry weight, the kernels' own arithmetic (bf16 P) passes
the criterion, and every wrong reference -- a lost key, a key too many, swapped blocks, a causal
limit off by one, a lost partition, a lost new token -- is rejected for every query head it
touches.  Also: the layout formulas and the float64 reference against ops/reference.py, and the
case table against the list of positions and shapes the tests must cover."""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import reference as ref
from tests import attention_cases as ac

ALL_CASES = ([("decode", n) for n in ac.DECODE_CASES] + [("prefill", n) for n in ac.PREFILL_CASES]
             + [("mixed", "mixed")])


def get_case(kind, name):
    if kind == "decode":
        return ac.decode_case(name), ac.decode_ref(name)
    if kind == "prefill":
        return ac.prefill_case(name), ac.prefill_ref(name)
    return ac.mixed_case(), ac.mixed_ref()


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_needles_emulation_and_mutants(kind, name):
    case, r = get_case(kind, name)
    cu = case.cu_q
    classes = {}
    emu_worst = 0.0
    for s, seq in enumerate(case.seqs):
        L, ctx = seq.qlen, seq.ctx
        sl = slice(cu[s], cu[s] + L)
        # needle weights, for every query that sees the needle
        for n in seq.needles:
            w = r.p[s][:, max(0, n - (ctx - L)):, n]
            assert w.numel() and 0.05 <= float(w.min()) and float(w.max()) <= 1.0, (name, s, n, float(w.min()))
        # the kernels' arithmetic is accepted
        emu = ac.seq_attention64(case, s, bf16_p=True)[0]
        assert bool(ac.accepted(emu, r.out[sl], r.A[sl]).all()), (name, s)
        emu_worst = max(emu_worst, ac.ratio(emu, r.out[sl], r.A[sl]))
        # every mutant is rejected, for every query head it touches
        for label, mutant, touched in ac.mutants(case, s):
            bad = ac.seq_attention64(case, s, mutant=mutant, bf16_p=True)[0]
            ok = ac.accepted(bad, r.out[sl], r.A[sl])
            assert not bool(ok[touched].any()), (name, s, seq, label, ok[touched].nonzero().tolist()[:4])
            classes[label.split()[0]] = classes.get(label.split()[0], 0) + len(touched) * case.nq
    assert emu_worst < 1.0, emu_worst
    want = {"omit_key", "causal", "swap_bt"} | ({"omit_new_key", "include_ctx", "omit_partition"} if case.kpart else set())
    assert want <= set(classes), (name, classes)
    print(f"{kind} {name}: bf16-P emulation worst |err| / (u A) = {emu_worst:.3f}; query heads rejected per mutant "
          f"class: {classes}")


def test_omitting_a_needle_moves_the_output_by_many_bounds():
    """The margin behind the rejections: the smallest move, over every needle of the longest
    decode case and every query head, is above 20 u A (the bound is 2.25 u A)."""
    case, r = get_case("decode", "p512_g4_bs32_loud")
    worst = np.inf
    for s, seq in enumerate(case.seqs):
        for n in seq.needles:
            out = ac.seq_attention64(case, s, mutant=("omit_key", n))[0]
            if seq.ctx == 1:
                continue
            move = ((out - r.out[s:s + 1]).abs() / (ac.U * r.A[s:s + 1])).amax(dim=-1)
            worst = min(worst, float(move.min()))
    assert worst > 20, worst


@pytest.mark.parametrize("bs", [32, 64, 96])
def test_layout_formulas_match_reference(bs):
    tok = np.arange(bs)
    assert np.array_equal(ac._offsets(ac.kcache_off, tok), ref.kcache_index(bs).numpy())
    assert np.array_equal(ac._offsets(ac.vcache_off, tok), ref.vcache_index(bs).numpy())
    for fn in (ac.kcache_off, ac.vcache_off):   # a permutation of the slab
        assert sorted(ac._offsets(fn, tok).reshape(-1).tolist()) == list(range(bs * ac.HD))


@pytest.mark.parametrize("nq,nkv,bs", [(8, 2, 32), (4, 4, 64), (16, 1, 96)])
def test_float64_reference_matches_fp32_reference(nq, nkv, bs):
    """Random data (no needles, no poison): ops.reference.paged_attention is this reference to fp32 accuracy."""
    seqs = [ac.Seq(c, L, ()) for c, L in ((1, 1), (33, 1), (200, 1), (97, 40), (130, 130), (65, 3))]
    case = ac.build_case("random", nq, nkv, bs, "quiet", seqs, seed=7)
    g = torch.Generator().manual_seed(3)
    case.kc = torch.randn(case.kc.shape, generator=g).to(torch.bfloat16)
    case.vc = torch.randn(case.vc.shape, generator=g).to(torch.bfloat16)
    case.q = torch.randn(case.q.shape, generator=g).to(torch.bfloat16)
    got = ac.reference(case).out
    exp = ref.paged_attention(case.q.float(), case.kc, case.vc, case.bt, torch.tensor(case.ctxs),
                              torch.tensor(case.cu_q), ac.SCALE)
    torch.testing.assert_close(got.float(), exp, atol=2e-6, rtol=2e-6)


def test_criterion_rejects_what_assert_close_lets_through():
    """What the exact tests add: on randn data the older check (assert_close, atol = rtol = 2e-2)
    passes a decode output with the last key missing (the one the fold path adds); on the
    needle inputs the criterion rejects the same mistakes, and anything not finite."""
    rnd = ac.build_case("random", 8, 1, 32, "quiet", [ac.Seq(1200, 1, ())], seed=11)
    g = torch.Generator().manual_seed(5)
    rnd.kc = torch.randn(rnd.kc.shape, generator=g).to(torch.bfloat16)
    rnd.vc = torch.randn(rnd.vc.shape, generator=g).to(torch.bfloat16)
    rnd.q = torch.randn(rnd.q.shape, generator=g).to(torch.bfloat16)
    good = ac.seq_attention64(rnd, 0)[0]
    for mutant in (("omit_key", 1199),):
        bad = ac.seq_attention64(rnd, 0, mutant=mutant, bf16_p=True)[0]
        torch.testing.assert_close(bad.float(), good.float(), atol=2e-2, rtol=2e-2)   # blind
    case, r = get_case("decode", "p128_g8_bs32_quiet")
    s = max(range(len(case.seqs)), key=lambda i: case.seqs[i].ctx)
    assert case.seqs[s].ctx == 700
    for mutant in (("omit_key", 699), ("omit_partition", 43, 16)):
        bad = ac.seq_attention64(case, s, mutant=mutant, bf16_p=True)[0]
        assert not bool(ac.accepted(bad, r.out[s:s + 1], r.A[s:s + 1]).any())
    nan = torch.full_like(bad, float("nan"))
    assert not bool(ac.accepted(nan, r.out[s:s + 1], r.A[s:s + 1]).any())
    assert ac.ratio(nan, r.out[s:s + 1], r.A[s:s + 1]) == float("inf")
    big = r.out[s:s + 1] + ac.POISON_V
    assert not bool(ac.accepted(big, r.out[s:s + 1], r.A[s:s + 1]).any())


def test_fused_inputs_are_exact():
    """Slabs sum exactly (in any order) to the bf16 targets, the rotation table holds quarter
    turns only, and rotating the targets gives back the case's queries and new-token keys."""
    case = ac.decode_case("p128_g4_bs64_loud")
    for S, fold in ((1, True), (4, False), (3, True)):
        fi = ac.fused_inputs(case, S, fold)
        assert torch.equal(fi.slabs.flip(0).double().sum(0), fi.target.double())
        assert torch.equal(ac.sequential_sum(fi.slabs).to(torch.bfloat16), fi.target)
        cs = fi.cos_sin
        assert set(cs.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(cs[:, :64] ** 2 + cs[:, 64:] ** 2,
                                                                            torch.ones(cs.shape[0], 64))
        B, nq, nkv = len(case.seqs), case.nq, case.nkv
        qkv = fi.target.clone().view(B, nq + 2 * nkv, ac.HD)
        kc, vc = fi.kc0.clone(), fi.vc0.clone()
        assert not torch.equal(kc, case.kc)
        ref.rope_and_cache(qkv.view(B, -1), fi.positions, cs, kc, vc, fi.slots, nq, nkv, ac.HD)
        live = torch.tensor(case.ctxs) > 0
        assert torch.equal(qkv[live, :nq], case.q[live])
        assert torch.equal(kc, case.kc) and torch.equal(vc, case.vc)
        assert (fi.slots[~live] == -1).all() and (fi.slots[live] >= 0).all()
        if fold:
            assert torch.equal(fi.positions[live], torch.tensor(case.ctxs, dtype=torch.int32)[live] - 1)
        else:
            assert (fi.positions != torch.tensor(case.ctxs, dtype=torch.int32) - 1)[torch.tensor(case.ctxs) > 1].all()


def test_case_table_covers_the_listed_positions_and_shapes():
    D = {n: ac.decode_case(n) for n in ac.DECODE_CASES}
    for n, c in D.items():
        assert c.kpart == ac.DECODE_CASES[n][5]
        assert set(ac.BASE_CTXS[:7]) <= set(c.ctxs), n
        # poison: slots past ctx, unowned blocks, block-table entries past the sequence's blocks
        for s, seq in enumerate(c.seqs):
            nb = (seq.ctx + c.bs - 1) // c.bs
            assert (c.bt[s, nb:] == c.poison_block).all() and c.bt.shape[1] > nb
            assert 0 <= int(c.bt.min()) and int(c.bt.max()) < c.kc.shape[0]
        owned = set(c.bt.unique().tolist()) - {c.poison_block}
        assert c.kc.shape[0] - len(owned) == 4
        assert torch.isfinite(c.kc.float()).all() and torch.isfinite(c.vc.float()).all()
    full = [c for c in D.values() if set(ac.BASE_CTXS) <= set(c.ctxs)]
    for part in (128, 512):
        tags = set()
        for c in full:
            if c.kpart == part:
                tags |= {t for s in c.seqs for t in s.tags}
        assert {"0", "31", "32", "bs-1", "bs", "kpart-1", "kpart", "part_first", "last_part_first", "tail32", "tail8",
                "ctx-2", "ctx-1"} <= tags, (part, tags)
    # a workgroup walks more than one partition: more than 4 partitions of a sequence
    assert any(c.kpart == 128 and max(c.ctxs) > 512 for c in D.values())
    assert any(c.kpart == 512 and max(c.ctxs) > 2048 and sum(x > 1536 for x in c.ctxs) >= 2 for c in D.values())
    assert any(c.n_parts == 1 and c.kpart == 512 for c in D.values())
    assert any(c.n_parts == 1 and c.kpart == 128 for c in D.values())
    multi = [c for c in D.values() if c.n_parts > 1]
    assert {c.bs for c in multi if c.kpart == 128} == {32, 64, 96} == {c.bs for c in multi if c.kpart == 512}
    assert {c.G for c in D.values()} == {1, 4, 8, 16}
    assert {c.poison for c in D.values() if c.kpart == 128} == {"quiet", "loud"} == {c.poison for c in D.values() if c.kpart == 512}
    assert any(0 in c.ctxs for c in D.values() if c.kpart == 128) and any(0 in c.ctxs for c in D.values() if c.kpart == 512)
    # decode_max_ctx: 0, exactly max(ctx), and a value that changes n_parts -- three different n_parts per partition size
    for part in (128, 512):
        rules = {}
        for n, c in D.items():
            if c.kpart == part and c.n_parts > 1:
                rules.setdefault(ac.DECODE_CASES[n][6], set()).add(c.n_parts - (max(c.ctxs) + part - 1) // part)
        assert set(rules) == {"zero", "exact", "plus"}, rules
        assert rules["exact"] == {0} and rules["plus"] == {1} and min(rules["zero"]) >= 2, rules
    for c in D.values():
        if ac.DECODE_CASES[c.name][6] == "exact":
            assert c.decode_max_ctx == max(c.ctxs)
        if ac.DECODE_CASES[c.name][6] == "zero":
            assert c.decode_max_ctx == 0

    P = {n: ac.prefill_case(n) for n in ac.PREFILL_CASES}
    assert {c.G for c in P.values() if ac.prefill_kernel(c.G) == "mfma32"} == {1, 2, 4, 8}
    assert {c.G for c in P.values() if ac.prefill_kernel(c.G) == "wave16"} == {3, 16}
    for n, c in P.items():
        assert ac.prefill_kernel(c.G) == ac.PREFILL_CASES[n][4]
        assert {s.qlen for s in c.seqs} == {1, 31, 32, 33, 65}
        assert {s.ctx - s.qlen for s in c.seqs} == {0, 1, 63, 64, 100}
        assert {"diag", "63", "64", "ctx-1"} <= {t for s in c.seqs for t in s.tags}
        for seq in c.seqs:   # every 16-query group: a needle at its first query's position
            assert all(seq.ctx - seq.qlen + 16 * g in seq.needles for g in range((seq.qlen + 15) // 16))
            assert seq.ctx - 1 in seq.needles
    assert {c.bs for c in P.values()} == {32, 64, 96} and {c.poison for c in P.values()} == {"quiet", "loud"}

    m = ac.mixed_case()
    assert 0 < m.num_decode < len(m.seqs) and all(s.qlen == 1 for s in m.seqs[:m.num_decode])
    assert any(s.qlen > 1 for s in m.seqs[m.num_decode:]) and m.n_parts > 1
