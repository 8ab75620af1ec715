"""The verify-attention test inputs can fail (CPU): the float64 reference of
tests/attention_verify_cases.py is what the contract says, the ops' CPU path meets the criterion
against it, and every wrong reading of the contract -- the causal limit off by one either way, R
ignored so that padding rows attend, the tile's columns taken head-major, C taken as excluding the
new tokens -- misses the criterion on every (row, head) whose limit it moves."""
import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import reference
from tests import attention_cases as ac
from tests import attention_verify_cases as vc

NAMES = list(vc.CASES)
SMALL = ["g4_qr4_kv2", "g8_qr2_kv1", "g2_qr5_kv2", "g1_qr16_kv1"]


def test_cases_cover_the_issue():
    shapes = {(G, qr) for G, qr, _, _, _ in vc.CASES.values()}
    assert shapes == {(4, 4), (4, 2), (8, 2), (2, 5), (1, 16)}
    for G, qr in shapes:
        assert {nkv for g, q, nkv, _, _ in vc.CASES.values() if (g, q) == (G, qr)} == {1, 2}
    for name in NAMES:
        c = vc.case(name)
        assert c.qr * c.G <= 16
        seen = {(s.ctx, s.rows) for s in c.seqs}
        for R in range(1, c.qr + 1):
            assert (R, R) in seen and all((C, R) in seen for C in vc.CTXS)
        assert 0 in c.ctxs
        # scattered block tables: the blocks of the longest sequence are not in order
        s = max(range(len(c.seqs)), key=lambda i: c.seqs[i].ctx)
        n = (c.seqs[s].ctx + c.bs - 1) // c.bs
        assert c.bt[s, :n].tolist() != sorted(c.bt[s, :n].tolist())


def test_limits_are_the_contract():
    lim = reference.verify_limits([10, 0, 3, 7], [2, 1, 3, 1], 3, 2, 2)
    want = [[8, 8], [9, 9], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [0, 0], [1, 1], [2, 2], [6, 6], [-1, -1], [-1, -1]]
    assert lim.tolist() == want


@pytest.mark.parametrize("name", SMALL)
def test_reference_agrees_with_the_prefill_reference(name):
    """A verify step of R rows is a causal chunk of R query tokens ending at key C - 1: the float64
    reference of the prefill tests (its own gather, by the layout formulas) gives the same numbers."""
    c, ref = vc.case(name), vc.case_ref(name)
    live = [s for s in range(len(c.seqs)) if c.seqs[s].ctx > 0][::3]
    rows = torch.tensor([s * c.qr + j for s in live for j in range(c.seqs[s].rows)])
    pc = ac.Case(name, c.nq, c.nkv, c.bs, c.poison, [ac.Seq(c.seqs[s].ctx, c.seqs[s].rows, ()) for s in live],
                 c.q[rows], c.kc, c.vc, c.bt[torch.tensor(live)], -1)
    pref = ac.reference(pc)
    assert torch.allclose(ref.out[rows], pref.out, rtol=0, atol=1e-12)
    assert torch.allclose(ref.A[rows], pref.A, rtol=0, atol=1e-12)
    pad = torch.ones(len(c.seqs) * c.qr, dtype=torch.bool)
    pad[torch.tensor([s * c.qr + j for s in range(len(c.seqs)) if c.seqs[s].ctx > 0 for j in range(c.seqs[s].rows)])] = False
    assert pad.any() and not ref.out[pad].any() and not ref.A[pad].any()


def verify_md(c, device="cpu", ws=(None, None)):
    T = len(c.seqs) * c.qr
    return A.AttnMetadata(num_decode=T, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0,
                          slot_mapping=torch.full((T,), -1, dtype=torch.int32, device=device), verify_qr=c.qr,
                          verify_rows=torch.tensor(c.rows, dtype=torch.int32, device=device),
                          verify_block_tables=c.bt.to(device),
                          verify_context_lens=torch.tensor(c.ctxs, dtype=torch.int32, device=device),
                          decode_part_o=ws[0], decode_part_ml=ws[1])


@pytest.mark.parametrize("name", SMALL)
def test_cpu_op_meets_the_criterion(name):
    """ops.attention.paged_verify on CPU tensors (what the CPU engine runs): within the bound, and
    exact zeros for padding rows and padded sequences in an output that held NaN."""
    c, ref = vc.case(name), vc.case_ref(name)
    out = torch.full((c.q.shape[0], c.nq * vc.HD), float("nan"), dtype=torch.bfloat16)
    got = A.paged_verify(c.q, c.kc, c.vc, verify_md(c), ac.SCALE, out=out)
    assert got is out
    ac.check(out, ref, name)
    lim = reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G)
    dead = (lim < 0).all(dim=1)
    assert dead.any() and torch.equal(out[dead].view(torch.int16), torch.zeros_like(out[dead]).view(torch.int16))


def test_cpu_op_refusals():
    c = vc.case("g4_qr4_kv1")
    md = verify_md(c)
    md.verify_rows = md.verify_rows.clone()
    md.verify_rows[0] = c.qr + 1
    with pytest.raises(ValueError, match="verify_rows"):
        A.paged_verify(c.q, c.kc, c.vc, md, ac.SCALE)
    md = verify_md(c)
    md.verify_qr = 5   # 5 rows x group 4 > 16 columns
    with pytest.raises(ValueError, match="qr"):
        A.paged_verify(c.q[:20], c.kc, c.vc, md, ac.SCALE)
    md = verify_md(c)
    with pytest.raises(TypeError, match="bfloat16"):
        A.paged_verify(c.q, c.kc.to(reference.FP8), c.vc.to(reference.FP8), md, ac.SCALE)


# (one q head per kv head: row-major and head-major columns are the same order, no such mutant)
MUTANTS = [(n, m) for n in NAMES for m in reference.VERIFY_MUTANTS if not (m == "head_major" and vc.CASES[n][0] == 1)]


@pytest.mark.parametrize("name,mutant", MUTANTS)
def test_mutants_miss_the_criterion(name, mutant):
    c, ref = vc.case(name), vc.case_ref(name)
    lim = reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G)
    mlim = reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G, mutant)
    touched = lim != mlim
    frac = float(touched.float().mean())
    assert frac > 0.2, f"{mutant} moves the limit of only {frac:.0%} of the (row, head) pairs"
    out, _ = reference.paged_verify(c.q, c.kc, c.vc, c.bt, c.ctxs, c.rows, c.qr, ac.SCALE, dtype=torch.float64,
                                    mutant=mutant)
    ok = ac.accepted(out, ref.out, ref.A)
    assert not bool(ok[touched].any()), f"{mutant}: accepted at {(ok & touched).nonzero().tolist()[:8]}"
    assert bool(ok[~touched].all())
