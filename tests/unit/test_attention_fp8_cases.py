"""The FP8 KV-cache attention tests can fail: on the CPU, for every FP8 case the GPU tests use
(tests/attention_fp8_cases.py), every needle keeps its weight after quantisation, the kernels' own
arithmetic (e4m3 widened to bf16, P rounded to bf16) stays inside ``2.25 u A``, and every wrong
reference of attention_cases.mutants is rejected on every query head it touches -- zero missed.

Also shown: why quiet-poison cases run at ``v_scale >= 2`` (at 1 the slot after the context,
stored 448, is no longer loud enough for the longest contexts and ``include_ctx`` slips through),
that the twins' fused-decode targets are FP8-representable (the CPU writer reproduces the twin's
bytes from them), and the reference cast on the rounding ties, the subnormal edge and the clamp.
"""
import pytest
import torch

from polykey_service_amd.ops import reference as ref
from tests import attention_cases as ac
from tests import attention_fp8_cases as f8

ALL = ([("decode", n) for n in f8.DECODE] + [("prefill", n) for n in f8.PREFILL] + [("mixed", "")])


def get(kind, name):
    f = {"decode": f8.decode_case, "prefill": f8.prefill_case}[kind](name) if kind != "mixed" else f8.mixed_case()
    return f, f8.reference(kind, name)


def survey(case, r):
    """-> (largest emulation ratio, smallest needle weight, missed mutants [(seq, label)], mutants tried)"""
    cu = case.cu_q
    emu_worst, w_min, missed, tried = 0.0, 1.0, [], 0
    for s, seq in enumerate(case.seqs):
        L, ctx = seq.qlen, seq.ctx
        sl = slice(cu[s], cu[s] + L)
        for n in seq.needles:
            w = r.p[s][:, max(0, n - (ctx - L)):, n]
            assert w.numel() and float(w.max()) <= 1.0
            w_min = min(w_min, float(w.min()))
        emu = ac.seq_attention64(case, s, bf16_p=True)[0]
        assert bool(ac.accepted(emu, r.out[sl], r.A[sl]).all()), (case.name, s)
        emu_worst = max(emu_worst, ac.ratio(emu, r.out[sl], r.A[sl]))
        for label, mutant, touched in ac.mutants(case, s):
            tried += 1
            bad = ac.seq_attention64(case, s, mutant=mutant, bf16_p=True)[0]
            if bool(ac.accepted(bad, r.out[sl], r.A[sl])[touched].any()):
                missed.append((s, label))
    return emu_worst, w_min, missed, tried


@pytest.mark.parametrize("kind,name", ALL)
def test_needles_emulation_and_mutants(kind, name):
    f, r = get(kind, name)
    emu_worst, w_min, missed, tried = survey(f.case, r)
    print(f"{kind} {name} scales ({f.k_scale}, {f.v_scale}): emulation worst {emu_worst:.3f}, smallest needle weight "
          f"{w_min:.3f}, {len(missed)} of {tried} mutants missed")
    assert w_min >= 0.05, w_min
    assert emu_worst < 1.0, emu_worst
    assert tried > 0 and not missed, missed


def test_quiet_poison_needs_a_v_scale_of_two():
    """At v_scale = 1 the quiet case misses ``include_ctx`` on its longest contexts (the poison
    slot dequantises to 448 only); the GPU tests therefore run it at v_scale = 2."""
    name = "p128_g8_bs32_quiet"
    f = f8.decode_case(name, (1.0, 1.0))
    _, _, missed, _ = survey(f.case, ac.reference(f.case))
    assert missed and {label for _, label in missed} == {"include_ctx"}, missed
    assert f8.DECODE[name][1] >= 2.0


def test_twins_hold_what_the_cache_holds():
    f = f8.decode_case("p512_g4_bs32_loud")
    base = ac.decode_case("p512_g4_bs32_loud")
    assert f.kc8.dtype == f8.FP8 and f.kc8.shape == base.kc.shape and f.vc8.shape == base.vc.shape
    assert torch.equal(f.case.kc.float(), f.kc8.float() * f.k_scale)
    assert torch.equal(f.case.vc.float(), f.vc8.float() * f.v_scale)
    # poison: V stored +-448 and finite, loud K representable as it is
    pk, pv = ac.poison_rows("loud")
    blk = f.case.poison_block
    assert float(f.vc8[blk].float().abs().min()) == 448.0 and torch.isfinite(f.case.vc.float()).all()
    assert torch.equal(ref.k_cache_logical(f.case.kc[blk:blk + 1])[0, 0, 0].double(), torch.tensor(pk))
    assert not (f.kc8.view(torch.uint8) == 0x80).any() and not (f.vc8.view(torch.uint8) == 0x80).any()
    # quantising what the cache holds changes nothing
    assert f8.same_bytes(f8.quantize(f.case.kc, f.k_scale), f.kc8)
    assert f8.same_bytes(f8.quantize(f.case.vc, f.v_scale), f.vc8)


@pytest.mark.parametrize("name,S,fold", [("p128_g8_bs32_quiet", 4, True), ("p128_g16_bs96_loud", 1, False),
                                         ("p512_g4_bs32_loud", 3, True)])
def test_fused_targets_are_representable(name, S, fold):
    """The CPU writer turns the fused-decode targets into exactly the twin's bytes."""
    f = f8.decode_case(name)
    x = f8.fused_inputs(f, S, fold)
    case, fi = f.case, x.fi
    B, nq, nkv = len(case.seqs), case.nq, case.nkv
    assert not f8.same_bytes(x.kc0, f.kc8) and not f8.same_bytes(x.vc0, f.vc8)
    qkv = fi.target.clone()
    kc, vc = x.kc0.clone(), x.vc0.clone()
    ref.rope_and_cache(qkv, fi.positions, fi.cos_sin, kc, vc, fi.slots, nq, nkv, ac.HD, k_scale=f.k_scale,
                       v_scale=f.v_scale)
    assert f8.same_bytes(kc, f.kc8) and f8.same_bytes(vc, f.vc8)
    # what the fused kernels are given is the slab sums: there a -0 target is +0, and the quarter
    # turns put -0 into some zeros of the new K rows -- the only difference from the twin's bytes
    n, pairs = f8.byte_mismatches(x.kc_want, f.kc8)
    assert n == x.neg_zeros and pairs in ([], [[0x80, 0x00]]) and f8.same_bytes(x.vc_want, f.vc8)
    assert not f8.same_bytes(x.kc_want, x.kc0)
    print(f"{name} S={S} fold={fold}: {n} K bytes -0 where the twin holds +0")
    live = torch.tensor(case.ctxs) > 0
    assert torch.equal(qkv.view(B, nq + 2 * nkv, ac.HD)[live, :nq], case.q[live])


def test_reference_cast():
    x = torch.tensor([1.0625, 1.1875, 464.0, 1.5 * 2.0 ** -9, 2.0 ** -10, 2.0 ** -9, 1e4, -1e4, float("inf"),
                      -float("inf"), 448.0, -448.0, -0.0])
    want = torch.tensor([1.0, 1.25, 448.0, 2.0 ** -8, 0.0, 2.0 ** -9, 448.0, -448.0, 448.0, -448.0, 448.0, -448.0, -0.0])
    got = f8.quantize(x, 1.0)
    assert torch.equal(got.float(), want) and got.view(torch.uint8)[-1] == 0x80
    assert f8.same_bytes(got, ref.quantize_fp8(x, 1.0))
    assert torch.equal(f8.quantize(x, 0.5).float()[:2], torch.tensor([2.0, 2.5]))
    assert torch.equal(ref.dequantize_fp8(ref.quantize_fp8(x[:2], 0.5), 0.5), torch.tensor([1.0, 1.25]))


def test_writer_inputs_cover_the_listed_values():
    x = f8.writer_inputs(33, 4, 2, 0)
    assert x.shape == (33, 8 * ac.HD) and x.dtype == torch.bfloat16
