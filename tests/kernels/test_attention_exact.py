"""Paged attention kernels against a float64 reference, on inputs where every key position counts.

tests/attention_cases.py builds the inputs (needle keys at the positions where the index
arithmetic can slip, loud finite poison in everything a sequence does not own), the float64
reference and the criterion ``|out - ref64| <= 2.25 u A + 1e-30``, u = 2^-8, A = sum_j p_j |v_j|;
tests/unit/test_attention_cases.py shows on the CPU that every wrong reference (a lost key, a key
too many, swapped blocks, a causal limit off by one, a lost partition, a lost new token) fails it.

Largest observed ``|out - ref64| / (u A)`` on MI355X per test family (the bound is 2.25 as
derived; the CPU emulation of the kernels' arithmetic, P rounded to bf16, reaches 0.55-0.62):

    family                                   largest ratio
    decode (paged_attention)                 0.586
    fused decode (paged_decode_from_qkv)     0.586
    fused launch (gemm.qkv_attn_fused)       0.586
    prefill, MFMA 32x32 kernel               0.618
    prefill, one wave per head kernel        0.615
    mixed decode + prefill                   0.584
"""
import dataclasses

import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm
from tests import attention_cases as ac

pytestmark = pytest.mark.gpu
HD = ac.HD
D = "cuda"
I32 = torch.int32


def wide_q(case):
    """The queries inside a QKV-wide buffer (row stride above nq * 128) whose other columns are loud."""
    T = case.q.shape[0]
    buf = torch.full((T, case.nq + 2 * case.nkv, HD), ac.POISON_V, dtype=torch.bfloat16)
    buf[:, :case.nq] = case.q
    return buf.to(D)[:, :case.nq]


def decode_md(case, workspace, slots=None):
    B = len(case.seqs)
    return A.AttnMetadata(num_decode=B, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0,
                          slot_mapping=(torch.zeros(B, dtype=I32) if slots is None else slots).to(D),
                          decode_block_tables=case.bt.to(D), decode_context_lens=torch.tensor(case.ctxs, dtype=I32, device=D),
                          decode_part_o=workspace[0], decode_part_ml=workspace[1], decode_max_ctx=case.decode_max_ctx)


def workspace_for(case):
    return A.decode_workspace(len(case.seqs), case.nq, case.bt.shape[1], case.bs, D)


def both_orders(case, ref):
    """The case, then the same sequences reversed: the second launch on the same workspace
    finds another sequence's partials in every slot."""
    return ((case, ref, "first launch"), (ac.reversed_case(case), ac.reversed_ref(ref), "second launch, reversed"))


@pytest.mark.parametrize("name", list(ac.DECODE_CASES))
def test_decode(name):
    case, ref = ac.decode_case(name), ac.decode_ref(name)
    ws = workspace_for(case)
    kc, vc = case.kc.to(D), case.vc.to(D)
    worst = 0.0
    for c, r, what in both_orders(case, ref):
        out = A.paged_attention(wide_q(c), kc, vc, decode_md(c, ws), ac.SCALE)
        worst = max(worst, ac.check(out, r, f"{name}, {what}"))
    assert torch.equal(kc.cpu(), case.kc) and torch.equal(vc.cpu(), case.vc)   # decode only reads the cache
    print(f"\nratio decode {name}: {worst:.3f}")


@pytest.mark.parametrize("name", ["p128_g8_bs32_quiet", "p512_g4_bs32_loud"])
@pytest.mark.parametrize("delta", [-1, 1])
def test_decode_with_a_wrong_context_is_rejected(name, delta):
    """The check bites on the GPU too: the kernel run on contexts one key short (the needle at
    ctx - 1 lost) or one key long (the poison slot after ctx let in; a valid slot of the last
    block or of the poison block) misses the criterion on every query head of every sequence."""
    case, ref = ac.decode_case(name), ac.decode_ref(name)
    assert case.decode_max_ctx == 0
    live = torch.tensor(case.ctxs) > 0
    wrong = dataclasses.replace(case, seqs=[dataclasses.replace(s, ctx=s.ctx + delta if s.ctx else 0) for s in case.seqs])
    out = A.paged_attention(wide_q(case), case.kc.to(D), case.vc.to(D), decode_md(wrong, workspace_for(case)), ac.SCALE)
    ok = ac.accepted(out.view(ref.out.shape).cpu(), ref.out, ref.A)
    assert not bool(ok[live].any()), ok.nonzero().tolist()[:8]


def flipped(fi: ac.FusedInputs) -> ac.FusedInputs:
    return dataclasses.replace(fi, slabs=fi.slabs.flip(1), target=fi.target.flip(0), positions=fi.positions.flip(0),
                               slots=fi.slots.flip(0))


FROM_QKV = [(n, 4, True) for n in ac.DECODE_CASES] + [(n, 1, False) for n in ac.DECODE_CASES] + [
    ("p128_g4_bs64_loud", 3, True), ("p512_g4_bs32_loud", 8, False), ("p512_g4_bs96_quiet", 2, True),
    ("p128_g16_bs96_loud", 16, False)]


@pytest.mark.parametrize("name,S,fold", FROM_QKV)
def test_decode_from_qkv(name, S, fold):
    """Decode attention fed by the QKV split-K slabs: the new token of every sequence is the needle
    at key ctx - 1, whose cache row holds poison until the kernel writes it.  fold: its position
    is ctx - 1 and its key / value go through LDS; otherwise the kernel stores the row first.
    The slabs sum exactly and the rotation is by exact quarter turns, so the float64 reference
    of the plain decode case applies unchanged; the caches must end bit-identical to the case's
    (the written rows, and every other slot untouched, poison included)."""
    case, ref = ac.decode_case(name), ac.decode_ref(name)
    fi = ac.fused_inputs(case, S, fold)
    ws = workspace_for(case)
    B = len(case.seqs)
    worst = 0.0
    for (c, r, what), f in zip(both_orders(case, ref), (fi, flipped(fi))):
        kc, vc = fi.kc0.to(D), fi.vc0.to(D)
        p = gemm.Partial(f.slabs.to(D).reshape(-1), S, B, f.slabs.shape[2])
        out = A.paged_decode_from_qkv(p, f.positions.to(D), fi.cos_sin.to(D), kc, vc, decode_md(c, ws, f.slots),
                                      ac.SCALE, case.nq, case.nkv)
        worst = max(worst, ac.check(out, r, f"{name}, S {S}, fold {fold}, {what}"))
        assert torch.equal(kc.cpu(), case.kc), "K cache: written rows or untouched slots differ"
        assert torch.equal(vc.cpu(), case.vc), "V cache: written rows or untouched slots differ"
    print(f"\nratio from_qkv {name} S={S} fold={fold}: {worst:.3f}")


@pytest.mark.parametrize("name", list(ac.DECODE_CASES))
@pytest.mark.parametrize("fold", [True, False])
def test_qkv_attn_fused(name, fold):
    """The fused QKV projection -> decode attention launch on the same cases.  The projection is
    exact: input row m is 32 at column m (so its RMS is 1 and the row scale rounds away), weight
    column m is the bf16 target row m / 32, every other product is zero -- the slabs the launch
    leaves in the workspace must sum to the targets bit for bit, and then the float64 reference
    applies unchanged."""
    case, ref = ac.decode_case(name), ac.decode_ref(name)
    H = 1024
    B, N = len(case.seqs), (case.nq + 2 * case.nkv) * HD
    S = gemm.choose_split(N, H, B)
    fi = ac.fused_inputs(case, 1, fold)
    ws = workspace_for(case)
    flow = torch.zeros(gemm.FLOW_WORDS, dtype=I32, device=D)
    slab_ws = torch.empty(S * B * N, dtype=torch.float32, device=D)
    worst = 0.0
    for (c, r, what), f in zip(both_orders(case, ref), (fi, flipped(fi))):
        x = torch.zeros(B, H, dtype=torch.bfloat16)
        x[torch.arange(B), torch.arange(B)] = 32.0
        w = torch.zeros(N, H, dtype=torch.bfloat16)
        w[:, :B] = (f.target.float() / 32).t().to(torch.bfloat16)
        assert torch.equal(w[:, :B].float().t() * 32, f.target.float())
        x = x.to(D)
        rs = gemm.RowScale(gemm.residual_parts(None, x.clone(), torch.empty((H // gemm.PART_COLS) * B, device=D)), 1e-5)
        kc, vc = fi.kc0.to(D), fi.vc0.to(D)
        slab_ws.fill_(float("nan"))
        out = gemm.qkv_attn_fused(x, gemm.pack_weight(w.to(D)), rs, slab_ws, f.positions.to(D), fi.cos_sin.to(D), kc, vc,
                                  decode_md(c, ws, f.slots), ac.SCALE, case.nq, case.nkv, flow)
        got = ac.sequential_sum(slab_ws.view(S, B, N).cpu()).to(torch.bfloat16)
        assert torch.equal(got, f.target), "the projection's slabs do not sum to the targets"
        worst = max(worst, ac.check(out, r, f"{name}, fold {fold}, {what}"))
        assert torch.equal(kc.cpu(), case.kc), "K cache: written rows or untouched slots differ"
        assert torch.equal(vc.cpu(), case.vc), "V cache: written rows or untouched slots differ"
    assert int(flow.abs().sum()) == 0, flow.nonzero().tolist()
    print(f"\nratio fused {name} fold={fold}: {worst:.3f}")


def prefill_md(case, first=0):
    """Prefill metadata of sequences first.. of ``case`` (cu_q relative to the first prefill token)."""
    seqs = case.seqs[first:]
    cu = torch.tensor([0] + [s.qlen for s in seqs], dtype=I32).cumsum(0).to(I32)
    return dict(num_prefill=len(seqs), num_prefill_tokens=int(cu[-1]), max_prefill_q_len=max(s.qlen for s in seqs),
                prefill_block_tables=case.bt[first:].contiguous().to(D),
                prefill_context_lens=torch.tensor([s.ctx for s in seqs], dtype=I32, device=D), prefill_cu_q=cu.to(D))


@pytest.mark.parametrize("name", list(ac.PREFILL_CASES))
def test_prefill(name):
    """Both prefill kernels (GQA groups 1, 2, 4, 8: MFMA 32x32; 3, 16: one wave per head), query
    lengths 1-65 on prefixes 0-100 in one batch, needles on and just after the causal diagonal of
    every 16-query group, at keys 63 / 64 and at ctx - 1, poison past ctx."""
    case, ref = ac.prefill_case(name), ac.prefill_ref(name)
    T = case.q.shape[0]
    md = A.AttnMetadata(num_decode=0, slot_mapping=torch.zeros(T, dtype=I32, device=D), **prefill_md(case))
    kc, vc = case.kc.to(D), case.vc.to(D)
    out = A.paged_attention(wide_q(case), kc, vc, md, ac.SCALE)
    worst = ac.check(out, ref, name)
    assert torch.equal(kc.cpu(), case.kc) and torch.equal(vc.cpu(), case.vc)
    print(f"\nratio prefill {ac.PREFILL_CASES[name][4]} {name}: {worst:.3f}")


def test_mixed_decode_and_prefill():
    """One call with decode tokens (128-key partitions, one context past 512) and prefill chunks."""
    case, ref = ac.mixed_case(), ac.mixed_ref()
    nd, T = case.num_decode, case.q.shape[0]
    po, pml = A.decode_workspace(nd, case.nq, case.bt.shape[1], case.bs, D)
    md = A.AttnMetadata(num_decode=nd, slot_mapping=torch.zeros(T, dtype=I32, device=D),
                        decode_block_tables=case.bt[:nd].contiguous().to(D),
                        decode_context_lens=torch.tensor(case.ctxs[:nd], dtype=I32, device=D),
                        decode_part_o=po, decode_part_ml=pml, **prefill_md(case, nd))
    out = A.paged_attention(wide_q(case), case.kc.to(D), case.vc.to(D), md, ac.SCALE)
    worst = ac.check(out, ref, "mixed")
    print(f"\nratio mixed: {worst:.3f}")
