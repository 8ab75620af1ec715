"""FP8 (e4m3) KV cache: the quantising writers and the dequantising attention kernels, exactly.

tests/attention_fp8_cases.py turns the exact attention cases into their FP8 twins (the bytes the
kernels read, the dequantised cache the float64 reference reads); the criterion is the unchanged
``|out - ref64| <= 2.25 u A + 1e-30`` of tests/attention_cases.py, and
tests/unit/test_attention_fp8_cases.py shows on the CPU that every wrong reference fails it.  The
writers are compared byte for byte with the CPU reference cast
``x.clamp(-448, 448).to(float8_e4m3fn)`` on caches pre-filled with 0x7E.

Largest observed ``|out - ref64| / (u A)`` on MI355X per family (bound 2.25; the CPU emulation
of the kernels' arithmetic reaches 0.55-0.61):

    family                                   largest ratio
    decode (paged_attention)                 0.594
    fused decode (paged_decode_from_qkv)     0.594
    prefill, MFMA 32x32 kernel               0.609
    prefill, one wave per head kernel        0.599
    mixed decode + prefill                   0.599

The fused decode kernels' caches are compared byte for byte, sign of zero included, with what the
CPU reference writer makes of the same slab sums (attention_fp8_cases.fused_inputs).  That
expectation is the twin's bytes except for zeros of the new K rows that the quarter-turn rotation
of the summed slabs makes -0: 164 K bytes (fold) / 174 (non-fold) in the two 128-key cases, 1352 /
1504 in p512_g4_bs32_loud; the GPU caches match it exactly on every launch.
"""
import dataclasses

import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm
from tests import attention_cases as ac
from tests import attention_fp8_cases as f8

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
    return ((case, ref, "first launch"), (ac.reversed_case(case), ac.reversed_ref(ref), "second launch, reversed"))


def prefill_md(case, first=0):
    seqs = case.seqs[first:]
    cu = torch.tensor([0] + [s.qlen for s in seqs], dtype=I32).cumsum(0).to(I32)
    return dict(num_prefill=len(seqs), num_prefill_tokens=int(cu[-1]), max_prefill_q_len=max(s.qlen for s in seqs),
                prefill_block_tables=case.bt[first:].contiguous().to(D),
                prefill_context_lens=torch.tensor([s.ctx for s in seqs], dtype=I32, device=D), prefill_cu_q=cu.to(D))


def scales(f):
    return dict(k_scale=f.k_scale, v_scale=f.v_scale)


# ------------------------------------------------------------------------------------ writer
@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.5, 2.0)])
@pytest.mark.parametrize("mode", ["tile", "scattered"])
@pytest.mark.parametrize("bs", [32, 96])
def test_rope_and_cache_bytes(bs, mode, ks, vs):
    """rope_and_cache into an FP8 cache: T = 32 tokens filling one aligned 32-slot run (the packed
    path: 8-byte stores built in registers) and T = 33 with scattered slots, rows with slot -1
    and two rows in one block.  Rounding ties, the subnormal edge, the clamp and -0.0 are among
    the inputs; the rotation is by exact quarter turns.  Every written byte equals the CPU
    reference cast and every other byte is still 0x7E; q / k are rotated in place as for bf16."""
    nq, nkv, num_blocks = 4, 2, 7
    T = 32 if mode == "tile" else 33
    g = torch.Generator().manual_seed(bs + T)
    if mode == "tile":
        slots = (3 * bs + (bs - 32) + torch.arange(32)).to(I32)       # the last 32-slot tile of block 3
    else:
        slots = torch.randperm(5 * bs, generator=g)[:T].to(I32)       # blocks 0-4, no slot twice
        slots[1], slots[2] = 5 * bs + 1, 5 * bs + bs - 1              # two rows in block 5
        slots[[4, 9, 31]] = -1                                        # rotated, not stored
        live = slots[slots >= 0]
        assert live.unique().numel() == live.numel()
    positions = torch.randint(0, 64, (T,), generator=g).to(I32)
    cs = ac.quarter_turn_table(64, seed=bs)
    qkv = f8.writer_inputs(T, nq, nkv, seed=bs + T)
    kc_want, vc_want, q_want = f8.expected_cache(qkv, positions, cs, slots, nq, nkv, bs, num_blocks, ks, vs)
    kc = torch.full((num_blocks, nkv, bs, HD), 0x7E, dtype=torch.uint8, device=D).view(f8.FP8)
    vc = torch.full((num_blocks, nkv, HD, bs), 0x7E, dtype=torch.uint8, device=D).view(f8.FP8)
    x = qkv.to(D)
    A.rope_and_cache(x, positions.to(D), cs.to(D), kc, vc, slots.to(D), nq, nkv, HD, k_scale=ks, v_scale=vs)
    assert torch.equal(x.cpu().view(torch.int16), q_want.view(torch.int16)), "rotated q / k (or v) differ"
    kb, vb = kc.cpu().view(torch.uint8), vc.cpu().view(torch.uint8)
    n_written = int((slots >= 0).sum()) * nkv * HD
    for got, want, what in ((kb, kc_want.view(torch.uint8), "K"), (vb, vc_want.view(torch.uint8), "V")):
        bad = (got != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} bytes differ, first at {bad[0].tolist()}: " \
                                 f"{int(got[tuple(bad[0])])} != {int(want[tuple(bad[0])])}"
    # the expectation itself: written slots differ from the fill somewhere, the rest is untouched
    assert int((kc_want.view(torch.uint8) != 0x7E).sum()) <= n_written
    assert int((kc_want.view(torch.uint8) != 0x7E).sum()) > n_written // 2


# ------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(f8.DECODE))
def test_decode(name):
    f, ref = f8.decode_case(name), f8.reference("decode", name)
    case = f.case
    ws = workspace_for(case)
    kc, vc = f.kc8.to(D), f.vc8.to(D)
    worst = 0.0
    for c, r, what in both_orders(case, ref):
        out = A.paged_attention(wide_q(c), kc, vc, decode_md(c, ws), ac.SCALE, **scales(f))
        worst = max(worst, ac.check(out, r, f"{name}, {what}"))
    assert f8.same_bytes(kc, f.kc8) and f8.same_bytes(vc, f.vc8)   # decode only reads the cache
    print(f"\nratio fp8 decode {name}: {worst:.3f}")


@pytest.mark.parametrize("delta", [-1, 1])
def test_decode_with_a_wrong_context_is_rejected(delta):
    """The check bites on the GPU: contexts one key short (the needle at ctx - 1 lost) or one key
    long (the poison slot after ctx let in) miss the criterion on every live query head."""
    name = "p512_g4_bs32_loud"
    f, ref = f8.decode_case(name), f8.reference("decode", name)
    case = f.case
    assert case.decode_max_ctx == 0
    live = torch.tensor(case.ctxs) > 0
    wrong = dataclasses.replace(case, seqs=[dataclasses.replace(s, ctx=s.ctx + delta if s.ctx else 0) for s in case.seqs])
    out = A.paged_attention(wide_q(case), f.kc8.to(D), f.vc8.to(D), decode_md(wrong, workspace_for(case)), ac.SCALE,
                            **scales(f))
    ok = ac.accepted(out.view(ref.out.shape).cpu(), ref.out, ref.A)
    assert not bool(ok[live].any()), ok.nonzero().tolist()[:8]


def flipped(fi: ac.FusedInputs) -> ac.FusedInputs:
    return dataclasses.replace(fi, slabs=fi.slabs.flip(1), target=fi.target.flip(0), positions=fi.positions.flip(0),
                               slots=fi.slots.flip(0))


FROM_QKV = [(n, 4, True) for n in f8.DECODE] + [(n, 1, False) for n in f8.DECODE] + [("p128_g16_bs96_loud", 3, True)]


@pytest.mark.parametrize("name,S,fold", FROM_QKV)
def test_decode_from_qkv(name, S, fold):
    """Decode attention fed by the QKV split-K slabs over an FP8 cache: the new token of every
    sequence is the needle at key ctx - 1, whose cache row holds poison until the kernel writes
    it.  fold: its k / v go through LDS, quantised as the cache stores them; otherwise the kernel
    stores the row first.  The caches must end byte-identical, sign of zero included, to what the
    CPU reference writer makes of the same slabs (attention_fp8_cases.fused_inputs: the twin's
    bytes, with -0 in some zeros of the new K rows): the written rows and every untouched slot."""
    f, ref = f8.decode_case(name), f8.reference("decode", name)
    case = f.case
    x = f8.fused_inputs(f, S, fold)
    ws = workspace_for(case)
    B = len(case.seqs)
    worst = 0.0
    for (c, r, what), fi in zip(both_orders(case, ref), (x.fi, flipped(x.fi))):
        kc, vc = x.kc0.to(D), x.vc0.to(D)
        p = gemm.Partial(fi.slabs.to(D).reshape(-1), S, B, fi.slabs.shape[2])
        out = A.paged_decode_from_qkv(p, fi.positions.to(D), x.fi.cos_sin.to(D), kc, vc, decode_md(c, ws, fi.slots),
                                      ac.SCALE, case.nq, case.nkv, **scales(f))
        worst = max(worst, ac.check(out, r, f"{name}, S {S}, fold {fold}, {what}"))
        for got, want, which in ((kc, x.kc_want, "K"), (vc, x.vc_want, "V")):
            n, pairs = f8.byte_mismatches(got, want)
            assert n == 0, f"{which} cache: {n} bytes of the written rows or untouched slots differ: (got, want) {pairs}"
    print(f"\nfp8 from_qkv {name} S={S} fold={fold}: {x.neg_zeros} K bytes are -0 where the twin holds +0")
    print(f"\nratio fp8 from_qkv {name} S={S} fold={fold}: {worst:.3f}")


# ----------------------------------------------------------------------------------- prefill
@pytest.mark.parametrize("name", list(f8.PREFILL))
def test_prefill(name):
    """Both prefill kernels over an FP8 cache (GQA groups 1, 4, 8: MFMA 32x32, dequantised between
    the global load and the LDS store; 3: one wave per head with a converting load)."""
    f, ref = f8.prefill_case(name), f8.reference("prefill", name)
    case = f.case
    T = case.q.shape[0]
    md = A.AttnMetadata(num_decode=0, slot_mapping=torch.zeros(T, dtype=I32, device=D), **prefill_md(case))
    kc, vc = f.kc8.to(D), f.vc8.to(D)
    out = A.paged_attention(wide_q(case), kc, vc, md, ac.SCALE, **scales(f))
    worst = ac.check(out, ref, name)
    assert f8.same_bytes(kc, f.kc8) and f8.same_bytes(vc, f.vc8)
    print(f"\nratio fp8 prefill {ac.PREFILL_CASES[name][4]} {name}: {worst:.3f}")


def mixed_md(case):
    nd, T = case.num_decode, case.q.shape[0]
    po, pml = A.decode_workspace(nd, case.nq, case.bt.shape[1], case.bs, D)
    return A.AttnMetadata(num_decode=nd, slot_mapping=torch.zeros(T, dtype=I32, device=D),
                          decode_block_tables=case.bt[:nd].contiguous().to(D),
                          decode_context_lens=torch.tensor(case.ctxs[:nd], dtype=I32, device=D),
                          decode_part_o=po, decode_part_ml=pml, **prefill_md(case, nd))


def test_mixed():
    """One call with decode tokens (128-key partitions, one context past 512) and prefill chunks."""
    f, ref = f8.mixed_case(), f8.reference("mixed")
    out = A.paged_attention(wide_q(f.case), f.kc8.to(D), f.vc8.to(D), mixed_md(f.case), ac.SCALE, **scales(f))
    worst = ac.check(out, ref, "mixed")
    print(f"\nratio fp8 mixed: {worst:.3f}")


def test_bf16_unchanged():
    """No state leaks from an FP8 launch: a bf16 decode case and a bf16 prefill case give
    bit-identical output before and after FP8 calls on the same stream and workspace."""
    dname, pname = "p128_g8_bs32_quiet", "g4_bs96_quiet"
    dcase, pcase = ac.decode_case(dname), ac.prefill_case(pname)
    ws = workspace_for(dcase)
    dkc, dvc, pkc, pvc = dcase.kc.to(D), dcase.vc.to(D), pcase.kc.to(D), pcase.vc.to(D)
    pmd = A.AttnMetadata(num_decode=0, slot_mapping=torch.zeros(pcase.q.shape[0], dtype=I32, device=D), **prefill_md(pcase))

    def bf16_run():
        d = A.paged_attention(wide_q(dcase), dkc, dvc, decode_md(dcase, ws), ac.SCALE)
        p = A.paged_attention(wide_q(pcase), pkc, pvc, pmd, ac.SCALE)
        return d.cpu().view(torch.int16), p.cpu().view(torch.int16)

    before = bf16_run()
    ac.check(before[0].view(torch.bfloat16), ac.decode_ref(dname), "bf16 decode")
    fd, fp = f8.decode_case(dname), f8.prefill_case(pname)
    A.paged_attention(wide_q(fd.case), fd.kc8.to(D), fd.vc8.to(D), decode_md(fd.case, ws), ac.SCALE, **scales(fd))
    A.paged_attention(wide_q(fp.case), fp.kc8.to(D), fp.vc8.to(D), pmd, ac.SCALE, **scales(fp))
    after = bf16_run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_mismatched_cache_dtypes_are_an_error():
    f = f8.prefill_case("g1_bs32_quiet")
    case = f.case
    md = A.AttnMetadata(num_decode=0, slot_mapping=torch.zeros(case.q.shape[0], dtype=I32, device=D), **prefill_md(case))
    with pytest.raises(TypeError):
        A.paged_attention(wide_q(case), f.kc8.to(D), case.vc.to(D), md, ac.SCALE)


BAD_KV = [(2, 1.0, 1.0), (1, 0.0, 1.0), (1, float("inf"), 1.0), (1, float("nan"), 1.0), (1, 1.0, -1.0)]


@pytest.mark.parametrize("kv_dtype,ks,vs", BAD_KV)
def test_entry_points_refuse_a_bad_cache_type_before_launching(kv_dtype, ks, vs):
    """Each of the four entry points, called as ops/attention.py calls it at the smallest legal
    shape (1 sequence, nq = nkv = 1, one block of 32, context 1), returns -1 for an unknown
    kv_dtype or an FP8 scale that is not positive and finite, and launches nothing: the marker in
    the output (for rope_and_cache, the qkv rows it rotates in place) and the cache bytes stay."""
    from polykey_service_amd.ops import native
    marker = lambda *shape: torch.full(shape, 0x7E, dtype=torch.uint8, device=D)
    out, qkv = marker(1, 2 * HD), marker(1, 3 * 2 * HD)                       # bf16 rows
    kc, vc = marker(1, 1, 32, 2 * HD), marker(1, 1, HD, 2 * 32)               # room for either element type
    q = torch.zeros(1, HD, dtype=torch.bfloat16, device=D)
    slab = torch.zeros(1, 1, 3 * HD, device=D)                                # S = 1, M = 1
    zero, one = torch.zeros(1, dtype=I32, device=D), torch.ones(1, dtype=I32, device=D)   # positions / slots / table; context
    cu = torch.tensor([0, 1], dtype=I32, device=D)
    cs = torch.zeros(1, HD, device=D)
    kv, st = (kv_dtype, ks, vs), native.stream_ptr()
    calls = {
        "pk_rope_and_cache": (qkv.data_ptr(), zero.data_ptr(), cs.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                              zero.data_ptr(), 1, 1, 1, HD, 32, 3 * HD, *kv, st),
        "pk_paged_decode": (out.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), zero.data_ptr(), one.data_ptr(),
                            0, 0, 1, 1, 1, 32, 1, HD, HD, ac.SCALE, 0, *kv, st),
        "pk_paged_decode_qkv": (out.data_ptr(), slab.data_ptr(), 1, 1, zero.data_ptr(), cs.data_ptr(), zero.data_ptr(),
                                kc.data_ptr(), vc.data_ptr(), zero.data_ptr(), one.data_ptr(), 0, 0, 1, 1, 1, 32, 1,
                                HD, ac.SCALE, 0, *kv, st),
        "pk_paged_prefill": (out.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), zero.data_ptr(), one.data_ptr(),
                             cu.data_ptr(), 1, 1, 1, 32, 1, HD, HD, 1, ac.SCALE, *kv, st),
    }
    for name, args in calls.items():
        assert len(args) == len(native.SIGNATURES[name]), name
        with pytest.raises(native.KernelError, match="code -1"):
            native.call(name, *args)
    torch.cuda.synchronize()
    for t in (out, qkv, kc, vc):
        assert bool((t == 0x7E).all())
