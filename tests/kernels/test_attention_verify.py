"""pk_paged_verify (verify attention of speculative decoding) against the float64 reference, on the
inputs of tests/attention_verify_cases.py: (G, qr) in {(4,4), (4,2), (8,2), (2,5), (1,16)} at one and
two kv heads, every R in 1..qr, contexts on both sides of the 32-key step and of both partition
sizes, scattered block tables, padded sequences.  tests/unit/test_attention_verify_cases.py shows
on the CPU that every wrong reading of the contract fails these inputs.

The bound is the decode kernels' (tests/attention_cases.py), unchanged: the same roundings -- P in
bf16, fp32 sums, one output rounding -- so ``|out - ref64| <= 2.25 u A + 1e-30``.
"""
import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import native, reference
from tests import attention_cases as ac
from tests import attention_verify_cases as vc

pytestmark = pytest.mark.gpu
HD = ac.HD
D = "cuda"
I32 = torch.int32


def md_for(c, ws, max_blocks=None):
    T = len(c.seqs) * c.qr
    return A.AttnMetadata(num_decode=T, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0,
                          slot_mapping=torch.full((T,), -1, dtype=I32, device=D), verify_qr=c.qr,
                          verify_rows=torch.tensor(c.rows, dtype=I32, device=D), verify_block_tables=c.bt.to(D),
                          verify_context_lens=torch.tensor(c.ctxs, dtype=I32, device=D),
                          decode_part_o=ws[0], decode_part_ml=ws[1])


def wide_q(c):
    """The queries inside a QKV-wide buffer (row stride above nq * 128) whose other columns are loud."""
    T = c.q.shape[0]
    buf = torch.full((T, c.nq + 2 * c.nkv, HD), ac.POISON_V, dtype=torch.bfloat16)
    buf[:, :c.nq] = c.q
    return buf.to(D)[:, :c.nq]


def nan_out(c):
    return torch.full((c.q.shape[0], c.nq * HD), float("nan"), dtype=torch.bfloat16, device=D)


def check_zeros(out, c, what):
    lim = reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G)
    dead = (lim < 0).all(dim=1)
    got = out.cpu()[dead].view(torch.int16)
    assert torch.equal(got, torch.zeros_like(got)), f"{what}: padding rows / padded sequences are not exact zeros"
    return int(dead.sum())


@pytest.mark.parametrize("name", list(vc.CASES))
def test_verify(name):
    """The whole case in one launch (512-key partitions) and in launches of few sequences (128-key
    partitions), on one workspace: every launch finds another launch's partials in its slots."""
    c, ref = vc.case(name), vc.case_ref(name)
    kc, vcache = c.kc.to(D), c.vc.to(D)
    cap = c.bt.shape[1] * c.bs
    n = len(c.seqs)
    ws = A.verify_workspace(n, c.qr, c.nq, c.bt.shape[1], c.bs, D)
    assert ac.decode_dispatch(n, c.nkv, cap)[0] == ac.PART
    out = A.paged_verify(wide_q(c), kc, vcache, md_for(c, ws), ac.SCALE, out=nan_out(c))
    worst = ac.check(out, ref, f"{name}, one launch")
    n_dead = check_zeros(out, c, name)
    assert n_dead >= 2 * c.qr
    chunk = vc.small_partition_chunk(c.nkv, cap)
    assert ac.decode_dispatch(chunk, c.nkv, cap)[0] == ac.PART_SMALL
    # the sequences dealt round-robin: every launch holds short and long contexts
    n_launch = (n + chunk - 1) // chunk
    for i in range(n_launch):
        idx = list(range(i, n, n_launch))
        sub, sref = vc.subset(c, ref, idx)
        out = A.paged_verify(wide_q(sub), kc, vcache, md_for(sub, ws), ac.SCALE, out=nan_out(sub))
        worst = max(worst, ac.check(out, sref, f"{name}, launch {i} of {n_launch} at 128-key partitions"))
        check_zeros(out, sub, f"{name}, launch {i}")
    assert torch.equal(kc.cpu(), c.kc) and torch.equal(vcache.cpu(), c.vc)   # verify only reads the cache
    print(f"\nratio verify {name}: {worst:.3f}")


def test_mutant_rows_are_rejected_on_the_gpu():
    """The check bites on the GPU too: the kernel told R = qr for every sequence (padding rows
    attend, real rows shift) misses the criterion on every (row, head) whose limit that moves."""
    name = "g4_qr4_kv1"
    c, ref = vc.case(name), vc.case_ref(name)
    ws = A.verify_workspace(len(c.seqs), c.qr, c.nq, c.bt.shape[1], c.bs, D)
    md = md_for(c, ws)
    md.verify_rows = torch.full_like(md.verify_rows, c.qr)
    out = A.paged_verify(wide_q(c), c.kc.to(D), c.vc.to(D), md, ac.SCALE, out=nan_out(c))
    ok = ac.accepted(out.view(ref.out.shape).cpu(), ref.out, ref.A)
    touched = reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G) != \
        reference.verify_limits(c.ctxs, c.rows, c.qr, c.nq, c.G, "ignore_rows")
    assert touched.any() and not bool(ok[touched].any())
    assert bool(ok[~touched].all())


# (C, R) whose rows all lie in the partition of key C - 1 at both partition sizes, so a decode
# launch at context C - R + j + 1 walks the same partitions: 200 and 700 among them
def bitwise_seqs(qr):
    ctxs = (qr, 31, 33, 127, 253, 515 + qr, 1100, 0, 200, 700)   # (the last ten sequences make the small launch)
    seqs = [vc.VSeq(C, R) for C in ctxs for R in sorted({1, (qr + 1) // 2, qr}) if C == 0 or C >= R]
    for s in seqs:
        for part in (ac.PART, ac.PART_SMALL):
            assert s.ctx == 0 or (s.ctx - s.rows) // part == (s.ctx - 1) // part, (s, part)
    return seqs


@pytest.mark.parametrize("kpart", [ac.PART_SMALL, ac.PART])
@pytest.mark.parametrize("shape", ["g4_qr4_kv1", "g8_qr2_kv2", "g2_qr5_kv1", "g1_qr16_kv2"])
def test_rows_equal_decode_bit_for_bit(shape, kpart):
    """Row j of a sequence is bit for bit what pk_paged_decode returns for a sequence of context
    C - R + j + 1 with that row's q (zeros past R): the same launch plan (the same sequences, block
    tables and workspace), the same keys per wave, and masked keys add exact zeros."""
    G, qr, nkv, bs, poison = vc.CASES[shape]
    seqs = bitwise_seqs(qr)
    chunk = vc.small_partition_chunk(nkv, 1100 + 3 * bs)
    if kpart == ac.PART_SMALL:
        seqs = seqs[-chunk:] if len(seqs) > chunk else seqs
    else:
        seqs = seqs * (2 * chunk // len(seqs) + 1)
    c = vc.build(shape + "_bitwise", G, qr, nkv, bs, poison, seqs, seed=77)
    n, cap = len(seqs), c.bt.shape[1] * bs
    assert ac.decode_dispatch(n, nkv, cap)[0] == kpart
    kc, vcache = c.kc.to(D), c.vc.to(D)
    ws = A.verify_workspace(n, qr, c.nq, c.bt.shape[1], bs, D)
    q = wide_q(c)
    out = A.paged_verify(q, kc, vcache, md_for(c, ws), ac.SCALE, out=nan_out(c)).view(n, qr, c.nq * HD)
    ac.check(out, vc.ref64(c), shape)
    bt = c.bt.to(D)
    for j in range(qr):
        ctx = torch.tensor([s.ctx - s.rows + j + 1 if s.ctx > 0 and j < s.rows else 0 for s in seqs], dtype=I32, device=D)
        md = A.AttnMetadata(num_decode=n, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0,
                            slot_mapping=torch.zeros(n, dtype=I32, device=D), decode_block_tables=bt,
                            decode_context_lens=ctx, decode_part_o=ws[0], decode_part_ml=ws[1])
        dec = A.paged_attention(q[j::qr], kc, vcache, md, ac.SCALE)
        same = (dec.view(torch.int16) == out[:, j].view(torch.int16)).all(dim=1)
        assert bool(same.all()), f"row {j}: sequences {[(seqs[i].ctx, seqs[i].rows) for i in (~same).nonzero().flatten().tolist()]}"


@torch.inference_mode()
def test_graph_replay_with_rewritten_inputs():
    """One captured launch, replayed on other sequences: context_lens, n_rows, the block tables and
    the queries are rewritten in place between replays.  (Under inference mode, as the engine captures:
    a capture updates the process-wide generator state, which an engine's capture earlier in the
    process may have created as inference tensors.)"""
    name = "g4_qr4_kv2"
    c, ref = vc.case(name), vc.case_ref(name)
    n = 8
    picks = [list(range(i, i + n)) for i in (0, 9, 30)] + [list(range(len(c.seqs) - n, len(c.seqs)))]
    kc, vcache = c.kc.to(D), c.vc.to(D)
    ws = A.verify_workspace(n, c.qr, c.nq, c.bt.shape[1], c.bs, D)
    sub0, _ = vc.subset(c, ref, picks[0])
    md = md_for(sub0, ws)
    q = wide_q(sub0)
    out = nan_out(sub0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.paged_verify(q, kc, vcache, md, ac.SCALE, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.paged_verify(q, kc, vcache, md, ac.SCALE, out=out)
    for idx in picks[1:] + picks[:1]:
        sub, sref = vc.subset(c, ref, idx)
        md.verify_context_lens.copy_(torch.tensor(sub.ctxs, dtype=I32))
        md.verify_rows.copy_(torch.tensor(sub.rows, dtype=I32))
        md.verify_block_tables.copy_(sub.bt)
        q.copy_(sub.q)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ac.check(out, sref, f"replay on sequences {idx[0]}..")
        check_zeros(out, sub, "replay")


def raw_call(c, kc, vcache, qr, kv_dtype=0, out_stride=None):
    lib = native.lib()
    n = len(c.seqs)
    q = c.q.to(D)
    out = torch.zeros((n * c.qr, c.nq * HD), dtype=torch.bfloat16, device=D)
    ws = A.verify_workspace(n, c.qr, c.nq, c.bt.shape[1], c.bs, D)
    bt = c.bt.to(D)
    rc = lib.pk_paged_verify(out.data_ptr(), q.data_ptr(), kc.data_ptr(), vcache.data_ptr(), bt.data_ptr(),
                             torch.tensor(c.ctxs, dtype=I32, device=D).data_ptr(),
                             torch.tensor(c.rows, dtype=I32, device=D).data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(),
                             n, qr, c.nq, c.nkv, c.bs, bt.stride(0), q.stride(0), out_stride or out.stride(0),
                             float(ac.SCALE), 0, kv_dtype, native.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_refusals():
    """-1, and nothing launched: an FP8 cache, more columns than the tile has, no row at all,
    output rows that are not contiguous."""
    c = vc.case("g4_qr4_kv1")
    kc, vcache = c.kc.to(D), c.vc.to(D)
    assert raw_call(c, kc, vcache, c.qr) == 0
    assert raw_call(c, kc.view(torch.uint8), vcache.view(torch.uint8), c.qr, kv_dtype=1) == -1
    assert raw_call(c, kc, vcache, 5) == -1          # 5 rows x 4 heads = 20 columns
    assert raw_call(c, kc, vcache, 0) == -1
    assert raw_call(c, kc, vcache, c.qr, out_stride=2 * c.nq * HD) == -1
    c8 = vc.case("g8_qr2_kv1")
    assert raw_call(c8, c8.kc.to(D), c8.vc.to(D), 3) == -1   # 3 x 8 = 24
    with pytest.raises(TypeError, match="bfloat16"):
        A.paged_verify(c.q.to(D), kc.to(reference.FP8), vcache.to(reference.FP8), md_for(c, (None, None)), ac.SCALE)
    with pytest.raises(ValueError, match="qr"):
        md = md_for(c, (None, None))
        md.verify_qr = 5
        A.paged_verify(c.q[:20].to(D), kc, vcache, md, ac.SCALE)
