"""Inputs and the float64 reference of the verify-attention tests (speculative decoding):
tests/kernels/test_attention_verify.py (the HIP kernel) and tests/unit/test_attention_verify_cases.py
(the CPU proof that those inputs can fail).  Everything here runs on the CPU.

The contract (ops/attention.py paged_verify): sequence s owns ``qr`` query rows ``s * qr + j``, the
first ``R`` real; ``C`` counts the cached keys including the R written this step; row ``j < R``
attends keys ``0 .. C - R + j``, every other row is zeros.

Inputs follow tests/attention_cases.py: every query -- the padding rows' too -- carries the
component ``C_Q`` along the unit direction E, background keys have none, and a *needle* is the key
``gamma E`` with a +-4 value row.  The needles of a sequence are the R keys written this step
(``C - R .. C - 1``) and a few fixed positions before them, so for row j the key on its limit is a
needle it must see, and the keys of the *later* drafts, beyond its limit but inside C, are needles
it must not see: one key too many or too few moves the output by many bounds.  Whatever a sequence
does not own is poison as in attention_cases (V = 2^100, K quiet or loud).  The criterion is
attention_cases' unchanged: ``|out - ref64| <= 2.25 u A + 1e-30``.
"""
import dataclasses
import functools

import numpy as np
import torch

from polykey_service_amd.ops import reference
from tests import attention_cases as ac

HD = ac.HD
CTXS = (31, 32, 33, 127, 128, 129, 131, 511, 512, 513, 515, 1100)   # and C = R, for every R
FIXED_NEEDLES = (0, 126, 128, 510, 512)

# name -> (G, qr, n_kv, block size, poison)
CASES = {
    "g4_qr4_kv1": (4, 4, 1, 32, "loud"),
    "g4_qr4_kv2": (4, 4, 2, 64, "quiet"),
    "g4_qr2_kv1": (4, 2, 1, 96, "quiet"),
    "g4_qr2_kv2": (4, 2, 2, 32, "loud"),
    "g8_qr2_kv1": (8, 2, 1, 32, "loud"),
    "g8_qr2_kv2": (8, 2, 2, 64, "quiet"),
    "g2_qr5_kv1": (2, 5, 1, 64, "loud"),
    "g2_qr5_kv2": (2, 5, 2, 32, "quiet"),
    "g1_qr16_kv1": (1, 16, 1, 32, "quiet"),
    "g1_qr16_kv2": (1, 16, 2, 96, "loud"),
}


@dataclasses.dataclass
class VSeq:
    ctx: int   # C: keys cached, the R new ones included (0: a padded sequence)
    rows: int  # R


@dataclasses.dataclass
class VCase:
    name: str
    nq: int
    nkv: int
    qr: int
    bs: int
    poison: str
    seqs: list
    q: torch.Tensor    # [n_seqs * qr, nq, 128] bf16
    kc: torch.Tensor   # [blocks, nkv, bs, 128] bf16, physical layout
    vc: torch.Tensor   # [blocks, nkv, 128, bs] bf16, physical layout
    bt: torch.Tensor   # [n_seqs, max_blocks] int32, scattered

    @property
    def G(self):
        return self.nq // self.nkv

    @property
    def ctxs(self):
        return [s.ctx for s in self.seqs]

    @property
    def rows(self):
        return [s.rows for s in self.seqs]


def case_seqs(qr: int):
    """Every R in 1..qr with C = R and with every listed context, and two padded sequences."""
    seqs = [VSeq(R, R) for R in range(1, qr + 1)]
    seqs += [VSeq(C, R) for C in CTXS for R in range(1, qr + 1)]
    seqs.insert(3, VSeq(0, 1))
    seqs.append(VSeq(0, qr))
    return seqs


def needles_of(seq: VSeq):
    new = list(range(seq.ctx - seq.rows, seq.ctx))
    return sorted(set(new) | {k for k in FIXED_NEEDLES if k < seq.ctx - seq.rows})


def build(name, G, qr, nkv, bs, poison, seqs, seed=0) -> VCase:
    """Cache, scattered block tables and queries; one all-poison block behind every unused
    block-table entry, two entries more than the longest context needs."""
    rng = np.random.RandomState(seed)
    nq = G * nkv
    nblk = [(s.ctx + bs - 1) // bs for s in seqs]
    num_blocks = sum(nblk) + 4
    perm = rng.permutation(num_blocks).tolist()
    poison_block = perm.pop()
    pk, pv = ac.poison_rows(poison)
    kc = torch.empty(num_blocks, nkv, bs * HD, dtype=torch.bfloat16)
    vc = torch.empty(num_blocks, nkv, bs * HD, dtype=torch.bfloat16)
    alltok = np.arange(bs)
    kc[:, :, torch.from_numpy(ac._offsets(ac.kcache_off, alltok))] = torch.tensor(pk).to(torch.bfloat16)
    vc[:, :, torch.from_numpy(ac._offsets(ac.vcache_off, alltok))] = torch.tensor(pv).to(torch.bfloat16)
    bt = torch.full((len(seqs), max(nblk) + 2), poison_block, dtype=torch.int32)
    heads = torch.arange(nkv).view(1, nkv, 1)
    qs = []
    for s, seq in enumerate(seqs):
        qs.append(ac.grid(ac._perp(rng.standard_normal((qr, nq, HD)) * 0.5) + ac.C * ac.E))
        if seq.ctx == 0:
            continue
        blocks = [perm.pop() for _ in range(nblk[s])]
        bt[s, :nblk[s]] = torch.tensor(blocks, dtype=torch.int32)
        k = ac._perp(rng.standard_normal((seq.ctx, nkv, HD)))
        v = rng.standard_normal((seq.ctx, nkv, HD))
        for n in needles_of(seq):
            k[n] = ac.gamma_for(seq.ctx) * ac.E
            v[n] = rng.choice([-4.0, 4.0], size=(nkv, HD))
        j = np.arange(seq.ctx)
        blk = torch.tensor(blocks)[torch.from_numpy(j // bs)].view(-1, 1, 1)
        kc[blk, heads, torch.from_numpy(ac._offsets(ac.kcache_off, j % bs)).view(-1, 1, HD)] = ac.grid(k)
        vc[blk, heads, torch.from_numpy(ac._offsets(ac.vcache_off, j % bs)).view(-1, 1, HD)] = ac.grid(v)
    return VCase(name, nq, nkv, qr, bs, poison, list(seqs), torch.cat(qs), kc.view(num_blocks, nkv, bs, HD),
                 vc.view(num_blocks, nkv, HD, bs), bt)


@functools.lru_cache(maxsize=None)
def case(name: str) -> VCase:
    G, qr, nkv, bs, poison = CASES[name]
    return build(name, G, qr, nkv, bs, poison, case_seqs(qr), seed=300 + list(CASES).index(name))


def ref64(c: VCase, mutant=None) -> ac.Ref:
    out, A = reference.paged_verify(c.q, c.kc, c.vc, c.bt, c.ctxs, c.rows, c.qr, ac.SCALE, dtype=torch.float64,
                                    mutant=mutant)
    return ac.Ref(out, A, [])


@functools.lru_cache(maxsize=None)
def case_ref(name: str) -> ac.Ref:
    return ref64(case(name))


def subset(c: VCase, ref: ac.Ref, idx):
    """The sequences ``idx`` of a case as a launch of their own (same cache), with their reference."""
    rows = torch.tensor([s * c.qr + j for s in idx for j in range(c.qr)], dtype=torch.long)
    sub = dataclasses.replace(c, seqs=[c.seqs[s] for s in idx], q=c.q[rows], bt=c.bt[torch.tensor(idx)])
    return sub, ac.Ref(ref.out[rows], ref.A[rows], [])


def small_partition_chunk(nkv: int, max_ctx: int) -> int:
    """The most sequences a launch may hold and still take 128-key partitions (decode_plan)."""
    big = (max_ctx + ac.PART - 1) // ac.PART
    return (ac.DECODE_FILL - 1) // (nkv * min(big, ac.DECODE_Z))
