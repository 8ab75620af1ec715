"""Inputs, a float64 reference and the acceptance criterion shared by the exact attention tests:
tests/kernels/test_attention_exact.py (the HIP kernels) and tests/unit/test_attention_cases.py
(the CPU proof that those tests can fail).  Everything here runs on the CPU.

Criterion.  ``|out - ref64| <= 2.25 u A + 1e-30`` per output element, ``u = 2^-8`` (bf16 unit
roundoff), ``A = sum_j p_j |v_j|``.  The kernels round P to bf16 before the PV MFMA (u A), sum
the denominator from the unrounded p, and round the output to bf16 once (u |out| <= u A);
everything else is fp32.  2.25 is 2 plus 1/8 for the fp32 terms.

Inputs.  Random attention data hides a lost key: the output shrinks like 1/sqrt(ctx) and no key
carries weight.  Here every query head has the component ``C`` along the unit direction ``E``,
background keys have no component along ``E``, and a *needle* is the key ``gamma E`` with a +-4
value row, ``gamma`` such that its score is ln(ctx) + 1 above the background: each needle holds a
weight between 0.05 and 1 at every context length, and losing one moves the output by tens of
bounds.  Whatever a sequence does not own is *poison*, finite but loud: the slots of its last
block past ctx, every unowned block, and the block-table entries past its blocks (they point at
a valid all-poison block).  Poison V is 2^100; poison K is 0 ("quiet": any non-zero weight shows)
or 2^10 E ("loud": the key would win the softmax).

All values are bf16 numbers on the grid 2^-10 below 2^6, so fp32 sums of a few of them are exact
(the fused decode kernels are fed split-K slabs whose sum must be unambiguous).
"""
import dataclasses
import functools
import math

import numpy as np
import torch

HD = 128
U = 2.0 ** -8
BOUND = 2.25
FLOOR = 1e-30
C = 4.0
SCALE = 1.0 / math.sqrt(HD)
POISON_V = 2.0 ** 100
LOUD_K = 2.0 ** 10
MAX_NEEDLES = 8
DECODE_FILL = 64        # csrc/kernels/attention.hip g_decode_fill
DECODE_Z = 4            # g_decode_z
PART, PART_SMALL = 512, 128

# the unit direction: one entry of +-1/4 in each of the 16 8-dim granules of a row
E = np.zeros(HD)
for _i in range(16):
    E[8 * _i + (3 * _i) % 8] = 0.25 * (1 if (_i * (_i + 1) // 2) % 2 == 0 else -1)


# ------------------------------------------------------------------ cache layout (common.h)
def kcache_off(k_in_block, d):
    """Offset of K element (token, dim) inside one (block, kv head) slab: 32-token tiles of
    MFMA A-fragments, ((t * 4 + kk) * 64 + lane) * 8 + j."""
    k = k_in_block & 31
    lane = 16 * (d >> 5) + 4 * (k >> 3) + (k & 3)
    return (k_in_block >> 5) * 4096 + ((((k >> 2) & 1) * 4 + ((d >> 3) & 3)) * 64 + lane) * 8 + (d & 7)


def vcache_off(k_in_block, d):
    """Offset of V element (token, dim): per 32-token tile [d / 16][key / 8][d % 16][key % 8]."""
    k = k_in_block & 31
    return (k_in_block >> 5) * 4096 + ((((d >> 4) << 2) + (k >> 3)) * 16 + (d & 15)) * 8 + (k & 7)


def _offsets(fn, tok_in_block):
    """[n, 128] offsets of the rows ``tok_in_block`` (int array)."""
    return fn(np.asarray(tok_in_block, dtype=np.int64)[:, None], np.arange(HD, dtype=np.int64)[None, :])


# ---------------------------------------------------------------------------------- values
def grid(x) -> torch.Tensor:
    """-> bf16 tensor of the nearest values that are multiples of 2^-10 as well."""
    x = np.asarray(x, dtype=np.float64)
    assert np.abs(x).max(initial=0.0) < 64
    t = torch.from_numpy(np.round(x * 1024) / 1024).to(torch.bfloat16)
    assert torch.equal((t.double() * 1024).round() / 1024, t.double())
    return t


def gamma_for(ctx: int) -> float:
    """Needle length: score C gamma / sqrt(128) = ln(ctx) + 1 (background scores: mean 0, sd 1/2)."""
    return (math.log(ctx) + 1.0) * math.sqrt(HD) / C


def _perp(x):
    return x - (x @ E)[..., None] * E


# ----------------------------------------------------------------------------------- cases
@dataclasses.dataclass
class Seq:
    ctx: int          # keys, the new tokens included
    qlen: int         # query tokens (1: decode)
    needles: tuple    # key indices
    tags: tuple = ()  # which of the listed positions the needles stand for


@dataclasses.dataclass
class Case:
    name: str
    nq: int
    nkv: int
    bs: int
    poison: str
    seqs: list
    q: torch.Tensor         # [T, nq, 128] bf16 (post-RoPE)
    kc: torch.Tensor        # [blocks, nkv, bs, 128] bf16, physical layout
    vc: torch.Tensor        # [blocks, nkv, 128, bs] bf16, physical layout
    bt: torch.Tensor        # [n_seqs, max_blocks] int32
    poison_block: int
    num_decode: int = 0     # leading sequences that are decode tokens
    kpart: int = 0          # decode: keys per partition the launch must take
    decode_max_ctx: int = 0
    n_parts: int = 0

    @property
    def ctxs(self):
        return [s.ctx for s in self.seqs]

    @property
    def cu_q(self):
        return [0] + list(np.cumsum([s.qlen for s in self.seqs]))

    @property
    def G(self):
        return self.nq // self.nkv


def poison_rows(poison: str):
    """(K row, V row) of a slot no sequence owns."""
    k = np.zeros(HD) if poison == "quiet" else LOUD_K * E
    assert poison in ("quiet", "loud")
    return k, np.full(HD, POISON_V)


def build_case(name, nq, nkv, bs, poison, seqs, extra_cols=1, seed=0) -> Case:
    """Cache, block tables and queries of ``seqs``; blocks handed out in a shuffled order, three
    blocks left unowned, one more all-poison block behind every unused block-table entry."""
    rng = np.random.RandomState(seed)
    nblk = [(s.ctx + bs - 1) // bs for s in seqs]
    num_blocks = sum(nblk) + 4
    perm = rng.permutation(num_blocks).tolist()
    poison_block = perm.pop()
    pk, pv = poison_rows(poison)
    kc = torch.empty(num_blocks, nkv, bs * HD, dtype=torch.bfloat16)
    vc = torch.empty(num_blocks, nkv, bs * HD, dtype=torch.bfloat16)
    alltok = np.arange(bs)
    kc[:, :, torch.from_numpy(_offsets(kcache_off, alltok))] = torch.tensor(pk).to(torch.bfloat16)
    vc[:, :, torch.from_numpy(_offsets(vcache_off, alltok))] = torch.tensor(pv).to(torch.bfloat16)
    max_blocks = max(nblk + [1]) + extra_cols
    bt = torch.full((len(seqs), max_blocks), poison_block, dtype=torch.int32)
    qs = []
    heads = torch.arange(nkv).view(1, nkv, 1)
    for s, seq in enumerate(seqs):
        assert len(seq.needles) <= MAX_NEEDLES and all(0 <= n < seq.ctx for n in seq.needles)
        r = _perp(rng.standard_normal((seq.qlen, nq, HD)) * 0.5)
        qs.append(grid(r + C * E))
        if seq.ctx == 0:
            continue
        blocks = [perm.pop() for _ in range(nblk[s])]
        bt[s, :nblk[s]] = torch.tensor(blocks, dtype=torch.int32)
        k = _perp(rng.standard_normal((seq.ctx, nkv, HD)))
        v = rng.standard_normal((seq.ctx, nkv, HD))
        for n in seq.needles:
            k[n] = gamma_for(seq.ctx) * E
            v[n] = rng.choice([-4.0, 4.0], size=(nkv, HD))
        j = np.arange(seq.ctx)
        blk = torch.tensor(blocks)[torch.from_numpy(j // bs)].view(-1, 1, 1)
        kc[blk, heads, torch.from_numpy(_offsets(kcache_off, j % bs)).view(-1, 1, HD)] = grid(k)
        vc[blk, heads, torch.from_numpy(_offsets(vcache_off, j % bs)).view(-1, 1, HD)] = grid(v)
    return Case(name, nq, nkv, bs, poison, list(seqs), torch.cat(qs), kc.view(num_blocks, nkv, bs, HD),
                vc.view(num_blocks, nkv, HD, bs), bt, poison_block)


# ------------------------------------------------------------------------ float64 reference
def gather64(case: Case, bt_row, n_keys: int):
    """Logical K, V [n_keys, nkv, 128] float64 of one block-table row, by the layout formulas."""
    j = np.arange(n_keys)
    blk = torch.as_tensor(bt_row).long()[torch.from_numpy(j // case.bs)].view(-1, 1, 1)
    heads = torch.arange(case.nkv).view(1, case.nkv, 1)
    nb = case.kc.shape[0]
    k = case.kc.reshape(nb, case.nkv, -1)[blk, heads, torch.from_numpy(_offsets(kcache_off, j % case.bs)).view(-1, 1, HD)]
    v = case.vc.reshape(nb, case.nkv, -1)[blk, heads, torch.from_numpy(_offsets(vcache_off, j % case.bs)).view(-1, 1, HD)]
    return k.double(), v.double()


def seq_attention64(case: Case, s: int, mutant=None, bf16_p=False):
    """Causal GQA attention of sequence ``s`` in float64: query l of its qlen tokens sits at
    position ctx - qlen + l and attends to keys [0, position].
    -> (out [qlen, nq, 128], A = sum_j p_j |v_j| [qlen, nq, 128], p [nq, qlen, keys]).

    ``mutant`` makes it wrong on purpose (the CPU self-check): ("omit_key", i), ("include_ctx",),
    ("swap_bt", a, b), ("causal", +-1), ("omit_partition", part, keys per partition).
    ``bf16_p``: the kernels' arithmetic instead -- P = exp(s - max) rounded to bf16 for the PV
    product, denominator from the unrounded p, output rounded to bf16."""
    seq = case.seqs[s]
    L, ctx, nq = seq.qlen, seq.ctx, case.nq
    if ctx == 0 or L == 0:
        z = torch.zeros(L, nq, HD, dtype=torch.float64)
        return z, z.clone(), torch.zeros(nq, L, 0, dtype=torch.float64)
    kind = mutant[0] if mutant else None
    bt_row = case.bt[s].clone()
    if kind == "swap_bt":
        a, b = mutant[1], mutant[2]
        bt_row[a], bt_row[b] = case.bt[s, b], case.bt[s, a]
    n = ctx + (1 if kind == "include_ctx" else 0)
    delta = mutant[1] if kind == "causal" else 0   # the causal limit alone: keys stay below ctx
    k, v = gather64(case, bt_row, n)
    a0 = case.cu_q[s]
    q = case.q[a0:a0 + L].double()
    g = case.G
    k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)   # [n, nq, 128]
    scores = torch.einsum("lhd,jhd->hlj", q, k) * SCALE
    pos = torch.arange(ctx - L, ctx).view(L, 1) + delta
    keys = torch.arange(n).view(1, n)
    dead = keys > pos
    if kind == "include_ctx":
        dead = keys > pos + 1
    if kind == "omit_key":
        dead = dead | (keys == mutant[1])
    if kind == "omit_partition":
        dead = dead | ((keys >= mutant[1] * mutant[2]) & (keys < (mutant[1] + 1) * mutant[2]))
    scores = scores.masked_fill(dead[None], float("-inf"))
    m = scores.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))    # a query left without keys -> zeros
    pu = torch.exp(scores - m)
    den = pu.sum(-1, keepdim=True)
    den = torch.where(den > 0, den, torch.ones_like(den))
    p = pu / den
    if bf16_p:
        out = torch.einsum("hlj,jhd->lhd", pu.to(torch.bfloat16).double(), v) / den[..., 0].t()[..., None]
        out = out.to(torch.bfloat16).double()
    else:
        out = torch.einsum("hlj,jhd->lhd", p, v)
    return out, torch.einsum("hlj,jhd->lhd", p, v.abs()), p


@dataclasses.dataclass
class Ref:
    out: torch.Tensor   # [T, nq, 128] float64
    A: torch.Tensor
    p: list             # per sequence [nq, qlen, ctx]


def reference(case: Case) -> Ref:
    parts = [seq_attention64(case, s) for s in range(len(case.seqs))]
    return Ref(torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts]), [x[2] for x in parts])


def ratio(out, ref64, A) -> float:
    """Largest |out - ref64| / (u A) (inf where the output is not finite or A = 0 is missed)."""
    err = (out.double() - ref64).abs()
    inf, zero = torch.full_like(err, math.inf), torch.zeros_like(err)
    r = torch.where(A > 0, err / (U * A).clamp(min=1e-300), torch.where(err > FLOOR, inf, zero))
    r = torch.where(torch.isfinite(out.double()), r, inf)
    return float(r.max()) if r.numel() else 0.0


def accepted(out, ref64, A) -> torch.Tensor:
    """Per query head [T, nq]: every element within 2.25 u A + 1e-30 of the reference."""
    err = (out.double() - ref64).abs()
    return (err <= BOUND * U * A + FLOOR).all(dim=-1)   # NaN compares false


def check(out, ref: Ref, what=""):
    """Assert the criterion on ``out`` [T, nq * 128] or [T, nq, 128]; -> largest ratio."""
    out = out.reshape(ref.out.shape).cpu()
    ok = accepted(out, ref.out, ref.A)
    r = ratio(out, ref.out, ref.A)
    if not bool(ok.all()):
        bad = (~ok).nonzero().tolist()
        t, h = bad[0]
        e = (out[t, h].double() - ref.out[t, h]).abs() / (U * ref.A[t, h]).clamp(min=1e-300)
        raise AssertionError(f"{what}: {len(bad)} query heads outside {BOUND} u A; first (token {t}, head {h}), "
                             f"|out - ref| / (u A) = {float(e.max()):.3g} at dim {int(e.argmax())}; "
                             f"got {out[t, h, int(e.argmax())].item()!r} want {ref.out[t, h, int(e.argmax())].item()!r}; "
                             f"(token, head) list {bad[:12]}")
    return r


# ---------------------------------------------------------------- decode: dispatch and cases
def decode_dispatch(n_seqs: int, nkv: int, max_ctx: int):
    """csrc/kernels/attention.hip decode_plan, at the default fill 64 and
    z cap 4 -> (keys per partition, n_parts, grid z)."""
    big = (max_ctx + PART - 1) // PART
    part = PART_SMALL if n_seqs * nkv * min(big, DECODE_Z) < DECODE_FILL else PART
    n_parts = (max_ctx + part - 1) // part
    return part, n_parts, min(n_parts, DECODE_Z)


def decode_needles(ctx: int, bs: int, kpart: int):
    """The listed key positions that exist in a context, as chunks of at most 8 needles: each chunk
    becomes a sequence of its own, and each holds key ctx - 1 (the new token).
    -> [(needles, tags)]"""
    if ctx == 0:
        return [((), ())]
    n_parts = (ctx + kpart - 1) // kpart
    named = [(0, "0"), (31, "31"), (32, "32"), (bs - 1, "bs-1"), (bs, "bs"), (kpart - 1, "kpart-1"), (kpart, "kpart")]
    named += [(p * kpart, "part_first") for p in range(1, n_parts)]
    named += [((n_parts - 1) * kpart, "last_part_first"), ((ctx - 1) & ~31, "tail32"), (((ctx - 1) >> 3) << 3, "tail8"),
              (ctx - 2, "ctx-2")]
    tags = {}
    for k, t in named:
        if 0 <= k < ctx:
            tags.setdefault(k, []).append(t)
    tags.setdefault(ctx - 1, []).append("ctx-1")
    rest = sorted(k for k in tags if k != ctx - 1)
    chunks = [rest[i:i + MAX_NEEDLES - 1] for i in range(0, len(rest), MAX_NEEDLES - 1)] or [[]]
    return [(tuple(c + [ctx - 1]), tuple(sorted({t for k in c + [ctx - 1] for t in tags[k]}))) for c in chunks]


BASE_CTXS = (1, 8, 31, 32, 33, 127, 128, 129, 512, 513)

# name -> (nq, nkv, bs, poison, contexts, keys per partition, decode_max_ctx rule)
#   "zero": 0 (the block-table capacity decides n_parts), "exact": max(ctx), "plus": max(ctx) + one
#   partition.  The block tables are two partitions wider than the longest context, so the three
#   rules give three different n_parts.  A context of 0 is a padded row.
DECODE_CASES = {
    # 128-key partitions: n_seqs * n_kv * z < 64; 700 keys: workgroups z = 0, 1 walk partitions z and z + 4
    "p128_g8_bs32_quiet": (8, 1, 32, "quiet", BASE_CTXS + (700,), 128, "zero"),
    "p128_g16_bs96_loud": (16, 1, 96, "loud", BASE_CTXS + (700,), 128, "exact"),
    "p128_g4_bs64_loud": (4, 1, 64, "loud", BASE_CTXS + (700, 0), 128, "plus"),
    # 512-key partitions; 2100 keys: workgroup z = 0 walks partitions 0 and 4
    "p512_g4_bs32_loud": (32, 8, 32, "loud", BASE_CTXS + (1600, 2100, 0), 512, "zero"),
    "p512_g1_bs64_quiet": (8, 8, 64, "quiet", BASE_CTXS + (1600, 2100), 512, "exact"),
    "p512_g4_bs96_quiet": (32, 8, 96, "quiet", BASE_CTXS + (1600, 2100), 512, "plus"),
    # n_parts == 1: every sequence finishes in place, no merge launch
    "single_g4_bs32_loud": (32, 8, 32, "loud", BASE_CTXS[:-1], 512, "exact"),
    "single_g8_bs96_quiet": (8, 1, 96, "quiet", BASE_CTXS[:7], 128, "exact"),
}


@functools.lru_cache(maxsize=None)
def decode_case(name: str) -> Case:
    nq, nkv, bs, poison, ctxs, kpart, rule = DECODE_CASES[name]
    seqs = [Seq(c, 1, n, t) for c in ctxs for n, t in decode_needles(c, bs, kpart)]
    case = build_case(name, nq, nkv, bs, poison, seqs, extra_cols=(2 * kpart + bs - 1) // bs + 1,
                      seed=1 + list(DECODE_CASES).index(name))
    mx = max(ctxs)
    case.decode_max_ctx = {"zero": 0, "exact": mx, "plus": mx + kpart}[rule]
    case.num_decode = len(seqs)
    case.kpart, case.n_parts, _ = decode_dispatch(len(seqs), nkv, case.decode_max_ctx or case.bt.shape[1] * bs)
    assert case.kpart == kpart, (name, case.kpart)
    return case


@functools.lru_cache(maxsize=None)
def decode_ref(name: str) -> Ref:
    return reference(decode_case(name))


def reversed_case(case: Case) -> Case:
    """The same sequences in the opposite order (decode: one query each): a second launch on the
    same workspace then finds another sequence's partials in every slot."""
    assert all(s.qlen == 1 for s in case.seqs)
    return dataclasses.replace(case, seqs=case.seqs[::-1], q=case.q.flip(0), bt=case.bt.flip(0))


def reversed_ref(ref: Ref) -> Ref:
    return Ref(ref.out.flip(0), ref.A.flip(0), ref.p[::-1])


# ------------------------------------------------------------------------------ fused decode
@dataclasses.dataclass
class FusedInputs:
    slabs: torch.Tensor      # [S, B, N] fp32, summing exactly to ``target``
    target: torch.Tensor     # [B, N] bf16: pre-RoPE q | k | v rows of the new tokens
    positions: torch.Tensor  # [B] int32
    slots: torch.Tensor      # [B] int32, -1 for a padded row
    cos_sin: torch.Tensor    # [max_pos, 128] fp32, exact quarter turns
    kc0: torch.Tensor        # the cache before the launch: the new tokens' rows hold poison
    vc0: torch.Tensor


def quarter_turn_table(max_pos: int, seed=0) -> torch.Tensor:
    """cos | sin rows whose (cos, sin) pairs are (1,0), (0,1), (-1,0), (0,-1), chosen
    pseudo-randomly per (position, column): the rotation is exact in any precision."""
    k = np.random.RandomState(1000 + seed).randint(0, 4, size=(max_pos, HD // 2))
    cos = np.array([1.0, 0.0, -1.0, 0.0])[k]
    sin = np.array([0.0, 1.0, 0.0, -1.0])[k]
    return torch.from_numpy(np.concatenate([cos, sin], axis=1)).float()


def unrotate(x: torch.Tensor, cs_row: torch.Tensor) -> torch.Tensor:
    """Inverse of the neox rotation (a, b) = (x c - y s, y c + x s) on [..., 128] rows."""
    c, s = cs_row[:64].double(), cs_row[64:].double()
    a, b = x[..., :64].double(), x[..., 64:].double()
    return torch.cat([a * c + b * s, b * c - a * s], dim=-1)


def sequential_sum(slabs: torch.Tensor) -> torch.Tensor:
    """fp32 sum of the slabs in the kernels' order (slab 0 first)."""
    acc = torch.zeros_like(slabs[0])
    for sp in range(slabs.shape[0]):
        acc = acc + slabs[sp]
    return acc


def fused_inputs(case: Case, S: int, fold: bool, seed=0) -> FusedInputs:
    """Split-K slabs, positions, slots and rotation table from which the fused decode kernels
    must rebuild ``case``: the post-RoPE queries are case.q and the new token of every sequence
    is its key ctx - 1 (a needle), whose cache row holds poison until the kernel writes it.
    ``fold``: the new token's position is ctx - 1; else ctx // 2 (the kernel then stores the row
    before attending).  Every slab sum is exact: multiples of 2^-10 below 2^9."""
    rng = np.random.RandomState(2000 + seed)
    B, nq, nkv, bs = len(case.seqs), case.nq, case.nkv, case.bs
    ctxs = case.ctxs
    pos = [max(c - 1, 0) if fold else c // 2 for c in ctxs]
    cs = quarter_turn_table(max(max(ctxs), 1), seed)
    kc0, vc0 = case.kc.clone(), case.vc.clone()
    nb = kc0.shape[0]
    kf, vf = kc0.view(nb, nkv, -1), vc0.view(nb, nkv, -1)
    pk, pv = (torch.tensor(x).to(torch.bfloat16) for x in poison_rows(case.poison))
    target = grid(rng.standard_normal((B, nq + 2 * nkv, HD)))    # padded rows: anything
    slots = []
    for s, c in enumerate(ctxs):
        if c == 0:
            slots.append(-1)
            continue
        blk, off = int(case.bt[s, (c - 1) // bs]), (c - 1) % bs
        slots.append(blk * bs + off)
        ko = torch.from_numpy(_offsets(kcache_off, [off]))[0]
        vo = torch.from_numpy(_offsets(vcache_off, [off]))[0]
        target[s, :nq] = unrotate(case.q[s], cs[pos[s]]).to(torch.bfloat16)
        target[s, nq:nq + nkv] = unrotate(kf[blk][:, ko], cs[pos[s]]).to(torch.bfloat16)
        target[s, nq + nkv:] = vf[blk][:, vo]
        kf[blk][:, ko] = pk
        vf[blk][:, vo] = pv
    target = target.view(B, -1)
    parts = rng.randint(-32, 33, size=(S - 1,) + tuple(target.shape)) / 4.0
    last = target.double().numpy() - parts.sum(0)
    slabs = torch.from_numpy(np.concatenate([parts, last[None]])).float()
    assert torch.equal(slabs.double().sum(0), target.double())
    assert torch.equal(sequential_sum(slabs).to(torch.bfloat16), target)
    return FusedInputs(slabs, target, torch.tensor(pos, dtype=torch.int32), torch.tensor(slots, dtype=torch.int32),
                       cs, kc0, vc0)


# ------------------------------------------------------------------------------------ prefill
def prefill_needles(qlen: int, prefix: int):
    """Needles on and just after the causal diagonal of every 16-query group (the first key of
    the group: present from its first query on, absent from the last query of the group before --
    16 covers the 32- and 64-query groups of the MFMA-32 kernel too), at keys 63 and 64 (the
    64-key step) and at ctx - 1."""
    ctx = prefix + qlen
    tags = {}
    for g in range((qlen + 15) // 16):
        tags.setdefault(prefix + 16 * g, []).append("diag")
    for k, t in ((63, "63"), (64, "64"), (ctx - 1, "ctx-1")):
        if 0 <= k < ctx:
            tags.setdefault(k, []).append(t)
    keys = sorted(tags)
    return tuple(keys), tuple(sorted({t for k in keys for t in tags[k]}))


PREFILL_SEQS = ((1, 100), (31, 64), (32, 63), (33, 1), (65, 0), (65, 100), (1, 0), (33, 63), (32, 1))   # (qlen, prefix)

# name -> (nq, nkv, bs, poison, kernel)
PREFILL_CASES = {
    "g1_bs32_quiet": (2, 2, 32, "quiet", "mfma32"),
    "g2_bs64_loud": (4, 2, 64, "loud", "mfma32"),
    "g4_bs96_quiet": (8, 2, 96, "quiet", "mfma32"),
    "g8_bs32_loud": (8, 1, 32, "loud", "mfma32"),
    "g3_bs64_quiet": (6, 2, 64, "quiet", "wave16"),
    "g16_bs32_loud": (16, 1, 32, "loud", "wave16"),
}


def prefill_kernel(G: int) -> str:
    """csrc/kernels/attention.hip pk_paged_prefill: which kernel a GQA group takes."""
    return "mfma32" if G in (1, 2, 4, 8) else "wave16"


def prefill_seqs():
    return [Seq(p + L, L, *prefill_needles(L, p)) for L, p in PREFILL_SEQS]


@functools.lru_cache(maxsize=None)
def prefill_case(name: str) -> Case:
    nq, nkv, bs, poison, _ = PREFILL_CASES[name]
    return build_case(name, nq, nkv, bs, poison, prefill_seqs(), seed=50 + list(PREFILL_CASES).index(name))


@functools.lru_cache(maxsize=None)
def prefill_ref(name: str) -> Ref:
    return reference(prefill_case(name))


# -------------------------------------------------------------------------------------- mixed
MIXED_DECODE_CTXS = (33, 513, 700, 1)
MIXED_PREFILL = ((31, 64), (65, 100), (1, 0))
MIXED_SHAPE = (8, 2, 32, "loud", 128)   # nq, nkv, bs, poison, keys per decode partition


@functools.lru_cache(maxsize=None)
def mixed_case() -> Case:
    nq, nkv, bs, poison, kpart = MIXED_SHAPE
    seqs = [Seq(c, 1, n, t) for c in MIXED_DECODE_CTXS for n, t in decode_needles(c, bs, kpart)]
    nd = len(seqs)
    seqs += [Seq(p + L, L, *prefill_needles(L, p)) for L, p in MIXED_PREFILL]
    case = build_case("mixed", nq, nkv, bs, poison, seqs, seed=90)
    case.num_decode = nd
    case.kpart, case.n_parts, _ = decode_dispatch(nd, nkv, case.bt.shape[1] * bs)
    assert case.kpart == kpart
    return case


@functools.lru_cache(maxsize=None)
def mixed_ref() -> Ref:
    return reference(mixed_case())


# ------------------------------------------------------------------------------------ mutants
def mutants(case: Case, s: int):
    """Wrong references of sequence ``s`` that a correct kernel test must reject
    -> [(label, mutant, queries it touches)].  A mutant *touches* a query when it adds or removes
    a needle or lets poison in: a lost background key carries too little weight for any
    criterion to see, and attention does not depend on the order of fully owned blocks.
      omit_key i        each needle; the queries at or after it
      omit_new_key      decode: key ctx - 1 (the fold path's key)
      include_ctx       decode: the slot after the context (poison)
      causal +1 / -1    the queries that gain the needle just after their diagonal / lose the
                        needle on it (keys stay below ctx: decode is touched by -1 only)
      swap_bt           first and last block, where the last one is partial: poison moves in
      omit_partition    decode: each partition of the launch that holds a needle"""
    seq = case.seqs[s]
    L, ctx, bs = seq.qlen, seq.ctx, case.bs
    if ctx == 0:
        return []
    qpos = [ctx - L + l for l in range(L)]
    out = []
    for n in seq.needles:
        out.append((f"omit_key {n}", ("omit_key", n), [l for l in range(L) if qpos[l] >= n]))
    gain = [l for l in range(L) if qpos[l] + 1 in seq.needles]
    out.append(("causal +1", ("causal", 1), gain))
    out.append(("causal -1", ("causal", -1), [l for l in range(L) if qpos[l] in seq.needles]))
    nblk = (ctx + bs - 1) // bs
    if nblk >= 2 and ctx % bs:
        out.append(("swap_bt", ("swap_bt", 0, nblk - 1), [L - 1]))
    if L == 1 and case.kpart:
        out.append(("omit_new_key", ("omit_key", ctx - 1), [0]))
        out.append(("include_ctx", ("include_ctx",), [0]))
        for part in sorted({n // case.kpart for n in seq.needles}):
            out.append((f"omit_partition {part}", ("omit_partition", part, case.kpart), [0]))
    return [m for m in out if m[2]]
