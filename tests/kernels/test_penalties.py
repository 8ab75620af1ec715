"""Penalty kernels (csrc/kernels/penalties.hip) and pk_sample_alt against the reference
(ops/reference.py penalty_*), which works on the same packed 16-bit table.

Exact cases: bf16 logits on a 1/8 grid (|x| <= 16), r in {1, 2, 0.5, 4}, freq / pres on a 1/16
grid (|.| <= 2), counts <= 64 (plus two saturated at 0x7fff), biases on a 1/4 grid (|b| <= 100).
x / r and x * r stay on a 1/32 grid below 64, f * c on a 1/16 grid below 2^16, the sums on a 1/32
grid below 2^17: 22 bits at most, so every intermediate is exact in fp32 (and a contracted fma
would change nothing); the comparison is bitwise.  The fp32 reference equals its own float64 form
on these inputs (asserted below).

Realistic values: |got - ref64| <= 4 * 2^-24 * (|x| * max(r, 1/r) + |f| * c + |p| + |b|) per
element: four roundings (division or product, f * c, two subtractions / the bias add share the
last two), each at most half an ulp of a value bounded by the running magnitude.
"""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import penalties, sampler
from polykey_service_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0ABCD
SLOTS = [3, -1, 0, -1, 7]
N_SLOTS = 8


def _to(st, device):
    out = penalties.PenaltyState.__new__(penalties.PenaltyState)
    out.n_slots, out.vocab, out.stride = st.n_slots, st.vocab, st.stride
    for k in ("counts", "bias_ids", "bias_vals", "bias_n", "out"):
        setattr(out, k, getattr(st, k).to(device).contiguous())
    return out


def _state(V, seed, n_bias=(0, 300, 7), max_count=64, exact=True):
    """An 8-slot CPU state with random history in every slot (also the unused ones)."""
    g = torch.Generator().manual_seed(seed)
    st = penalties.PenaltyState(N_SLOTS, V, "cpu")
    c = st.counts.numpy().view(np.uint16)
    for slot in range(N_SLOTS):
        n_seen = min(V, 40)
        idx = torch.randperm(V, generator=g)[:n_seen].numpy()
        cnt = torch.randint(0, max_count + 1, (n_seen,), generator=g).numpy().astype(np.uint16)
        flag = (torch.randint(0, 2, (n_seen,), generator=g).numpy().astype(np.uint16)) << 15
        c[slot, idx] = cnt | flag
        c[slot, 0] = 0x8000 | 3                    # token 0: prompt and output
        c[slot, V - 1] = 5                         # token V-1: output only
    if V > 16:
        c[3, 11] = 0x7FFF                          # saturated counts, without and with the flag
        c[3, 12] = 0xFFFF
    for slot, nb in zip((3, 0, 7), n_bias):
        nb = min(nb, V)
        ids = torch.randperm(V, generator=g)[:nb]
        if nb >= 2:
            ids[0], ids[1] = 0, V - 1              # bias on the edges
            ids[2:] = torch.tensor([i for i in torch.randperm(V, generator=g).tolist() if i not in (0, V - 1)][:nb - 2])
        vals = torch.randint(-400, 401, (nb,), generator=g).float() / 4 if exact else (torch.rand(nb, generator=g) * 200 - 100)
        st.bias_ids[slot, :nb] = ids.to(torch.int32)
        st.bias_vals[slot, :nb] = vals
        st.bias_n[slot] = nb
    return st


def _exact_inputs(V, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(SLOTS)
    x = (torch.randint(-128, 129, (B, V), generator=g).float() / 8).to(torch.bfloat16)
    x[0, V // 2] = float("-inf")
    rep = torch.tensor([2.0, 1.0, 0.5, 4.0, 4.0])
    freq = torch.randint(-32, 33, (B,), generator=g).float() / 16
    pres = torch.randint(-32, 33, (B,), generator=g).float() / 16
    return x, rep, freq, pres


def _apply_gpu(st, x, rep, freq, pres, slots=SLOTS):
    d = _to(st, "cuda")
    d.out = torch.full_like(d.out, 0).view(torch.int32).fill_(NAN_BITS).view(torch.float32)
    xd = x.cuda()
    before = xd.clone()
    got = penalties.apply(d, xd, torch.tensor(slots, dtype=torch.int32).cuda(), rep.cuda(), freq.cuda(), pres.cuda())
    torch.cuda.synchronize()
    assert got.data_ptr() == d.out.data_ptr()
    assert torch.equal(xd.view(torch.int16), before.view(torch.int16))    # the logits are never written
    return d.out.cpu()


def _check_sentinels(got, V, slots=SLOTS):
    bits = got.view(torch.int32)
    for s in range(N_SLOTS):
        if s not in slots:
            assert bool((bits[s] == NAN_BITS).all()), f"unused slot {s} was written"
    # the padding of a used row (stride > V) is untouched too
    assert bool((bits[:, V:] == NAN_BITS).all())


@pytest.mark.parametrize("V", [8, 8 * 1024 + 8, 128256])
def test_apply_exact(V):
    st = _state(V, seed=V)
    assert st.stride == V  # all three are multiples of 8; the stride != V case is below
    x, rep, freq, pres = _exact_inputs(V, seed=V + 1)
    slots = torch.tensor(SLOTS, dtype=torch.int32)
    want = st.out.view(torch.int32).fill_(NAN_BITS).view(torch.float32).clone()
    st.out = want
    ref.penalty_apply(x, st.counts, slots, rep, freq, pres, st.bias_ids, st.bias_vals, st.bias_n, want)
    w64 = ref.penalty_apply(x, st.counts, slots, rep, freq, pres, st.bias_ids, st.bias_vals, st.bias_n,
                            dtype=np.float64)
    for s in (3, 0, 7):  # exactness of the case itself: fp32 with one rounding per operation == float64
        assert np.array_equal(want[s, :V].double().numpy(), w64[s])
    got = _apply_gpu(st, x, rep, freq, pres)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    _check_sentinels(got, V)
    assert float(got[3, V // 2]) == float("-inf")


def test_apply_stride_differs_from_v_and_fp32_logits():
    V, Vs = 8 * 1024 + 8, 8 * 1024 + 24
    st = _state(V, seed=5)
    # widen the rows: count-row and output stride != V
    wide = penalties.PenaltyState(N_SLOTS, V, "cpu")
    wide.stride = Vs
    wide.counts = torch.zeros((N_SLOTS, Vs), dtype=torch.int16)
    wide.counts[:, :V] = st.counts
    wide.counts[:, V:] = -1                      # garbage past V must not matter
    wide.out = torch.zeros((N_SLOTS, Vs))
    wide.bias_ids, wide.bias_vals, wide.bias_n = st.bias_ids, st.bias_vals, st.bias_n
    x, rep, freq, pres = _exact_inputs(V, seed=6)
    xs = torch.zeros((len(SLOTS), V + 40), dtype=torch.float32)   # fp32 logits with a row stride of their own
    xs[:, :V] = x.float()
    slots = torch.tensor(SLOTS, dtype=torch.int32)
    want = torch.zeros((N_SLOTS, Vs)).view(torch.int32).fill_(NAN_BITS).view(torch.float32)
    ref.penalty_apply(xs[:, :V], wide.counts, slots, rep, freq, pres, wide.bias_ids, wide.bias_vals, wide.bias_n, want)
    d = _to(wide, "cuda")
    d.out = d.out.view(torch.int32).fill_(NAN_BITS).view(torch.float32)
    xd = xs.cuda()[:, :V]
    assert xd.stride(0) == V + 40
    penalties.apply(d, xd, slots.cuda(), rep.cuda(), freq.cuda(), pres.cuda())
    torch.cuda.synchronize()
    got = d.out.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    _check_sentinels(got, V)


def test_apply_realistic_values_within_four_roundings():
    V = 128256
    st = _state(V, seed=9, exact=False)
    g = torch.Generator().manual_seed(10)
    B = len(SLOTS)
    x = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    rep, freq, pres = torch.full((B,), 1.3), torch.full((B,), 0.37), torch.full((B,), 0.11)
    slots = torch.tensor(SLOTS, dtype=torch.int32)
    w64 = ref.penalty_apply(x, st.counts, slots, rep, freq, pres, st.bias_ids, st.bias_vals, st.bias_n,
                            dtype=np.float64)
    got = _apply_gpu(st, x, rep, freq, pres)
    c = st.counts.numpy().view(np.uint16)
    r, f, p = float(rep[0]), float(freq[0]), float(pres[0])
    for row, s in enumerate(SLOTS):
        if s < 0:
            continue
        b = np.zeros(V)
        nb = int(st.bias_n[s])
        b[st.bias_ids[s, :nb].numpy()] = np.abs(st.bias_vals[s, :nb].double().numpy())
        cnt = (c[s, :V] & 0x7FFF).astype(np.float64)
        bound = 4 * 2.0 ** -24 * (np.abs(x[row].double().numpy()) * max(r, 1 / r) + abs(f) * cnt + abs(p) + b)
        err = np.abs(got[s, :V].double().numpy() - w64[s])
        assert np.all(err <= bound), (s, float(err.max()))
    _check_sentinels(got, V)


def test_update_counts_saturates_and_ignores_bad_rows():
    V = 1000
    st = _state(V, seed=2)
    assert st.stride == V
    c = st.counts.numpy().view(np.uint16)
    c[2, 17], c[4, 0], c[5, V - 1], c[6, 9] = 0x7FFF, 0xFFFF, 0x8000, 0
    slots = torch.tensor([2, 4, 5, 6, -1, 8, 1000, 1, 0, 3], dtype=torch.int32)
    toks = torch.tensor([17, 0, V - 1, 9, 5, 5, 5, V, -1, 44], dtype=torch.int32)
    d = _to(st, "cuda")
    penalties.update(d, slots.cuda(), toks.cuda(), len(slots))
    torch.cuda.synchronize()
    want = st.counts.clone()
    ref.penalty_update(want, slots, toks, V)
    w = want.numpy().view(np.uint16)
    assert w[2, 17] == 0x7FFF and w[4, 0] == 0xFFFF and w[5, V - 1] == 0x8001 and w[6, 9] == 1
    assert torch.equal(d.counts.cpu(), want)
    # only bad rows: the whole table is unchanged
    d2 = _to(st, "cuda")
    penalties.update(d2, torch.tensor([-1, 8, 1 << 20, 1, 0], dtype=torch.int32).cuda(),
                     torch.tensor([3, 3, 3, V, -7], dtype=torch.int32).cuda(), 5)
    torch.cuda.synchronize()
    assert torch.equal(d2.counts.cpu(), st.counts)


def _bits(vals):
    return np.asarray(vals, dtype=np.float32).view(np.int32).tolist()


def test_seed_duplicates_entries_append_and_clear():
    V = 8 * 1024 + 8
    st = penalties.PenaltyState(N_SLOTS, V, "cpu")
    st.counts.fill_(0x0101)          # stale history everywhere: clear = 1 must wipe it
    st.bias_n.fill_(9)
    st.bias_ids.fill_(1)
    st.bias_vals.fill_(1.0)
    d = _to(st, "cuda")
    # launch 1: two entries.  slot 5: the same id 1,000 times plus neighbours sharing its 32-bit
    # word; slot 2: prompt and output overlap, edges, out-of-range ids, a bias list.
    ids5 = [40, 41, 40, 0, V - 1] + [40] * 1000 + [41] * 3 + [V - 1]
    e5 = [5, 0, 5, 1004, 0, 1]
    p2, o2, b2 = [7, 7, 8, V, -1, V - 1], [8, 8, 9, V + 5, 0], [(0, 1.5), (V - 1, -100.0), (33, 0.25)]
    ids2 = p2 + o2 + [t for t, _ in b2] + _bits([b for _, b in b2])
    e2 = [2, len(ids5), len(p2), len(o2), len(b2), 1]
    bad = [N_SLOTS, 0, 3, 3, 0, 1, 1, 0, 1 << 20, 0, 0, 1]   # slot out of range; entry past the stream
    ids = torch.tensor(ids5 + ids2, dtype=torch.int32)
    entries = torch.tensor(e5 + e2 + bad, dtype=torch.int32)
    penalties.seed(d, entries.cuda(), 4, ids.cuda(), len(ids))
    penalties.seed(st, entries, 4, ids, len(ids))
    # launch 2: clear = 0 appends to slot 2 (counts, flags and bias); clear = 1 wipes slot 5's bias
    ids_b = [9, 100] + [8, 101] + [50] + _bits([2.0]) + [3] + [4, 4]
    entries_b = torch.tensor([2, 0, 2, 2, 1, 0, 5, 6, 1, 2, 0, 1], dtype=torch.int32)
    ids_b = torch.tensor(ids_b, dtype=torch.int32)
    penalties.seed(d, entries_b.cuda(), 2, ids_b.cuda(), len(ids_b))
    penalties.seed(st, entries_b, 2, ids_b, len(ids_b))
    torch.cuda.synchronize()
    got = _to(d, "cpu")
    flags2, counts2 = penalties.read_slot(got, 2)
    assert flags2 == {7, 8, V - 1, 9, 100} and counts2 == {8: 3, 9: 1, 0: 1, 101: 1}
    assert int(got.bias_n[2]) == 4 and got.bias_ids[2, :4].tolist() == [0, V - 1, 33, 50]
    assert got.bias_vals[2, :4].tolist() == [1.5, -100.0, 0.25, 2.0]
    assert penalties.read_slot(got, 5) == ({3}, {4: 2}) and int(got.bias_n[5]) == 0
    # everything, including the untouched slots, equals the reference
    for k in ("counts", "bias_n"):
        assert torch.equal(getattr(got, k), getattr(st, k)), k
    for s in range(N_SLOTS):
        n = int(st.bias_n[s]) if s in (2, 5) else 9
        assert torch.equal(got.bias_ids[s, :n], st.bias_ids[s, :n])
        assert torch.equal(got.bias_vals[s, :n], st.bias_vals[s, :n])


def test_seed_counts_a_thousand_duplicates():
    V = 128256
    d = _to(penalties.PenaltyState(2, V, "cpu"), "cuda")
    ids = torch.tensor([V - 2] * 1000 + [V - 1] * 1000, dtype=torch.int32).cuda()
    penalties.seed(d, torch.tensor([1, 0, 0, 2000, 0, 1], dtype=torch.int32).cuda(), 1, ids, 2000)
    torch.cuda.synchronize()
    assert penalties.read_slot(d, 1) == (set(), {V - 2: 1000, V - 1: 1000})
    assert penalties.read_slot(d, 0) == (set(), {})


# ---------------------------------------------------------------------------- pk_sample_alt
def _sample_params(B, greedy):
    if greedy:
        return (torch.zeros(B), torch.zeros(B, dtype=torch.int32), torch.ones(B), torch.zeros(B),
                torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32))
    return (torch.full((B,), 0.8), torch.full((B,), 50, dtype=torch.int32), torch.full((B,), 0.9), torch.zeros(B),
            torch.arange(B, dtype=torch.int32) + 11, torch.arange(B, dtype=torch.int32) * 3)


@pytest.mark.parametrize("greedy", [True, False])
def test_sample_alt_reads_alt_rows_as_fp32_and_the_rest_as_before(greedy):
    B, V, Vs = 6, 8 * 1024 + 8, 8 * 1024 + 16
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16).cuda()
    alt = (torch.randn(N_SLOTS, Vs, generator=g) * 3).cuda()          # fp32, unrelated to x
    slots = torch.tensor([4, -1, 0, -1, N_SLOTS, 7], dtype=torch.int32)   # N_SLOTS: out of range = no alt
    prm = [t.cuda() for t in _sample_params(B, greedy)]
    base = sampler.sample(x, *prm)
    none = sampler.sample(x, *prm, alt=alt, alt_slots=torch.full((B,), -1, dtype=torch.int32).cuda())
    got = sampler.sample(x, *prm, alt=alt, alt_slots=slots.cuda())
    rows = [b for b in range(B) if 0 <= int(slots[b]) < N_SLOTS]
    gathered = alt[slots[rows].long().cuda(), :V].contiguous()
    sub = [t[rows].contiguous() for t in prm]
    want_alt = sampler.sample(gathered, *sub)                               # pk_sample on fp32 rows
    torch.cuda.synchronize()
    assert torch.equal(none, base)
    for b in range(B):
        if b not in rows:
            assert int(got[b]) == int(base[b])
    assert [int(got[b]) for b in rows] == want_alt.tolist()
    assert [int(got[b]) for b in rows] != [int(base[b]) for b in rows]      # the alt rows really differ
