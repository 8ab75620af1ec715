"""QK-norm fused into the RoPE / KV-write kernels (Qwen3), against a float64 reference of the contract.

Contract (csrc/kernels/rope_cache.hip, gemm_skinny.hip), x the bf16 QKV projection output, per q / k head
of 128 values:

    y_i = x_i * rsqrt(sum_j x_j^2 / 128 + eps) * w_i          fp32
    out = bf16(RoPE_neox(y))                                  fp32 rotation, ONE rounding

v is untouched; the K cache receives ``out`` (an FP8 cache its e4m3 byte); padding rows (slot < 0) are
normalised and rotated but not cached.

Error bound on random inputs, for an output element r = y_a cos - y_b sin (or y_b cos + y_a sin):

    |out - ref| <= 2^-8 |ref| + 2^-16 (|y_a| + |y_b|)

The first term is the one bf16 rounding (half an ulp of an 8-bit significand is at most 2^-8 of the
value).  The second covers the fp32 arithmetic before it: rsqrt (1 ulp = 2^-23), the sum of squares
(128 terms, relative error well under 128 * 2^-24 = 2^-17, halved by the square root), two
multiplications for y (2^-24 each), and the rotation's products and sum (3 * 2^-24 of |y_a| + |y_b|,
cos and sin being at most 1) -- under 2^-17 (|y_a| + |y_b|) in total, so 2^-16 leaves a factor of two.

Grid inputs (multiples of 2^-3, |x| <= 4) make every slab sum and every sum of squares exact in fp32
in any order: there the slab kernel and ``rope_and_cache`` on the bf16 sum agree bit for bit.
"""
import pytest
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
I32 = torch.int32
EPS = 1e-6
MAX_POS = 512
HEADS = [(4, 1, 32), (16, 4, 64), (8, 8, 32)]  # nq, nkv, block size
TOKENS = [1, 31, 32, 33, 70]                    # around the kernel's 32-token tile
K_SCALE, V_SCALE = 0.5, 2.0


def cos_sin():
    return reference.rope_cos_sin_cache(MAX_POS, 128, 1e6)


def norm_weights(seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return [(0.5 + torch.rand(128, generator=g)).to(BF16) for _ in range(2)]


def make_slots(T, bs, kind, seed):
    """-> (slots [T] int32, number of blocks).  ``aligned``: the first 32 tokens fill one aligned
    32-slot run (the gathered V path) when there are that many, the rest follow on; ``scattered``: a
    random injective map with every fifth token a padding row (slot -1)."""
    g = torch.Generator().manual_seed(seed)
    nb = (T + bs - 1) // bs + 2
    if kind == "aligned":
        slots = (bs + torch.arange(T)).to(I32)  # block 0 stays untouched
    else:
        slots = torch.randperm(nb * bs, generator=g)[:T].to(I32)
        slots[torch.arange(T) % 5 == 3] = -1
    assert int(slots.max()) < nb * bs
    return slots, nb


def caches(nb, nkv, bs, fp8):
    """Pre-filled with NaN (bf16 0x7fc0 / e4m3 0x7f)."""
    if fp8:
        k = torch.full((nb, nkv, bs, 128), 0x7F, dtype=torch.uint8, device=DEV).view(A.FP8)
        v = torch.full((nb, nkv, 128, bs), 0x7F, dtype=torch.uint8, device=DEV).view(A.FP8)
    else:
        k = torch.full((nb, nkv, bs, 128), float("nan"), dtype=BF16, device=DEV)
        v = torch.full((nb, nkv, 128, bs), float("nan"), dtype=BF16, device=DEV)
    return k, v


def ref_qk(x, pos, cs, qw, kw, nq, nkv, eps=EPS):
    """float64 contract on x [T, nq + 2 nkv, 128] (bf16 values) -> (ref, slack), both [T, nq + nkv, 128]:
    the unrounded rotated heads and |y_a| + |y_b| of every element."""
    xd = x[:, :nq + nkv].double()
    w = torch.cat([qw.double().expand(nq, 128), kw.double().expand(nkv, 128)])
    y = xd * torch.rsqrt(xd.pow(2).sum(-1, keepdim=True) / 128 + eps) * w
    c = cs[pos.long()].double()
    co, si = c[:, None, :64], c[:, None, 64:]
    ya, yb = y[..., :64], y[..., 64:]
    ref = torch.cat([ya * co - yb * si, yb * co + ya * si], -1)
    slack = (ya.abs() + yb.abs()).repeat(1, 1, 2)
    return ref, slack


def within(got, ref, slack):
    return (got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -16 * slack


def logical(kc, vc):
    """Caches as [nb, nkv, bs, 128] (token, dim) rows on the CPU; FP8 as raw bytes."""
    if kc.dtype == A.FP8:
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
    return reference.k_cache_logical(kc).cpu(), reference.v_cache_logical(vc).cpu()


def check_caches(kc, vc, slots, k_rows, v_rows, bs, tag):
    """Addressed slots hold ``k_rows`` / ``v_rows`` [T, nkv, 128] bit for bit; every other element is
    still the NaN it was filled with."""
    fp8 = kc.dtype == A.FP8
    kl, vl = logical(kc, vc)
    nb, nkv = kl.shape[:2]
    nan_k = torch.full_like(kl, 0x7F) if fp8 else torch.full_like(kl, float("nan"))
    want_k, want_v = nan_k.clone(), nan_k.clone()
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            want_k[s // bs, :, s % bs] = k_rows[t]
            want_v[s // bs, :, s % bs] = v_rows[t]
    bits = (lambda a: a) if fp8 else (lambda a: a.view(torch.int16))
    assert torch.equal(bits(kl), bits(want_k)), tag
    assert torch.equal(bits(vl), bits(want_v)), tag


def run_rope(x, pos, cs, slots, nq, nkv, bs, nb, fp8, qw, kw, eps=EPS):
    """-> (qkv after the kernel [T, nh, 128] on the CPU, k cache, v cache); the buffer's row stride is
    wider than the row and its padding must stay NaN."""
    T, N = x.shape[0], (nq + 2 * nkv) * 128
    buf = torch.full((T, N + 128), float("nan"), dtype=BF16, device=DEV)
    buf[:, :N].copy_(x.reshape(T, N))
    kc, vc = caches(nb, nkv, bs, fp8)
    A.rope_and_cache(buf[:, :N], pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), nq, nkv, k_scale=K_SCALE,
                     v_scale=V_SCALE, q_norm=qw.to(DEV), k_norm=kw.to(DEV), eps=eps)
    torch.cuda.synchronize()
    assert bool(buf[:, N:].isnan().all())
    return buf[:, :N].cpu().view(T, nq + 2 * nkv, 128), kc, vc


def random_qkv(T, nh, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, nh, 128, generator=g).to(BF16)
    x[T // 2] = (x[T // 2].float() * 2.0 ** -10).to(BF16)  # mean square ~ 1e-6: eps decides this row
    return x


def expected_cache_rows(out, x, nq, nkv, fp8):
    k, v = out[:, nq:nq + nkv], x[:, nq + nkv:]
    if fp8:  # the e4m3 byte of the bf16 value the kernel left in the buffer / of the untouched v
        return (reference.quantize_fp8(k, K_SCALE).view(torch.uint8), reference.quantize_fp8(v, V_SCALE).view(torch.uint8))
    return k, v


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("nq,nkv,bs", HEADS)
@pytest.mark.parametrize("T", TOKENS)
def test_rope_and_cache_qknorm(T, nq, nkv, bs, fp8):
    cs = cos_sin()
    qw, kw = norm_weights()
    nh = nq + 2 * nkv
    for kind in ("aligned", "scattered"):
        x = random_qkv(T, nh, seed=T * 7 + nq)
        pos = torch.randint(0, MAX_POS, (T,), generator=torch.Generator().manual_seed(T)).to(I32)
        slots, nb = make_slots(T, bs, kind, seed=T + nkv)
        out, kc, vc = run_rope(x, pos, cs, slots, nq, nkv, bs, nb, fp8, qw, kw)
        ref, slack = ref_qk(x, pos, cs, qw, kw, nq, nkv)
        ok = within(out[:, :nq + nkv], ref, slack)
        assert bool(ok.all()), (kind, int((~ok).sum()))
        # eps matters on the small row: the same check against eps = 1e-5 must fail there
        ref5, slack5 = ref_qk(x, pos, cs, qw, kw, nq, nkv, eps=1e-5)
        assert not bool(within(out[T // 2, :nq + nkv], ref5[T // 2], slack5[T // 2]).all())
        # v in the buffer is untouched, bit for bit
        assert torch.equal(out[:, nq + nkv:].view(torch.int16), x[:, nq + nkv:].view(torch.int16))
        check_caches(kc, vc, slots, *expected_cache_rows(out, x, nq, nkv, fp8), bs, (kind, T))


def test_eps_argument_is_used():
    """The kernel with eps = 1e-5 meets the eps = 1e-5 reference and misses the 1e-6 one."""
    T, (nq, nkv, bs) = 33, HEADS[1]
    cs = cos_sin()
    qw, kw = norm_weights(1)
    x = random_qkv(T, nq + 2 * nkv, seed=5)
    pos = torch.arange(T, dtype=I32)
    slots, nb = make_slots(T, bs, "scattered", 3)
    out, _, _ = run_rope(x, pos, cs, slots, nq, nkv, bs, nb, False, qw, kw, eps=1e-5)
    ref5, s5 = ref_qk(x, pos, cs, qw, kw, nq, nkv, eps=1e-5)
    ref6, s6 = ref_qk(x, pos, cs, qw, kw, nq, nkv, eps=1e-6)
    assert bool(within(out[:, :nq + nkv], ref5, s5).all())
    assert not bool(within(out[T // 2, :nq + nkv], ref6[T // 2], s6[T // 2]).all())


def test_norm_weights_are_used_per_family():
    """q heads take q_norm, k heads k_norm: swapping them misses the bound."""
    T, (nq, nkv, bs) = 5, HEADS[1]
    cs = cos_sin()
    qw, kw = norm_weights(2)
    x = random_qkv(T, nq + 2 * nkv, seed=9)
    pos = torch.arange(T, dtype=I32)
    slots, nb = make_slots(T, bs, "aligned", 0)
    out, _, _ = run_rope(x, pos, cs, slots, nq, nkv, bs, nb, False, qw, kw)
    ref, s = ref_qk(x, pos, cs, kw, qw, nq, nkv)
    assert not bool(within(out[:, :nq], ref[:, :nq], s[:, :nq]).all())
    assert not bool(within(out[:, nq:nq + nkv], ref[:, nq:], s[:, nq:]).all())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_needle_changes_its_head_only(fp8):
    T, (nq, nkv, bs) = 33, HEADS[1]
    cs = cos_sin()
    qw, kw = norm_weights(3)
    x = random_qkv(T, nq + 2 * nkv, seed=21)
    pos = torch.arange(T, dtype=I32)
    slots, nb = make_slots(T, bs, "aligned", 0)
    base, kc0, vc0 = run_rope(x, pos, cs, slots, nq, nkv, bs, nb, fp8, qw, kw)
    for t, h, d in ((7, 3, 5), (32, nq + 2, 100)):  # a q head, a k head (second token tile)
        y = x.clone()
        y[t, h, d] = (y[t, h, d].float() * 2.0 ** 10 + 2.0 ** 10).to(BF16)
        got, kc, vc = run_rope(y, pos, cs, slots, nq, nkv, bs, nb, fp8, qw, kw)
        same = (got.view(torch.int16) == base.view(torch.int16)).all(-1)  # [T, nh]
        assert not bool(same[t, h]) and int((~same).sum()) == 1
        # the needle dominates its head's mean square: every other element of the head shrinks
        assert float(got[t, h].float().abs().sum()) != float(base[t, h].float().abs().sum())
        k0, v0 = logical(kc0, vc0)
        k1, v1 = logical(kc, vc)
        bits = (lambda a: a) if fp8 else (lambda a: a.view(torch.int16))
        diff = (bits(k0) != bits(k1)).any(-1)  # [nb, nkv, bs]
        assert int(diff.sum()) == (1 if h >= nq else 0)
        if h >= nq:
            s = int(slots[t])
            assert bool(diff[s // bs, h - nq, s % bs])
        assert torch.equal(bits(v0), bits(v1))


# --------------------------------------------------------------------------------- slab kernel
def dev_partial(slabs):
    S, M, N = slabs.shape
    buf = torch.full((slabs.numel() + 256,), float("nan"), dtype=torch.float32, device=DEV)
    buf[: slabs.numel()] = slabs.reshape(-1).to(DEV)
    return gemm.Partial(buf, S, M, N)


def slab_sum_bf16(slabs):
    """The kernel's slab sum: fp32, slab 0 first, then rounded to bf16 (the unfused GEMM output)."""
    acc = slabs[0].clone()
    for s in range(1, slabs.shape[0]):
        acc = acc + slabs[s]
    return acc.to(BF16)


def run_slab(slabs, pos, cs, slots, nq, nkv, bs, nb, qw, kw):
    kc, vc = caches(nb, nkv, bs, False)
    q = gemm.qkv_reduce_rope_cache(dev_partial(slabs), pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), nq, nkv,
                                   q_norm=qw.to(DEV), k_norm=kw.to(DEV), eps=EPS)
    torch.cuda.synchronize()
    return q.cpu(), kc, vc


@pytest.mark.parametrize("S", [1, 2, 4, 8])
@pytest.mark.parametrize("nq,nkv,bs", HEADS)
def test_qkv_reduce_rope_cache_qknorm_random(nq, nkv, bs, S):
    cs = cos_sin()
    qw, kw = norm_weights(4)
    nh = nq + 2 * nkv
    for M, kind in ((1, "aligned"), (33, "scattered"), (70, "aligned")):
        g = torch.Generator().manual_seed(S * 100 + M)
        slabs = torch.randn(S, M, nh * 128, generator=g) / S ** 0.5
        slabs[:, M // 2] *= 2.0 ** -10
        x = slab_sum_bf16(slabs).view(M, nh, 128)
        pos = torch.randint(0, MAX_POS, (M,), generator=g).to(I32)
        slots, nb = make_slots(M, bs, kind, seed=M + S)
        q, kc, vc = run_slab(slabs, pos, cs, slots, nq, nkv, bs, nb, qw, kw)
        ref, slack = ref_qk(x, pos, cs, qw, kw, nq, nkv)
        assert bool(within(q, ref[:, :nq], slack[:, :nq]).all()), (M, kind)
        ref5, slack5 = ref_qk(x, pos, cs, qw, kw, nq, nkv, eps=1e-5)
        assert not bool(within(q[M // 2], ref5[M // 2, :nq], slack5[M // 2, :nq]).all())
        # K rows: within the bound of the reference where cached; V rows: the bf16 slab sum, bit for bit
        kl, vl = logical(kc, vc)
        for t, s in enumerate(slots.tolist()):
            if s >= 0:
                assert bool(within(kl[s // bs, :, s % bs], ref[t, nq:], slack[t, nq:]).all()), (M, t)
        want_k = torch.stack([kl[max(s, 0) // bs, :, max(s, 0) % bs] for s in slots.tolist()])
        check_caches(kc, vc, slots, want_k, x[:, nq + nkv:], bs, (M, kind))  # nothing else was written


@pytest.mark.parametrize("S", [1, 2, 4, 8])
@pytest.mark.parametrize("nq,nkv,bs", HEADS)
def test_slab_kernel_equals_rope_and_cache_on_the_grid(nq, nkv, bs, S):
    """Multiples of 2^-3 with |sum| <= 4: slab sums (multiples of 2^-3 below 2^3) and sums of squares
    (multiples of 2^-6 below 2^11: 17 bits) are exact in fp32 in any order, so both kernels normalise
    with the same bits and must agree on q, the K tile and V bit for bit."""
    cs = cos_sin()
    qw, kw = norm_weights(5)
    nh = nq + 2 * nkv
    for M, kind in ((31, "scattered"), (70, "aligned")):
        g = torch.Generator().manual_seed(S + M)
        lim = 32 // S  # per-slab |value| <= lim / 8, so |sum| <= 4
        slabs = torch.randint(-lim, lim + 1, (S, M, nh * 128), generator=g).float() / 8
        x = slab_sum_bf16(slabs).view(M, nh, 128)
        assert torch.equal(x.double(), slabs.double().sum(0).view(M, nh, 128)) and float(x.float().abs().max()) <= 4
        pos = torch.randint(0, MAX_POS, (M,), generator=g).to(I32)
        slots, nb = make_slots(M, bs, kind, seed=M)
        q, kc, vc = run_slab(slabs, pos, cs, slots, nq, nkv, bs, nb, qw, kw)
        out, kc2, vc2 = run_rope(x, pos, cs, slots, nq, nkv, bs, nb, False, qw, kw)
        assert torch.equal(q.view(torch.int16), out[:, :nq].contiguous().view(torch.int16)), (M, kind)
        (k1, v1), (k2, v2) = logical(kc, vc), logical(kc2, vc2)
        assert torch.equal(k1.view(torch.int16), k2.view(torch.int16)), (M, kind)
        assert torch.equal(v1.view(torch.int16), v2.view(torch.int16)), (M, kind)
        ref, slack = ref_qk(x, pos, cs, qw, kw, nq, nkv)
        assert bool(within(q, ref[:, :nq], slack[:, :nq]).all())


def test_graph_capture_and_replay_with_rewritten_positions_and_slots():
    T, (nq, nkv, bs), S = 33, HEADS[1], 4
    nh, N = nq + 2 * nkv, (nq + 2 * nkv) * 128
    cs = cos_sin().to(DEV)
    qw, kw = (w.to(DEV) for w in norm_weights(6))
    nb = 5
    g = torch.Generator().manual_seed(1)
    slabs = torch.randn(S, T, N, generator=g) / 2
    p = dev_partial(slabs)
    x = slab_sum_bf16(slabs).view(T, nh, 128)
    src = x.reshape(T, N).to(DEV)
    qkv = torch.empty_like(src)
    pos = torch.zeros(T, dtype=I32, device=DEV)
    slots = torch.full((T,), -1, dtype=I32, device=DEV)
    kc, vc = caches(nb, nkv, bs, False)
    kc2, vc2 = caches(nb, nkv, bs, True)
    kc3, vc3 = caches(nb, nkv, bs, False)
    res = {}

    def step():
        qkv.copy_(src)
        A.rope_and_cache(qkv, pos, cs, kc, vc, slots, nq, nkv, q_norm=qw, k_norm=kw, eps=EPS)
        qkv.copy_(src)
        A.rope_and_cache(qkv, pos, cs, kc2, vc2, slots, nq, nkv, k_scale=K_SCALE, v_scale=V_SCALE, q_norm=qw,
                         k_norm=kw, eps=EPS)
        res["q"] = gemm.qkv_reduce_rope_cache(p, pos, cs, kc3, vc3, slots, nq, nkv, q_norm=qw, k_norm=kw, eps=EPS)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up: every slot is -1, nothing is cached
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for rnd in range(2):
        new_pos = torch.randint(0, MAX_POS, (T,), generator=g).to(I32)
        new_slots, _ = make_slots(T, bs, "scattered" if rnd else "aligned", seed=rnd)
        assert int(new_slots.max()) < nb * bs
        for c in (kc, vc, kc3, vc3):
            c.fill_(float("nan"))
        for c in (kc2, vc2):
            c.view(torch.uint8).fill_(0x7F)
        pos.copy_(new_pos)
        slots.copy_(new_slots)
        graph.replay()
        torch.cuda.synchronize()
        ref, slack = ref_qk(x, new_pos, cs.cpu(), qw.cpu(), kw.cpu(), nq, nkv)
        out = qkv.cpu().view(T, nh, 128)
        assert bool(within(out[:, :nq + nkv], ref, slack).all()), rnd
        assert bool(within(res["q"].cpu(), ref[:, :nq], slack[:, :nq]).all()), rnd
        check_caches(kc, vc, new_slots, *expected_cache_rows(out, x, nq, nkv, False), bs, rnd)
        check_caches(kc2, vc2, new_slots, *expected_cache_rows(out, x, nq, nkv, True), bs, rnd)
        kl, _ = logical(kc3, vc3)
        for t, s in enumerate(new_slots.tolist()):
            if s >= 0:
                assert bool(within(kl[s // bs, :, s % bs], ref[t, nq:], slack[t, nq:]).all()), (rnd, t)


def test_wrappers_refuse_half_a_pair_and_wrong_weights():
    kc, vc = caches(2, 1, 32, False)
    x = torch.zeros(1, 6 * 128, dtype=BF16, device=DEV)
    z = torch.zeros(1, dtype=I32, device=DEV)
    w = torch.ones(128, dtype=BF16, device=DEV)
    with pytest.raises(ValueError):
        A.rope_and_cache(x, z, cos_sin().to(DEV), kc, vc, z, 4, 1, q_norm=w)
    with pytest.raises(ValueError):
        A.rope_and_cache(x, z, cos_sin().to(DEV), kc, vc, z, 4, 1, q_norm=w, k_norm=w.float())
    with pytest.raises(ValueError):
        A.rope_and_cache(x, z, cos_sin().to(DEV), kc, vc, z, 4, 1, q_norm=w, k_norm=torch.ones(64, dtype=BF16, device=DEV))
    # the kernel loads the weights as 16-byte vectors: a contiguous view 2 bytes into its storage is refused
    odd = torch.ones(136, dtype=BF16, device=DEV)[1:129]
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 2
    with pytest.raises(ValueError, match="16-byte"):
        A.rope_and_cache(x, z, cos_sin().to(DEV), kc, vc, z, 4, 1, q_norm=w, k_norm=odd)
    p = gemm.Partial(torch.zeros(6 * 128, device=DEV), 1, 1, 6 * 128)
    with pytest.raises(ValueError, match="16-byte"):
        gemm.qkv_reduce_rope_cache(p, z, cos_sin().to(DEV), kc, vc, z, 4, 1, q_norm=odd, k_norm=w)
