"""Logprobs kernel (csrc/kernels/logprobs.hip) against the float64 reference.

Tolerance: logprobs to atol 1e-4 (no rtol), ids exactly.  fp32 log_softmax differs from float64
by <= 5.6e-6 on these inputs (bf16 randn x 3 at V = 128,256, checked on the CPU), so 1e-4 leaves
about 18x for the kernel's fast exp / log.  bf16 randn at V = 128,256 has only ~2,800 distinct
values, so ties inside the top 20 occur naturally and the exact-id check tests the tie rule
(value descending, id ascending).
"""
import pytest
import torch

from polykey_service_amd.ops import reference as ref
from polykey_service_amd.ops import sampler

pytestmark = pytest.mark.gpu

ATOL = 1e-4
NMAX = sampler.LOGPROB_NMAX
SENTINEL = 0x5A5A5A5A
N_MIX = (-1, 0, 1, 5, 20)


def _inputs(B, V, dtype, stride=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, stride or V, generator=g) * 3).to(dtype)
    n_top = torch.tensor([N_MIX[b % len(N_MIX)] for b in range(B)], dtype=torch.int32)
    tokens = torch.randint(0, V, (B,), generator=g, dtype=torch.int32)
    tokens[1] = V - 1                                             # the last column
    tokens[4] = int(torch.argmax(x[4, :V].float()))               # an id inside the top set (row 4: n = 20)
    tokens[3] = int(torch.topk(x[3, :V].float(), 3).indices[2])   # row 3: n = 5
    return x, tokens, n_top


def _run(x, V, tokens, n_top):
    B = x.shape[0]
    xd = x.cuda()[:, :V]
    out = torch.full((B, sampler.LOGPROB_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    got = sampler.logprobs(xd, tokens.cuda(), n_top.cuda(), out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu()


def _check(got, x, V, tokens, n_top):
    B = x.shape[0]
    want = ref.logprobs(x[:, :V], tokens, n_top, torch.full((B, sampler.LOGPROB_WORDS), SENTINEL, dtype=torch.int32))
    glp, gid, gtop = sampler.unpack_logprobs(got)
    wlp, wid, wtop = sampler.unpack_logprobs(want)
    for b in range(B):
        n = int(n_top[b])
        if n < 0:  # not requested: nothing written
            assert torch.equal(got[b], torch.full_like(got[b], SENTINEL)), b
            continue
        assert torch.equal(gid[b], wid[b]), (b, n, gid[b].tolist(), wid[b].tolist())
        n = min(n, V)
        assert gid[b, n:].eq(-1).all() and torch.isneginf(gtop[b, n:]).all(), b
        assert not torch.isnan(glp[b]) and not torch.isnan(gtop[b]).any(), b
        for g, w in ((glp[b:b + 1], wlp[b:b + 1]), (gtop[b, :n], wtop[b, :n])):
            fin = torch.isfinite(w)
            assert torch.equal(torch.isfinite(g), fin), b
            assert torch.equal(g[~fin], w[~fin]), b
            err = (g[fin].double() - w[fin].double()).abs().max().item() if fin.any() else 0.0
            assert err <= ATOL, (b, n, err)


@pytest.mark.parametrize("B,V,dtype,stride", [
    (16, 128256, torch.bfloat16, None),
    (8, 32000, torch.float32, None),
    (16, 4096 + 8, torch.bfloat16, None),
    (16, 40, torch.bfloat16, None),           # fewer than one vector per thread; n = 20 of 40
    (16, 4096 + 8, torch.bfloat16, 4096 + 8 + 64),  # logits = a column slice of a wider buffer
])
def test_matches_reference(B, V, dtype, stride):
    x, tokens, n_top = _inputs(B, V, dtype, stride)
    _check(_run(x, V, tokens, n_top), x, V, tokens, n_top)


@pytest.mark.parametrize("V,dtype", [(128256, torch.bfloat16), (4096 + 8, torch.float32), (40, torch.bfloat16)])
def test_constructed_ties_and_infinities(V, dtype):
    ninf = float("-inf")
    B = 8
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B, V, generator=g) * 3).to(dtype)
    x[0, :] = 1.5                                    # all equal: ids 0..n-1
    x[1, :] = -2.0
    for i in (3, V // 2, V - 1):                     # one maximum at three places: in id order
        x[1, i] = 7.0
    x[2, ::3] = ninf                                 # some -inf entries
    x[3, :] = ninf                                   # all -inf: -inf everywhere, no NaN
    x[4, :] = ninf
    x[4, V - 1] = 0.25                               # one finite entry, n = 20: -inf tail in id order
    x[5, :] = 0.0
    x[5, 1::2] = -0.0                                # signed zeros compare equal
    x[6, :] = 3.0
    x[6, 5] = 4.0                                    # ties below the maximum: 5, then 0..n-2
    n_top = torch.tensor([20, 5, 20, 20, 20, 5, 20, 1], dtype=torch.int32)
    tokens = torch.tensor([V - 1, V // 2, 0, 7, V - 1, 1, 0, 2], dtype=torch.int32)
    got = _run(x, V, tokens, n_top)
    _check(got, x, V, tokens, n_top)
    lp, ids, top = sampler.unpack_logprobs(got)
    assert ids[0].tolist() == list(range(20))
    assert ids[1, :5].tolist() == [3, V // 2, V - 1, 0, 1]
    assert ids[3].tolist() == list(range(20)) and torch.isneginf(top[3]).all() and torch.isneginf(lp[3])
    assert ids[4, :3].tolist() == [V - 1, 0, 1] and abs(float(top[4, 0])) <= ATOL and torch.isneginf(top[4, 1:]).all()
    assert ids[5, :5].tolist() == [0, 1, 2, 3, 4]
    assert ids[6].tolist() == [5] + list(range(5)) + list(range(6, 20))
    assert torch.isneginf(lp[2]) and abs(float(lp[4])) <= ATOL  # token 0 of row 2 is -inf; row 4's only token has p = 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_tie_pool_threshold(dtype):
    """The kernel settles ties in a 128-entry pool (the elements >= the n-th value) and walks the
    ids first when more would be gathered: 10 values above the tie level plus 117 / 118 / 119 /
    400 ties give pools of 127 / 128 (pool path) and 129 / 410 (id walk); n = 20 needs the 10
    lowest tied ids, n = 5 none of them."""
    V = 4096 + 8
    tie_counts = (117, 118, 119, 400)
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(2 * len(tie_counts), V, generator=g) - 6.0).clamp(max=-1.0).to(dtype)
    for r, t in enumerate(tie_counts):
        perm = torch.randperm(V, generator=g)
        for row in (2 * r, 2 * r + 1):
            x[row, perm[:10]] = torch.arange(11.0, 21.0).to(dtype)
            x[row, perm[10:10 + t]] = 5.0
    n_top = torch.tensor([20, 5] * len(tie_counts), dtype=torch.int32)
    tokens = torch.randint(0, V, (x.shape[0],), generator=g, dtype=torch.int32)
    _check(_run(x, V, tokens, n_top), x, V, tokens, n_top)


def test_graph_replay_equals_eager():
    B, V = 16, 4096 + 8
    x, tokens, n_top = _inputs(B, V, torch.bfloat16, seed=2)
    xd, td, nd = x.cuda(), tokens.cuda(), n_top.cuda()
    out = torch.full((B, sampler.LOGPROB_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sampler.logprobs(xd, td, nd, out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sampler.logprobs(xd, td, nd, out)
    # new step, same buffers: other logits, ids and list lengths
    x2, tokens2, n2 = _inputs(B, V, torch.bfloat16, seed=3)
    n2 = n2.roll(2)
    xd.copy_(x2)
    td.copy_(tokens2)
    nd.copy_(n2)
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.cpu()
    eager = _run(x2, V, tokens2, n2)
    assert torch.equal(replayed, eager)
    _check(replayed, x2, V, tokens2, n2)
