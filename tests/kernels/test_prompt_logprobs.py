"""Prompt-logprobs kernel (csrc/kernels/logprobs.hip, the kPrompt form) against an exact reference.

Ids and ranks are integers and are compared exactly (the reference below counts the rank on the
exact values in float64 / integers).  Logprobs: atol 1e-4, the tolerance tests/kernels/test_logprobs.py
derived for exactly the random input used here (bf16 randn x 3 at V = 128,256: fp32 log_softmax
is within 5.6e-6 of float64, 1e-4 leaves ~18x for the kernel's fast exp / log); constructed rows
use the same bound.  The no-tolerance anchor: the logprob word and the 40 list words are bit-identical
to what ``pk_logprobs`` writes for ``tokens = targets`` -- the two kernels are one template body.

Widths: 8 (one vector), 8184 (fewer vectors than the 1024 threads), 8192 (one per thread), 8200 (a
second vector for one thread), 128256 (the real width).  Padding columns (stride > V) are NaN, output
buffers are pre-filled with a sentinel, rows with ``targets < 0`` or ``n_top < 0`` must keep it.
"""
import pytest
import torch

from polykey_service_amd.ops import native, sampler
from tests.prompt_logprobs_cases import reference_rows

pytestmark = pytest.mark.gpu

ATOL = 1e-4  # tests/kernels/test_logprobs.py
NMAX = sampler.LOGPROB_NMAX
W = sampler.PROMPT_LOGPROB_WORDS
SENTINEL = 0x5A5A5A5A
N_MIX = (-1, 0, 1, 5, 20)
WIDTHS = (8, 8184, 8192, 8200, 128256)
NINF = float("-inf")


def run(x, V, targets, n_top):
    R = x.shape[0]
    xd = x.cuda()[:, :V]
    out = torch.full((R, W), SENTINEL, dtype=torch.int32, device="cuda")
    got = sampler.prompt_logprobs(xd, targets.cuda(), n_top.cuda(), out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu()


def close(g: float, w: float) -> bool:
    if w == NINF or g == NINF:
        return g == w
    return g == g and abs(g - w) <= ATOL


def check(got, x, V, targets, n_top):
    want = reference_rows(x, V, targets, n_top)  # float64, independent of ops/reference.py
    lp, rank, ids, top = sampler.unpack_prompt_logprobs(got)
    for r, w in enumerate(want):
        if w is None:
            assert torch.equal(got[r], torch.full_like(got[r], SENTINEL)), r
            continue
        wlp, wrank, wids, wtop = w
        assert int(rank[r]) == wrank, (r, int(rank[r]), wrank)
        assert ids[r].tolist() == wids, (r, ids[r].tolist(), wids)
        assert close(float(lp[r]), wlp), (r, float(lp[r]), wlp)
        for j in range(NMAX):
            assert close(float(top[r, j]), wtop[j]), (r, j, float(top[r, j]), wtop[j])
        n = min(int(n_top[r]), NMAX, V)
        if 0 < wrank <= n:  # the target sits at position rank - 1 of the list
            assert wids[wrank - 1] == int(targets[r])


def padded(R, V, dtype, seed):
    """Random rows in a buffer 64 columns wider than V, the padding NaN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((R, V + 64), float("nan"))
    x[:, :V] = torch.randn(R, V, generator=g) * 3
    return x.to(dtype), g


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", WIDTHS)
def test_constructed_rows(V, dtype):
    R = 16
    x, g = padded(R, V, dtype, seed=V)
    n_top = torch.tensor([N_MIX[r % len(N_MIX)] for r in range(R)], dtype=torch.int32)
    targets = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    n_top[0], n_top[5], n_top[10] = 0, 5, 20  # rows 0, 5, 10 would be "not asked" in the mix
    x[0, :V] = 1.5                                        # all equal: rank = t + 1
    x[1, :V] = 1.5
    x[2, :V] = 1.5
    targets[0], targets[1], targets[2] = 0, V // 2, V - 1
    x[3, :V] = (torch.arange(V) % 251).to(dtype)          # exact in bf16, long runs of ties
    targets[3] = min(V - 1, 251 + 17)
    x[4, :V] = 0.0                                        # signed zeros compare equal
    x[4, 1:V:2] = -0.0
    targets[4] = V - 1
    x[5, 0:V:3] = NINF                                    # -inf entries, the target on one
    targets[5] = 3 if V > 3 else 0
    x[6, :V] = NINF                                       # an all -inf row: -inf, never NaN
    targets[6] = V // 2
    targets[7] = int(torch.argmax(x[7, :V].float()))      # target = argmax: rank 1
    x[8, :V] = -2.0                                       # the last id among ties of the maximum
    tie = sorted({0, V // 2, V - 1})
    x[8, tie] = 7.0
    targets[8] = V - 1
    targets[9] = V + 5                                    # target >= V: -inf, rank 0, list as usual
    n_top[9] = 5
    targets[11] = -1                                      # no target: untouched whatever n_top says
    n_top[11] = 20
    got = run(x, V, targets, n_top)
    check(got, x, V, targets, n_top)
    lp, rank, ids, top = sampler.unpack_prompt_logprobs(got)
    assert [int(rank[r]) for r in (0, 1, 2)] == [1, V // 2 + 1, V]
    assert int(rank[4]) == V and int(rank[7]) == 1 and int(rank[8]) == len(tie) and int(rank[9]) == 0
    assert torch.isneginf(lp[5]) and torch.isneginf(lp[6]) and torch.isneginf(lp[9])
    assert int(rank[6]) == V // 2 + 1 and not torch.isnan(lp).any()
    assert torch.equal(got[11], torch.full_like(got[11], SENTINEL))
    assert not torch.isnan(top[[r for r in range(R) if n_top[r] >= 0 and targets[r] >= 0]]).any()


def random_rows():
    R, V = 16, 128256
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16)
    n_top = torch.tensor([N_MIX[r % len(N_MIX)] for r in range(R)], dtype=torch.int32)
    targets = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    targets[1] = V - 1
    targets[4] = int(torch.argmax(x[4].float()))
    targets[3] = int(torch.topk(x[3].float(), 3).indices[2])
    return x, V, targets, n_top


def test_random_rows_match_float64_and_pk_logprobs_bit_for_bit():
    x, V, targets, n_top = random_rows()
    got = run(x, V, targets, n_top)
    check(got, x, V, targets, n_top)
    # the anchor: pk_logprobs on the same rows with tokens = targets writes the same 41 words
    base = torch.full((x.shape[0], sampler.LOGPROB_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    sampler.logprobs(x.cuda(), targets.cuda(), n_top.cuda(), base)
    torch.cuda.synchronize()
    base = base.cpu()
    for r in range(x.shape[0]):
        if int(n_top[r]) < 0:
            continue
        assert int(got[r, 0]) == int(base[r, 0]), r
        assert torch.equal(got[r, 2:], base[r, 1:]), r


def test_refusals_leave_out_untouched():
    R, V = 2, 64
    x = torch.zeros((R, V + 8), dtype=torch.bfloat16, device="cuda")
    t = torch.zeros(R, dtype=torch.int32, device="cuda")
    n = torch.zeros(R, dtype=torch.int32, device="cuda")
    out = torch.full((R, W), SENTINEL, dtype=torch.int32, device="cuda")
    fn = native.lib().pk_prompt_logprobs
    s = native.stream_ptr()
    for V_, stride, dtype in ((V + 4, V + 8, 0), (V, V + 4, 0), (V, V - 8, 0), (0, V, 0), (V, V + 8, 2), (V, V + 8, -1)):
        assert fn(out.data_ptr(), x.data_ptr(), t.data_ptr(), n.data_ptr(), R, V_, stride, dtype, s) == -1
    with pytest.raises(native.KernelError):
        native.call("pk_prompt_logprobs", out.data_ptr(), x.data_ptr(), t.data_ptr(), n.data_ptr(), R, V + 4, V + 8, 0, s)
    assert fn(out.data_ptr(), x.data_ptr(), t.data_ptr(), n.data_ptr(), 0, V, V + 8, 0, s) == 0  # no rows: no launch
    torch.cuda.synchronize()
    assert out.cpu().eq(SENTINEL).all()
