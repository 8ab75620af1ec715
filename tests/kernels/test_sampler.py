"""Sampler kernel (csrc/kernels/sampler.hip) against the float64 reference sampler.

Every sampled token is judged by the reference's own float64 scores (tests/sampler_cases.py
``check_rows``): it must lie in ``reference.sampling_mask`` and its score ``x / T - log(-log u)``
must be within DELTA of the row's best, which is equality with ``reference.sample`` on every row
whose top-two gap exceeds DELTA.  No row is skipped.

DELTA = 32 x the fp32 floor = 1.26e-4.  The floor is the largest |fp32 - float64| of the reference
formula evaluated with every operation rounded to fp32, over all tokens within 1.0 of winning, on
the inputs of ``test_matches_reference`` and ``test_heterogeneous_batch`` (measured on the CPU;
tests/unit/test_sampler_reference.py re-measures it on the small shapes):
    V = 4,104 bf16 3.3e-6, fp32 3.95e-6, strided 3.6e-6, all-negative fp32 2.1e-6;
    V = 40 3.4e-6;  V = 128,256 3.7e-6;  heterogeneous 1.8e-6 / 1.3e-6.
The factor 32 is for the kernel's fast exp / log.  Rows with a top-two gap under DELTA, checked on
the CPU: 0 of the 2,886 sampled rows of those two tests (0 %; 4 rows, 0.14 %, have a gap under
2e-3), so the check means equality with ``reference.sample`` on every one of them.

Survivor sets are recovered from the kernel by coverage: one constructed row, 4,096 seeds, every
survivor at a renormalised probability >= 1/64 (a survivor stays unseen with probability
<= (63/64)^4096 ~ e^-64), every boundary clear of p by >= 0.03 in cumulative mass after bf16
rounding.  The set of tokens seen must equal the hand-written set, and their counts pass a
chi-square at p = 1e-4 against the renormalised probabilities.  Seeds are fixed: deterministic.
"""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import sampler
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu


def params(B, temp=0.0, k=0, p=1.0, mp=0.0, seed=0, off=0, device="cuda"):
    f = lambda v, dt: torch.full((B,), v, dtype=dt, device=device)
    return (f(temp, torch.float32), f(k, torch.int32), f(p, torch.float32), f(mp, torch.float32),
            torch.arange(B, dtype=torch.int32, device=device) + seed, f(off, torch.int32))


def launch(x, prm, out=None):
    """One sampler launch on CPU-side inputs -> tokens on the CPU."""
    got = sampler.sample(x, *[t.cuda() for t in prm], out=out)
    torch.cuda.synchronize()
    return got.cpu()


@pytest.mark.parametrize("V,dtype", [(128256, torch.bfloat16), (32000, torch.float32), (1024, torch.bfloat16)])
def test_greedy(V, dtype):
    x = torch.randn(64, V, device="cuda").to(dtype)
    x[5, 17] = 100.0
    x[6, :] = 1.0  # ties → lowest index
    out = sampler.sample(x, *params(64))
    exp = torch.argmax(x.float(), -1)
    exp[6] = 0
    assert torch.equal(out.long().cpu(), exp.cpu())
    assert torch.equal(sampler.greedy(x).long().cpu(), exp.cpu())


def test_top_k_1_is_greedy_and_rng_matches_reference():
    V, B = 4096, 16
    x = torch.randn(B, V, device="cuda") * 3
    out = sampler.sample(x, *params(B, temp=1.0, k=1))
    assert torch.equal(out.long().cpu(), torch.argmax(x, -1).cpu())
    # plain temperature sampling: every row is the reference's draw
    prm = params(B, temp=0.8, off=11, device="cpu")
    differ, close = sc.check_rows(x.cpu(), launch(x, prm), *prm)
    assert differ <= close


@pytest.mark.parametrize("k,p,mp", [(50, 1.0, 0.0), (0, 0.9, 0.0), (40, 0.5, 0.0), (0, 1.0, 0.1), (7, 0.95, 0.05)])
def test_survivor_sets(k, p, mp):
    """Random rows: every token lies in the reference mask and is the reference's draw.  That the
    survivor set is not too small either: test_survivor_set_and_distribution."""
    V, B = 32000, 8
    torch.manual_seed(0)
    x = torch.randn(B, V, device="cuda") * 2
    xc = x.cpu()
    for trial in range(20):
        prm = params(B, temp=0.7, k=k, p=p, mp=mp, seed=trial * 100, off=trial, device="cpu")
        sc.check_rows(xc, launch(x, prm), *prm)


def test_distribution_chi2():
    V = 8
    logits = torch.tensor([[2.0, 1.0, 0.5, 0.0, -1.0, -2.0, 0.3, 1.5]], device="cuda").repeat(4096, 1)
    B = logits.shape[0]
    t, k, p, mp, seeds, offs = params(B, temp=1.0)
    counts = np.zeros(V)
    for it in range(4):
        out = sampler.sample(logits, t, k, p, mp, seeds + it * B, offs).cpu().numpy()
        counts += np.bincount(out, minlength=V)
    probs = torch.softmax(logits[0].cpu(), -1).numpy()
    expct = probs * counts.sum()
    chi2 = ((counts - expct) ** 2 / expct).sum()
    assert chi2 < 30, (chi2, counts, expct)  # 7 dof, p≈1e-4


@pytest.mark.parametrize("B,V,dtype,negative,width,use_out,gen_seed", [
    (256, 128256, torch.bfloat16, False, None, False, 0),
    (512, 4096 + 8, torch.bfloat16, False, None, False, 1),       # the last slice is partial
    (512, 4096 + 8, torch.float32, False, None, False, 2),
    (512, 40, torch.bfloat16, False, None, False, 3),             # fewer than one vector per thread
    (512, 4096 + 8, torch.bfloat16, False, 4096 + 8 + 64, False, 4),  # a column slice of a wider buffer
    (512, 4096 + 8, torch.float32, True, None, True, 5),          # all logits negative; out= given
], ids=["128k-bf16", "4104-bf16", "4104-fp32", "40-bf16", "4104-strided", "4104-negative-out"])
def test_matches_reference(B, V, dtype, negative, width, use_out, gen_seed):
    """Temperatures 0.3 / 0.8 / 1.0 / 1.7 and five filter settings cycling over the rows, a seed
    and an offset per row: every token is the reference's draw (module docstring)."""
    x, prm = sc.random_case(B, V, dtype, negative=negative, width=width, gen_seed=gen_seed)
    xd = x.cuda()[:, :V]
    assert xd.stride(0) == (width or V)
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda") if use_out else None
    got = launch(xd, prm, out)
    if use_out:
        assert torch.equal(out.cpu(), got)
    differ, close = sc.check_rows(x[:, :V], got, *prm)
    print(f"rows not identical to the reference: {differ} of {B} (top-two gap under DELTA: {close})")


@pytest.mark.parametrize("V,reps", [(4096 + 8, 8), (128256, 2)])
def test_heterogeneous_batch(V, reps):
    """Greedy padding rows next to sampled rows, each filter alone / together / off, k = 1,
    T = 1e-4, all in one launch; the same requests rolled by 3 rows get the same tokens."""
    x, prm = sc.hetero_case(V, torch.bfloat16, reps)
    got = launch(x.cuda(), prm)
    differ, close = sc.check_rows(x, got, *prm)
    print(f"rows not identical to the reference: {differ} of {x.shape[0]} (top-two gap under DELTA: {close})")
    greedy = torch.argmax(x.float(), -1)
    for b in range(x.shape[0]):
        if b % 9 in (0, 1, 8):  # greedy, T = 1e-4 (bf16 randn x 3 rows: the maximum is unique), k = 1
            assert (x[b].float() == x[b].float().max()).sum() == 1
            assert int(got[b]) == int(greedy[b]), (b, b % 9)
    rolled = launch(x.roll(3, 0).cuda(), [t.roll(3, 0) for t in prm])
    assert torch.equal(rolled, got.roll(3, 0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(sc.LADDER_CASES))
def test_survivor_set_and_distribution(name, dtype):
    """The set of tokens the kernel returns over 4,096 seeds equals the hand-written survivor set
    (not too large, not too small), and their counts follow the renormalised probabilities."""
    row, temp, k, p, mp, survivors = sc.ladder_row(name, dtype)
    prm = sc.ladder_params(name)
    got = launch(row.cuda().repeat(sc.LADDER_N, 1), prm).tolist()
    assert sorted(set(got)) == survivors, (name, sorted(set(got)), survivors)
    chi2, bound = sc.chi2_of(got, row, temp, survivors)
    print(f"chi2 {chi2:.2f} (bound {bound}, {len(survivors) - 1} dof)")
    assert chi2 < bound, (name, chi2, bound)


@pytest.mark.parametrize("V", [128256, 4096 + 8])
def test_largest_uniform_is_not_one(V):
    """The largest value of the uniform stream, 1 - 2^-25, is a Gumbel draw of 17.33, not +inf: a
    token holding it 30 below the maximum loses, as in the reference, one within 3 of the maximum
    wins, as in the reference, and one behind a top-k filter stays out."""
    x, prm, idxs = sc.u_max_case(V)
    got = launch(x.cuda(), prm)
    differ, close = sc.check_rows(x, got, *prm)
    assert differ == 0 and close == 0, (differ, close)
    toks = got.tolist()
    assert all(toks[b] != idxs[b] for b in (0, 1, 2, 4)), (toks, idxs)
    assert toks[3] == idxs[3], (toks, idxs)


def test_graph_replay_equals_eager():
    B, V = 32, 4096 + 8
    x, prm = sc.random_case(B, V, torch.bfloat16, gen_seed=6)
    xd, pd = x.cuda(), [t.cuda() for t in prm]
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sampler.sample(xd, *pd, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sampler.sample(xd, *pd, out=out)
    # new step, same buffers: other logits, and every row another request's parameters
    x2, prm2 = sc.hetero_case(V, torch.bfloat16, 4, gen_seed=7)
    x2, prm2 = x2[:B], [t[:B].roll(5) for t in prm2]
    xd.copy_(x2)
    for d, t in zip(pd, prm2):
        d.copy_(t)
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.cpu()
    assert torch.equal(replayed, launch(x2.cuda(), prm2))
    sc.check_rows(x2, replayed, *prm2)


@pytest.mark.parametrize("V", [40, 64, 4096 + 8, 128256])
def test_greedy_ties_across_slices(V):
    """Greedy ties: a maximum repeated far apart in the row (different threads' vectors, different
    waves) resolves to its lowest index, at vocabularies below one vector per thread too; the
    full sampler and the greedy entry agree on every row, an all -inf row included."""
    x = torch.randn(16, V, device="cuda").to(torch.bfloat16)
    x[0, V - 1] = 50.0
    x[0, V // 2] = 50.0
    x[0, 3] = 50.0  # three slices hold the max: index 3 wins
    x[1, V - 1] = 60.0
    x[1, V - 9] = 60.0
    x[2, :] = -float("inf")
    exp = torch.argmax(x.float(), -1)
    exp[0], exp[1] = 3, V - 9
    got = sampler.greedy(x).long().cpu()
    assert torch.equal(got[:2], exp[:2].cpu()) and torch.equal(got[3:], exp[3:].cpu())
    assert torch.equal(sampler.sample(x, *params(16)).long().cpu(), got)
