"""The CPU reference sampler (ops/reference.py: philox_uniform, sampling_mask, sample), checked on
its own: tests/kernels/test_sampler.py judges the HIP kernel by it."""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import reference as ref
from tests import sampler_cases as sc

M = 0xFFFFFFFF


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    h ^= h >> 16
    return h


def scalar_uniform(seed, offset, idx):
    """The kernel's hash (csrc/kernels/sampler.hip row_hash / fmix32) in plain Python integers."""
    h = ((seed & M) * 0x9E3779B1 + 0x7F4A7C15) & M
    h ^= ((offset & M) + 0x85EBCA6B + ((h << 6) & M) + (h >> 2)) & M
    rh = _fmix32(h)
    x = _fmix32(rh ^ ((idx * 0xC2B2AE35) & M))
    return ((x >> 8) + 0.5) / (1 << 24)


def test_philox_uniform_matches_scalar_hash():
    rng = np.random.default_rng(0)
    triples = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, 5, 7), (2 ** 31 - 1, 2 ** 31 - 1, 128255), (-2 ** 31, 3, 4103)]
    triples += [(int(s), int(o), int(i)) for s, o, i in zip(rng.integers(-2 ** 31, 2 ** 31, 300),
                                                            rng.integers(0, 2 ** 31, 300), rng.integers(0, 128256, 300))]
    for seed, off, idx in triples:
        assert ref.philox_uniform(seed, off, idx + 1)[idx] == scalar_uniform(seed, off, idx), (seed, off, idx)
    for V, hits in sc.U_MAX_HITS.items():
        for seed, off, idx in hits:
            assert scalar_uniform(seed, off, idx) == sc.U_MAX
            u = ref.philox_uniform(seed, off, V)
            assert u[idx] == sc.U_MAX and u.max() == sc.U_MAX


def test_philox_uniform_statistics():
    """2^20 draws: strictly inside (0, 1), on the half-integer grid of 2^-24, mean and variance of
    a uniform, flat over 16 bins (chi-square at p = 1e-4); a prefix of a longer stream is the
    shorter stream."""
    n = 1 << 20
    u = ref.philox_uniform(12345, 6, n)
    assert u.dtype == np.float64 and u.min() >= 2.0 ** -25 and u.max() <= 1 - 2.0 ** -25
    assert np.array_equal(u * (1 << 24) - 0.5, np.floor(u * (1 << 24)))
    assert abs(u.mean() - 0.5) < 5 * (1 / 12 / n) ** 0.5
    assert abs(u.var() - 1 / 12) < 5 * (1 / 180 / n) ** 0.5
    counts = np.bincount((u * 16).astype(int), minlength=16)
    assert ((counts - n / 16) ** 2 / (n / 16)).sum() < sc.CHI2_1E4[15]
    assert np.array_equal(ref.philox_uniform(12345, 6, 1000), u[:1000])
    assert not np.array_equal(ref.philox_uniform(12345, 7, 1000), u[:1000])
    assert not np.array_equal(ref.philox_uniform(12346, 6, 1000), u[:1000])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(sc.LADDER_CASES))
def test_sampling_mask_on_ladders(name, dtype):
    """The hand-written survivor sets of the constructed rows; every survivor's renormalised
    probability is >= 1/64, which is what makes the kernel test's coverage argument hold."""
    row, temp, k, p, mp, survivors = sc.ladder_row(name, dtype)
    mask = ref.sampling_mask(row[None], temp, k, p, mp)[0]
    assert torch.nonzero(mask).view(-1).tolist() == survivors
    assert sc.survivor_probs(row, temp, survivors).min() >= 1 / 64
    assert len(survivors) == {"top_k_4": 4, "top_k_7_tied": 9, "top_p_062": 3, "top_k_4_top_p_06": 2, "min_p_03": 4,
                              "min_p_03_t05": 2}.get(name, len(survivors))


def test_sampling_mask_filters_off():
    x = torch.randn(3, 64)
    for k, p, mp in ((0, 1.0, 0.0), (64, 1.0, 0.0), (1000, 1.0, 0.0), (-1, 1.0, 0.0)):
        assert ref.sampling_mask(x, 0.7, k, p, mp).all()
    one = ref.sampling_mask(x, 0.7, 1, 1.0, 0.0)
    assert one.sum(-1).tolist() == [1, 1, 1] and torch.equal(one.float().argmax(-1), x.argmax(-1))


@pytest.mark.parametrize("name", list(sc.LADDER_CASES))
def test_sample_distribution_on_ladders(name):
    """reference.sample on the rows and seeds of the kernel test: the tokens drawn are exactly the
    survivors and their counts pass the same chi-square."""
    row, temp, k, p, mp, survivors = sc.ladder_row(name, torch.bfloat16)
    got = ref.sample(row.repeat(sc.LADDER_N, 1), *sc.ladder_params(name)).tolist()
    assert sorted(set(got)) == survivors
    chi2, bound = sc.chi2_of(got, row, temp, survivors)
    assert chi2 < bound, (chi2, bound)


def test_sample_greedy_rows_and_mixed_batch():
    """T = 0 rows are the argmax (lowest index on ties) whatever the other parameters say; the
    reference passes the check the kernel is held to; a request keeps its token when the batch
    is rolled."""
    x, prm = sc.hetero_case(4096 + 8, torch.bfloat16, 4)
    x[0, 100] = x[0, 7] = 50.0
    got = ref.sample(x, *prm)
    assert got.dtype == torch.int64 and int(got[0]) == 7
    for b in range(0, x.shape[0], 9):
        assert int(got[b]) == int(torch.argmax(x[b].float()))
    assert sc.check_rows(x, got, *prm) == (0, 0)
    assert torch.equal(ref.sample(x.roll(3, 0), *[t.roll(3, 0) for t in prm]), got.roll(3, 0))


@pytest.mark.parametrize("V", list(sc.U_MAX_HITS))
def test_sample_largest_uniform(V):
    """The rows of the kernel's u = 1 regression, on the reference: the token holding the largest
    uniform draws a Gumbel value of 17.33; it loses 30 below the maximum and wins 3 below it."""
    x, prm, idxs = sc.u_max_case(V)
    got = ref.sample(x, *prm).tolist()
    assert all(got[b] != idxs[b] for b in (0, 1, 2, 4)) and got[3] == idxs[3]
    assert abs(-np.log(-np.log(sc.U_MAX)) - 17.33) < 0.005
    assert sc.check_rows(x, got, *prm) == (0, 0)


@pytest.mark.parametrize("B,V,dtype,negative,gen_seed", [
    (512, 4096 + 8, torch.bfloat16, False, 1), (512, 4096 + 8, torch.float32, False, 2),
    (512, 40, torch.bfloat16, False, 3), (512, 4096 + 8, torch.float32, True, 5)])
def test_fp32_floor_is_what_delta_assumes(B, V, dtype, negative, gen_seed):
    """DELTA = 32 x FP32_FLOOR: the floor, re-measured on the kernel test's small inputs (the
    reference formula rounded to fp32 at every step against float64, over the tokens within 1.0 of
    winning), stays under the constant, and no row of them has a top-two gap under DELTA."""
    assert sc.DELTA == 32 * sc.FP32_FLOOR and sc.DELTA <= 2e-3
    x, prm = sc.random_case(B, V, dtype, negative=negative, gen_seed=gen_seed)
    t, _, _, _, seeds, offs = prm
    floor = 0.0
    for b in range(B):
        s64 = sc.ref_scores(x[b], float(t[b]), int(seeds[b]), int(offs[b]))
        s32 = sc.fp32_scores(x[b], float(t[b]), int(seeds[b]), int(offs[b]))
        near = s64 >= s64.max() - 1.0
        floor = max(floor, float(np.abs(s32[near].astype(np.float64) - s64[near]).max()))
    assert floor <= sc.FP32_FLOOR, floor
    assert sc.check_rows(x, ref.sample(x, *prm), *prm) == (0, 0)
