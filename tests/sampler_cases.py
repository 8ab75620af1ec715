"""Inputs and float64 checks shared by the sampler tests: tests/kernels/test_sampler.py (the HIP
kernel) and tests/unit/test_sampler_reference.py (the CPU reference the kernel is judged by).

Everything here runs on the CPU.  The kernel's token for a row is judged by the *reference's*
scores: it must lie in ``reference.sampling_mask`` and its float64 Gumbel-max score
``x / T - log(-log u)``, ``u = reference.philox_uniform(seed, offset, V)``, must be within
``DELTA`` of the row's best.  How ``DELTA`` was set is in the docstring of test_sampler.py.
"""
import math

import numpy as np
import torch

from polykey_service_amd.ops import reference as ref

FP32_FLOOR = 3.95e-6        # largest |fp32 - float64| score among near-winners, measured on the CPU
DELTA = 32 * FP32_FLOOR     # 1.26e-4

# chi-square critical values at p = 1e-4, by degrees of freedom
CHI2_1E4 = {1: 15.137, 2: 18.421, 3: 21.108, 4: 23.513, 5: 25.745, 6: 27.856, 7: 29.878, 8: 31.828, 15: 44.263}

NINF = float("-inf")


# ---------------------------------------------------------------------------- per-row checks
def ref_scores(row: torch.Tensor, temp: float, seed: int, offset: int) -> np.ndarray:
    """float64 Gumbel-max scores of one logits row (no mask)."""
    x = row.double().numpy()
    u = ref.philox_uniform(seed, offset, x.shape[0])
    return x / temp - np.log(-np.log(u))


def fp32_scores(row: torch.Tensor, temp: float, seed: int, offset: int) -> np.ndarray:
    """The same scores with every operation rounded to fp32:
    fl(x * fl(1 / T)) - fl(log(fl(-log1p(-fl(1 - u))))).  Used to measure the fp32 floor."""
    f = np.float32
    x = row.float().numpy()
    u = ref.philox_uniform(seed, offset, x.shape[0])
    w = (1.0 - u).astype(f)
    with np.errstate(divide="ignore"):  # u < 2^-25 rounds w to 1: the draw is -inf, far from winning
        t = (-np.log1p(-w.astype(np.float64))).astype(f)
        g = np.log(t.astype(np.float64)).astype(f)
    s = x * (f(1.0) / f(temp))
    return (s - g).astype(f)


def check_rows(logits, tokens, temperature, top_k, top_p, min_p, seeds, offsets, delta=DELTA):
    """Every row of one launch against the reference (all arguments on the CPU).  A greedy row
    (temperature <= 0) must be the argmax exactly.  A sampled row's token must be in the reference
    mask and score within ``delta`` of the reference's best, which is equality wherever the row's
    top-two gap exceeds ``delta``.  Returns (rows not identical to the reference, rows whose
    top-two gap is under ``delta``)."""
    B, V = logits.shape
    tokens = [int(t) for t in tokens]
    differ = close = 0
    for b in range(B):
        t, tok = float(temperature[b]), tokens[b]
        assert 0 <= tok < V, (b, tok)
        row = logits[b]
        if t <= 0.0:
            assert tok == int(torch.argmax(row.float())), ("greedy row", b, tok)
            continue
        k, p, mp = int(top_k[b]), float(top_p[b]), float(min_p[b])
        keep = ref.sampling_mask(row[None], t, k, p, mp)[0].numpy()
        assert keep[tok], ("token outside the reference mask", b, tok, t, k, p, mp)
        sc = np.where(keep, ref_scores(row, t, int(seeds[b]), int(offsets[b])), -np.inf)
        best = int(np.argmax(sc))
        assert sc[tok] >= sc[best] - delta, ("not the reference's draw", b, tok, best, sc[best] - sc[tok], t, k, p, mp)
        differ += tok != best
        if keep.sum() > 1:
            close += sc[best] - np.partition(sc, -2)[-2] <= delta
    return differ, close


# -------------------------------------------------------------------------------- random rows
TEMPS = (0.3, 0.8, 1.0, 1.7)
# per-row filter cycle (top_k, top_p, min_p); 5 entries against 4 temperatures: every pairing occurs
FILTERS = ((0, 1.0, 0.0), (50, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (20, 0.95, 0.02))


def make_params(rows):
    """rows: list of (temperature, top_k, top_p, min_p, seed, offset) -> the six CPU tensors."""
    c = list(zip(*rows))
    f32, i32 = torch.float32, torch.int32
    return (torch.tensor(c[0], dtype=f32), torch.tensor(c[1], dtype=i32), torch.tensor(c[2], dtype=f32),
            torch.tensor(c[3], dtype=f32), torch.tensor(c[4], dtype=i32), torch.tensor(c[5], dtype=i32))


def random_case(B, V, dtype, negative=False, width=None, gen_seed=0):
    """randn x 3 logits (``negative``: shifted so every logit is below zero; ``width`` > V: a wider
    buffer whose first V columns are the logits) and per-row parameters cycling TEMPS x FILTERS
    with a seed and an offset of each row's own."""
    g = torch.Generator().manual_seed(gen_seed)
    x = torch.randn(B, width or V, generator=g) * 3
    if negative:
        x = x - x.max() - 1.0
    x = x.to(dtype)
    rows = [(TEMPS[b % 4], *FILTERS[b % 5], 1000 * gen_seed + b, (7 * b + 11) % 997) for b in range(B)]
    return x, make_params(rows)


def hetero_case(V, dtype, reps, gen_seed=5):
    """The batch the engine builds: greedy padding next to sampled rows, every filter alone,
    together, and switched off in its own way.  9 kinds x ``reps``."""
    kinds = [
        (0.0, 0, 1.0, 0.0),        # greedy
        (1e-4, 0, 1.0, 0.0),       # near-zero temperature: greedy where the maximum is unique
        (0.8, 0, 1.0, 0.0),        # plain temperature
        (1.0, 30, 1.0, 0.0),       # top-k only
        (1.7, 0, 0.8, 0.0),        # top-p only
        (0.8, 0, 1.0, 0.1),        # min-p only
        (1.0, 25, 0.9, 0.03),      # all three
        (0.3, V + 5, 1.0, 0.0),    # each filter off: k >= V, p = 1, min_p = 0
        (1.7, 1, 1.0, 0.0),        # k = 1
    ]
    g = torch.Generator().manual_seed(gen_seed)
    B = len(kinds) * reps
    x = (torch.randn(B, V, generator=g) * 3).to(dtype)
    rows = [(*kinds[b % 9], 77 + 13 * b, (31 * b + 5) % 509) for b in range(B)]
    return x, make_params(rows)


# ------------------------------------------------------------------ constructed survivor sets
LADDER_V = 4096 + 8
LADDER_N = 4096
# one position per 512-column stretch (each is read by another wave), the last in the partial slice
LADDER_POS = (3, 700, 1300, 2047, 2600, 3333, 4000, 4100, 999, 1777)
LADDER = (.30, .20, .15, .10, .08, .07, .05, .05)
LADDER_TIED = (.30, .20, .15, .10, .08, .07, .04, .04, .04)   # the 7th value tied three ways

# name -> (probabilities, shift, rest, temperature, top_k, top_p, min_p, survivors as ladder slots).
# logit = log(probability) + shift at LADDER_POS[slot]; every other column holds `rest`
# ("inf": -40 and -inf alternating).  The survivor sets are written out by hand:
#   top-k 4              the four largest.
#   top-k 7, ties        six values above the three-way tie at .04: the threshold keeps all nine.
#   top-p .62            mass before slot 0..3 = 0, .30, .50, .65: three start below .62.
#   top-k 4 + top-p .6   renormalised over the four (.75): .40, .267, .20, .133; mass before =
#                        0, .40, .667: two.  Over the whole row it would be 0, .30, .50, .65: three.
#   min-p .3, T = 1      p >= .3 * .30 = .09: four (.10 stays, .08 goes).
#   min-p .3, T = .5     probabilities are squared by the temperature: .09, .04, .0225, ...;
#                        >= .3 * .09 = .027 keeps two.  In unscaled space it would keep four.
LADDER_CASES = {
    "top_k_4": (LADDER, 5.0, -40.0, 1.0, 4, 1.0, 0.0, (0, 1, 2, 3)),
    "top_k_7_tied": (LADDER_TIED, 5.0, -40.0, 1.0, 7, 1.0, 0.0, (0, 1, 2, 3, 4, 5, 6, 7, 8)),
    "top_p_062": (LADDER, 5.0, -40.0, 1.0, 0, 0.62, 0.0, (0, 1, 2)),
    "top_k_4_top_p_06": (LADDER, 5.0, -40.0, 1.0, 4, 0.6, 0.0, (0, 1)),
    "min_p_03": (LADDER, 5.0, -40.0, 1.0, 0, 1.0, 0.3, (0, 1, 2, 3)),
    "min_p_03_t05": (LADDER, 5.0, -40.0, 0.5, 0, 1.0, 0.3, (0, 1)),
    "negative_top_k_4": (LADDER, -3.0, -40.0, 1.0, 4, 1.0, 0.0, (0, 1, 2, 3)),
    "negative_top_p_062": (LADDER, -3.0, -40.0, 1.0, 0, 0.62, 0.0, (0, 1, 2)),
    "straddle_top_k_4": (LADDER, 2.0, -40.0, 1.0, 4, 1.0, 0.0, (0, 1, 2, 3)),
    "straddle_top_p_062": (LADDER, 2.0, -40.0, 1.0, 0, 0.62, 0.0, (0, 1, 2)),
    "inf_rest_top_k_4_top_p_06": (LADDER, 5.0, "inf", 1.0, 4, 0.6, 0.0, (0, 1)),
    "inf_rest_min_p_03": (LADDER, 2.0, "inf", 1.0, 0, 1.0, 0.3, (0, 1, 2, 3)),
}


def ladder_row(name, dtype):
    """-> (row [LADDER_V] of ``dtype``, temperature, top_k, top_p, min_p, survivor token ids)."""
    probs, shift, rest, temp, k, p, mp, slots = LADDER_CASES[name]
    row = torch.full((LADDER_V,), -40.0 if rest == "inf" else rest, dtype=torch.float64)
    if rest == "inf":
        row[1::2] = NINF
    for slot, pr in enumerate(probs):
        row[LADDER_POS[slot]] = math.log(pr) + shift
    return row.to(dtype), temp, k, p, mp, sorted(LADDER_POS[s] for s in slots)


def ladder_params(name, n=LADDER_N):
    """The row's parameters for seeds 0..n-1, at an offset of the case's own (another stream)."""
    _, _, _, temp, k, p, mp, _ = LADDER_CASES[name]
    offset = list(LADDER_CASES).index(name)
    return make_params([(temp, k, p, mp, seed, offset) for seed in range(n)])


def survivor_probs(row, temp, survivors):
    """float64 renormalised probabilities of the survivor tokens, in the order given."""
    z = row.double()[survivors] / temp
    return torch.softmax(z, -1).numpy()


def chi2_of(tokens, row, temp, survivors):
    """(chi-square of the observed token counts against the renormalised reference
    probabilities, the p = 1e-4 bound for len(survivors) - 1 degrees of freedom)."""
    counts = np.array([(np.asarray(tokens) == s).sum() for s in survivors], dtype=np.float64)
    expect = survivor_probs(row, temp, survivors) * len(tokens)
    return float(((counts - expect) ** 2 / expect).sum()), CHI2_1E4[len(survivors) - 1]


# ----------------------------------------------------------------------------- the u = 1 draw
# (seed, offset, idx): philox_uniform(seed, offset, V)[idx] == 1 - 2**-25, the largest value of the
# stream (top 24 hash bits all ones).  In fp32, (float(x >> 8) + 0.5f) * 2^-24 rounds it to 1.0f.
U_MAX = 1.0 - 2.0 ** -25
U_MAX_HITS = {
    128256: ((3, 0, 38630), (22, 0, 125180), (25, 0, 14668)),
    4096 + 8: ((2046, 0, 2540), (6952, 0, 2609), (7349, 0, 1396)),   # about one seed in 4,000 has one
}


def u_max_case(V, dtype=torch.bfloat16):
    """Five rows of randn logits at T = 1 around the three hits of U_MAX_HITS[V]:
      0-2  the hit token 30 below the row maximum, no filter: its true Gumbel value is
           -log(-log(U_MAX)) = 17.33, so the reference does not pick it;
      3    the first hit within 3 of the maximum: the reference does pick it;
      4    the second hit 30 below the maximum again, behind a top-k 50 filter.
    -> (logits, parameters, hit token per row)."""
    hits = U_MAX_HITS[V]
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, V, generator=g)
    rows, idxs = [], []
    for b, (hit, below, k) in enumerate(((0, 30.0, 0), (1, 30.0, 0), (2, 30.0, 0), (0, 3.0, 0), (1, 30.0, 50))):
        seed, off, idx = hits[hit]
        x[b, idx] = NINF
        x[b, idx] = x[b].max() - below
        rows.append((1.0, k, 1.0, 0.0, seed, off))
        idxs.append(idx)
    return x.to(dtype), make_params(rows), idxs
