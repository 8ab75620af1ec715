"""The checkers of tests/prompt_logprobs_cases.py can fail: each rejects the mutants it is there to
catch, and accepts the real thing (ops/reference.py prompt_logprobs, model_runner.prompt_targets)."""
import math

import pytest
import torch

from polykey_service_amd.engine.model_runner import prompt_targets
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.ops import sampler
from tests import prompt_logprobs_cases as C


# ------------------------------------------------------------------ rank and list order
def _key(row):
    return torch.where(row == 0, torch.zeros_like(row), row).tolist()


def correct(row, t, n):
    v = _key(row)
    order = sorted(range(len(v)), key=lambda j: (-v[j], j))
    return 1 + sum(1 for j in range(len(v)) if v[j] > v[t] or (v[j] == v[t] and j < t)), order[:n]


def rank_ge(row, t, n):  # ">=" instead of the total order: every tie counts as ahead
    v = _key(row)
    return 1 + sum(1 for j in range(len(v)) if v[j] >= v[t] and j != t), correct(row, t, n)[1]


def ties_by_id_descending(row, t, n):
    v = _key(row)
    order = sorted(range(len(v)), key=lambda j: (-v[j], -j))
    return 1 + sum(1 for j in range(len(v)) if v[j] > v[t] or (v[j] == v[t] and j > t)), order[:n]


def rank_zero_based(row, t, n):
    rank, ids = correct(row, t, n)
    return rank - 1, ids


def signed_zeros_differ(row, t, n):  # -0.0 ordered below +0.0
    v = [(-1e-30 if str(f) == "-0.0" else f) for f in row.tolist()]
    order = sorted(range(len(v)), key=lambda j: (-v[j], j))
    return 1 + sum(1 for j in range(len(v)) if v[j] > v[t] or (v[j] == v[t] and j < t)), order[:n]


def test_row_checker_accepts_the_rule_and_the_cpu_reference():
    x, targets = C.tie_rows()
    C.check_rows(correct, x, targets)

    def cpu_reference(row, t, n):
        out = ref.prompt_logprobs(row[None], torch.tensor([t], dtype=torch.int32), torch.tensor([n], dtype=torch.int32))
        _, rank, ids, _ = sampler.unpack_prompt_logprobs(out)
        return int(rank[0]), ids[0, :n].tolist()
    C.check_rows(cpu_reference, x, targets)


@pytest.mark.parametrize("mutant", [rank_ge, ties_by_id_descending, rank_zero_based, signed_zeros_differ])
def test_row_checker_rejects(mutant):
    x, targets = C.tie_rows()
    with pytest.raises(AssertionError):
        C.check_rows(mutant, x, targets)


def test_reference_rows_special_cases():
    x, targets = C.tie_rows()
    V = x.shape[1]
    t = torch.tensor([V // 2, V + 3, -1, 3, 0], dtype=torch.int32)
    n = torch.tensor([0, 2, 5, -1, 1], dtype=torch.int32)
    rows = C.reference_rows(x, V, t, n)
    assert rows[2] is None and rows[3] is None
    assert rows[0][1] == V // 2 + 1 and abs(rows[0][0] + math.log(V)) < 1e-12
    assert rows[1][0] == C.NINF and rows[1][1] == 0 and rows[1][2][:2] == [6, 13]
    assert rows[4][0] == C.NINF and rows[4][1] == V - len(range(0, V, 5)) + 1  # a -inf target of a live row
    dead = C.reference_rows(torch.full((1, 16), C.NINF), 16, [5], [3])[0]
    assert dead[0] == C.NINF and dead[1] == 6 and dead[2][:3] == [0, 1, 2] and all(v == C.NINF for v in dead[3])


# ------------------------------------------------------------------ targets of a step's rows
def _rows(chunks):
    return [(s, p) for s, start, length in chunks for p in range(start, start + length)]


def _asks(s, i):
    return s.prompt_logprobs is not None and 0 < i < len(s.prompt_ids) and s.prompt_logprobs[i] is None


def own_token(chunks):  # the row's own token instead of the next one (off by one)
    return [s.prompt_ids[p] if _asks(s, p) else -1 for s, p in _rows(chunks)]


def shifted_input_ids(chunks):
    """The step's input ids shifted by one row: right inside a chunk, but the last row of a chunk
    gets the first token of the next sequence (or nothing) instead of the prompt's own next token."""
    rows = _rows(chunks)
    ids = [s.token_slice(p, p + 1)[0] for s, p in rows]
    out = []
    for r, (s, p) in enumerate(rows):
        nxt = ids[r + 1] if r + 1 < len(rows) else -1
        out.append(nxt if _asks(s, p + 1) else -1)
    return out


def last_row_of_chunk_dropped(chunks):
    out = []
    for s, start, length in chunks:
        for p in range(start, start + length):
            out.append(s.prompt_ids[p + 1] if _asks(s, p + 1) and p + 1 < start + length else -1)
    return out


def recorded_recomputed(chunks):  # ignores what is on record: a recompute duplicates entries
    return [s.prompt_ids[p + 1] if s.prompt_logprobs is not None and p + 1 < len(s.prompt_ids) else -1
            for s, p in _rows(chunks)]


def last_prompt_row_scores_first_output(chunks):
    return [s.token_slice(p + 1, p + 2)[0] if s.prompt_logprobs is not None and s.prompt_lp_missing
            and p + 1 < s.num_tokens and (p + 1 >= len(s.prompt_ids) or s.prompt_logprobs[p + 1] is None) else -1
            for s, p in _rows(chunks)]


def test_target_checker_accepts_prompt_targets():
    C.check_targets(prompt_targets)


@pytest.mark.parametrize("mutant", [own_token, shifted_input_ids, last_row_of_chunk_dropped, recorded_recomputed,
                                    last_prompt_row_scores_first_output])
def test_target_checker_rejects(mutant):
    with pytest.raises(AssertionError):
        C.check_targets(mutant)


def test_prompt_targets_examples():
    a = C.make_seq(range(100, 106))
    b = C.make_seq(range(200, 203))
    assert prompt_targets([(a, 0, 4), (b, 0, 3)]) == [101, 102, 103, 104, 201, 202, -1]
    assert prompt_targets([(a, 4, 2)]) == [105, -1]
    d = C.make_seq(range(400, 408), recorded=range(1, 5), outputs=[410, 411])
    assert prompt_targets([(d, 0, 10)]) == [-1, -1, -1, -1, 405, 406, 407, -1, -1, -1]
    assert prompt_targets([(C.make_seq(range(5), asks=False), 0, 5)]) == [-1] * 5
