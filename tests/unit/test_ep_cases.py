"""The expert all-to-all cases (tests/ep_cases.py) on the CPU: the reference model passes its own
checks on every (world, shape, call), every mutant of the contract fails them on some case, and the
case list reaches every loop trip and edge of csrc/comm/ep_alltoall.hip -- so a GPU kernel that
passes the same checks moves the rows the contract says."""
import pytest
import torch

from tests import ep_cases as ec

SEQUENCES = [(w, s) for w in ec.WORLDS for s in ec.SHAPES]


def run_sequence(world, shape, mutant=None):
    """The call sequence with no refill between calls: the (possibly mutated) model runs on, and each
    call is checked against what the contract makes of the correct state before it."""
    C, H = ec.SHAPES[shape]
    bufs = ec.Buffers(world, C, H)
    good_x = [b.clone() for b in bufs.recv_x]
    good_r = [b.clone() for b in bufs.ret_x]
    for call in range(len(ec.CALLS)):
        sends = ec.make_sends(world, shape, call)
        ec.dispatch_ref(world, C, sends, bufs, mutant)
        for d in range(world):
            good_x[d], _ = ec.check_dispatch(d, world, C, bufs.recv_x[d], bufs.recv_e[d], sends, good_x[d])
        y = [ec.expert_bits(d, bufs.recv_x[d], bufs.recv_e[d]) for d in range(world)]
        ec.return_ref(world, C, y, sends, bufs, mutant)
        for s in range(world):
            good_r[s] = ec.check_return(s, world, C, bufs.ret_x[s], sends, good_r[s])


@pytest.mark.parametrize("world,shape", SEQUENCES)
def test_the_reference_passes_its_own_checks(world, shape):
    run_sequence(world, shape)


@pytest.mark.parametrize("mutant", ec.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    rejected = []
    for world, shape in SEQUENCES:
        try:
            run_sequence(world, shape, mutant)
        except AssertionError:
            rejected.append((world, shape))
    assert rejected, mutant
    # at every world size, not only at one
    assert {w for w, _ in rejected} == set(ec.WORLDS), (mutant, rejected)


def test_a_wrong_key_or_rank_is_seen_in_the_returned_row():
    ks = {int(ec.key(d, torch.tensor([e]))[0]) for d in range(8) for e in range(-1, 8)}
    assert len(ks) == 8 * 9


def test_rows_hold_nan_and_negative_zero_patterns_and_differ():
    b = ec.row_bits(3, 2, 50, 8)
    f = b.view(torch.bfloat16).float()
    assert bool(torch.isnan(f).any()) and int(b[0, 0]) == -0x8000
    assert len({tuple(r.tolist()) for r in b}) == 50
    assert not torch.equal(b, ec.row_bits(3, 1, 50, 8)) and not torch.equal(b, ec.row_bits(2, 2, 50, 8))
    assert len(set(ec.row_ids(3, 2, 50).tolist())) == 8


@pytest.mark.parametrize("world", sorted(ec.MOE_TOKENS))
def test_the_moe_operands_route_as_planned_and_poison_unused_experts(world):
    from tests import moe_cases as mc
    E, k, C = ec.MOE_E, ec.MOE_K, ec.MOE_C
    per = E // world
    rounds = ec.MOE_TOKENS[world]
    flat = [t for tokens in rounds for t in tokens]
    assert 0 in flat and 1 in flat and max(flat) >= 17 and all(len(t) == world for t in rounds)
    multi_tile = False
    for rnd, tokens in enumerate(rounds):
        assert max(tokens) * k <= C
        xs, router, w13, w2 = ec.moe_operands(world, rnd)
        used = set()
        for r, T in enumerate(tokens):
            assert xs[r].shape == (T, ec.MOE_H)
            ids, w = mc.route64(xs[r].double() @ router.double().t(), k, True)
            assert ids.tolist() == [list(p) for p in ec.moe_routes(r, T)]  # the planned experts, in order
            used.update(ids.flatten().tolist())
            for e in range(E):  # rows one peer sends one expert: more than a 16-row tile somewhere
                multi_tile |= e // per != r and int((ids == e).sum()) > 16
        nan13, nan2 = torch.isnan(w13.float()).flatten(1), torch.isnan(w2.float()).flatten(1)
        for e in range(E):
            assert bool(nan13[e].all()) == bool(nan2[e].all()) == bool(nan13[e].any()) == (e not in used)
        assert 7 not in used
    assert multi_tile


def test_the_case_list_reaches_every_loop_trip_and_edge():
    seen = set()
    for world, shape in SEQUENCES:
        C, H = ec.SHAPES[shape]
        prev = None
        for call in range(len(ec.CALLS)):
            n = ec.counts(world, C, call)
            assert all(sum(row) <= C for row in n)
            for s in range(world):
                if sum(n[s]) == 0:
                    seen.add("idle rank")
                for d in range(world):
                    v = n[s][d]
                    if v > 64 and v % 64:
                        seen.add("n > 64, n % 64 != 0")
                    if v == C:
                        seen.add("n == C")
                    if v > 16384:
                        seen.add("n > 16384")
                    if C - v > 16384:
                        seen.add("C - n > 16384")
                    if v > 0 and s == d:
                        seen.add("self-send")
                    if v in (63, 64, 65):
                        seen.add(f"n == {v}")
                    if v and H // 8 > 256:
                        seen.add("row wider than 256 units")
                    if prev is not None and prev[s][d] > 0 and v < prev[s][d]:
                        seen.add("shrinks")
                    if prev is not None and prev[s][d] == C and 0 < v < C:
                        seen.add("small after full")
            prev = n
    assert seen == {"idle rank", "n > 64, n % 64 != 0", "n == C", "n > 16384", "C - n > 16384", "self-send",
                    "n == 63", "n == 64", "n == 65", "row wider than 256 units", "shrinks", "small after full"}, seen
    assert (ec.SHAPES["B"][1] // 8) % 256 == 1  # the column loop's second trip has a remainder of one
