"""The guided decoding kernels (csrc/kernels/grammar.hip) against the reference
(ops/reference.py), exactly: kept words are compared as int32 bit patterns, dropped ones are -inf,
NaN sentinels stand where nothing may be written.  Inputs: tests/grammar_cases.py."""
import numpy as np
import pytest
import torch

from polykey_service_amd.ops import grammar as gram
from polykey_service_amd.ops import reference as ref
from tests import grammar_cases as gc

pytestmark = pytest.mark.gpu

CHUNK = 256  # words per load call: every table arrives in pieces


def _device_state(case):
    st = gram.GrammarState(case["n_slots"], case["off"], case["data"], "cuda")
    for entry, g in gc.tables().items():
        words = torch.from_numpy(gram.pack(g.cmap, g.trans, g.accept)).cuda()
        for w0 in range(0, words.numel(), CHUNK):
            piece = words[w0:w0 + CHUNK].contiguous()
            gram.load(st, entry, w0, piece, piece.numel())
    ent = torch.from_numpy(case["entries"]).cuda().reshape(-1)
    gram.seed(st, ent, case["entries"].shape[0])
    return st


@pytest.mark.parametrize("V,B", gc.SHAPES)
def test_mask_and_advance_match_the_reference(V, B):
    case = gc.kernel_case(V, B)
    pool, rec = gc.cpu_state(case)
    st = _device_state(case)
    torch.cuda.synchronize()
    assert torch.equal(st.pool.cpu(), pool) and torch.equal(st.rec.cpu(), rec)  # chunked load, seed
    slots = torch.from_numpy(case["slots"]).cuda()
    want = gc.reference_mask(case, pool, rec)
    got = gc.poison(case).cuda()
    gram.mask(st, got, slots, B, V)
    torch.cuda.synchronize()
    dropped = int((torch.isinf(want) & ~torch.isinf(gc.poison(case))).sum())
    kept = int(torch.isfinite(want[:, :V]).sum())
    print(f"V={V} B={B}: {dropped} ids dropped, {kept} kept")
    assert dropped > 0 and kept > 0
    assert torch.equal(gc.bits(got.cpu()), gc.bits(want))
    toks = gc.pick_tokens(case, want)
    ref.grammar_advance(pool, rec, case["slots"], toks, B, case["off"], case["data"], V)
    gram.advance(st, slots, torch.from_numpy(toks).cuda(), B, V)
    torch.cuda.synchronize()
    assert torch.equal(st.rec.cpu(), rec)
    assert torch.equal(st.pool.cpu(), pool)


def test_graph_replays_follow_three_reference_steps():
    V, B = 1000, 5
    case = gc.kernel_case(V, B)
    pool, rec = gc.cpu_state(case)
    st = _device_state(case)
    slots = torch.from_numpy(case["slots"]).cuda()
    rows = gc.poison(case).cuda()
    toks = torch.zeros(B, dtype=torch.int32, device="cuda")

    def step():
        gram.mask(st, rows, slots, B, V)
        gram.advance(st, slots, toks, B, V)

    rec0 = st.rec.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up; its effects are undone below
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    st.rec.copy_(rec0)
    moved = 0
    for i in range(3):
        before = rec.clone()
        want = gc.reference_mask(case, pool, rec)
        t = gc.pick_tokens(case, want, i)
        ref.grammar_advance(pool, rec, case["slots"], t, B, case["off"], case["data"], V)
        moved += int((rec[:, 1] != before[:, 1]).sum())
        rows.copy_(gc.poison(case))
        toks.copy_(torch.from_numpy(t))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gc.bits(rows.cpu()), gc.bits(want)), i
        assert torch.equal(st.rec.cpu(), rec), i
    assert moved >= 3


def test_no_constrained_row_writes_nothing():
    case = gc.kernel_case(259, 1)
    st = _device_state(case)
    rows = torch.full((case["n_slots"], case["stride"]), float("nan"), device="cuda")
    for slots in ([-1], [case["n_slots"]], [int(np.setdiff1d(np.arange(case["n_slots"]), case["slots"])[0])]):
        s = torch.tensor(slots, dtype=torch.int32, device="cuda")
        rec = st.rec.clone()
        gram.mask(st, rows, s, 1, 259)
        gram.advance(st, s, torch.tensor([2], dtype=torch.int32, device="cuda"), 1, 259)
        torch.cuda.synchronize()
        assert bool(torch.isnan(rows).all()) and torch.equal(st.rec, rec)
