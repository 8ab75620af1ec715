"""Engine-level checks of parallel sampling (SamplingParams.n > 1) shared by the CPU test
(tests/unit/test_parallel_sampling_cpu.py: tiny-llama, reference ops) and the GPU test
(tests/e2e/test_parallel_sampling_gpu.py: tiny-llama-gqa4, graphs on, bf16 and FP8 KV).  Every function
takes ``make(**engine_config_overrides) -> LLMEngine`` and steps the engine by hand."""
import math

import torch

from polykey_service_amd.engine import SamplingParams
from polykey_service_amd.ops import reference as ref

BS = 32


def prompt_of(P: int):
    return [1] + [5 + (i * 7) % 200 for i in range(P - 1)]


def drain(e):
    while e.has_unfinished():
        e.step()


def run(e, prompt, sp):
    """-> the request's choices (Sequence objects) after it ran to the end.  The prefix cache is
    emptied afterwards, so that the next request on this engine prefills its whole prompt again: two
    runs of one prompt then are the same launches, and their results may be compared exactly."""
    s0 = e.add_request(prompt, sp)
    drain(e)
    e.bm.reset_prefix_cache()
    return s0.choices or [s0]


def step_until_forked(e, s0):
    """Step until the step that completed choice 0's prompt (and forked) has run."""
    while s0.seq_id in e.scheduler.parked:
        e.step()


def _slots(e, seq, block_index, n_slots):
    """K and V of the first ``n_slots`` token slots of the sequence's block, per layer, as raw integers
    (gather_kv undoes the K tiling and V's transposed layout)."""
    table = torch.tensor(e.bm.table(seq.seq_id)[block_index:block_index + 1], dtype=torch.int32)
    out = []
    for k, v in e.runner.kv_caches:
        kk, vv = ref.gather_kv(k.cpu(), v.cpu(), table, n_slots)
        raw = torch.uint8 if kk.element_size() == 1 else torch.int16
        out.append((kk.contiguous().view(raw), vv.contiguous().view(raw)))
    return out


# ------------------------------------------------------------------------------ structure
def check_structure(make):
    e = make()
    nb = e.bm.num_blocks
    s0 = e.add_request(prompt_of(71), SamplingParams(max_tokens=4, temperature=1.0, seed=3, n=4, ignore_eos=True))
    assert [c.index for c in s0.choices] == [0, 1, 2, 3] and len(e.scheduler.parked[s0.seq_id]) == 3
    step_until_forked(e, s0)
    t0 = e.bm.table(s0.seq_id)
    assert len(t0) == 3
    privates = set()
    for c in s0.choices[1:]:
        t = e.bm.table(c.seq_id)
        assert t[:2] == t0[:2] and len(t) == 3 and t[2] != t0[2], (t, t0)
        privates.add(t[2])
        assert c.num_computed == 70 and c.forked_tokens == 70 and c.num_pending == 1
        assert e.bm.ref_count(t[2]) == 1
    assert len(privates) == 3
    assert [e.bm.ref_count(b) for b in t0] == [4, 4, 1]
    # the private block's first (71 - 1) % 32 = 6 token slots are choice 0's, bit for bit, K and V, every layer
    want = _slots(e, s0, 2, 6)
    assert len(want) == len(e.runner.kv_caches) and any(int(k.abs().max()) > 0 for k, _ in want)
    for c in s0.choices[1:]:
        for (k, v), (wk, wv) in zip(_slots(e, c, 2, 6), want):
            assert torch.equal(k, wk) and torch.equal(v, wv)
    assert e.kv_forks == 1 and e.kv_fork_fallbacks == 0 and e.kv_fork_shared_tokens == 3 * 70
    assert e.runner.stats.get("kv_copy_launches", 0) == 1
    assert e.scheduler.num_cached_tokens == 0  # a fork is no prefix-cache hit
    drain(e)
    assert all(len(c.output_ids) == 4 for c in s0.choices)
    assert e.bm.num_free == nb and e.bm.num_seqs == 0 and not e.scheduler.groups and not e.scheduler.by_request
    # (P - 1) % bs == 0: nothing to copy
    s0 = e.add_request(prompt_of(65), SamplingParams(max_tokens=3, n=3, ignore_eos=True))
    step_until_forked(e, s0)
    t0 = e.bm.table(s0.seq_id)
    for c in s0.choices[1:]:
        assert e.bm.table(c.seq_id) == t0[:2] and c.num_computed == 64
    assert e.runner.stats["kv_copy_launches"] == 1 and e.kv_forks == 2
    drain(e)
    assert [c.output_ids for c in s0.choices[1:]] == [s0.output_ids] * 2  # greedy choices are identical
    assert e.bm.num_free == nb


# ------------------------------------------------------- identity, repeatability, seeds
def check_identity_repeatability_seeds(make):
    e = make()
    prompt = prompt_of(71)
    sp = dict(max_tokens=8, temperature=1.0, seed=11, logprobs=5, ignore_eos=True)
    one = run(e, prompt, SamplingParams(n=1, **sp))[0]
    four = run(e, prompt, SamplingParams(n=4, **sp))
    again = run(e, prompt, SamplingParams(n=4, **sp))
    # choice 0 is the request as it runs with n = 1 on an idle engine: the same prefill launch, the same seed
    assert four[0].output_ids[0] == one.output_ids[0] and four[0].logprobs[0] == one.logprobs[0]
    assert [c.seed for c in four] == [11, 12, 13, 14]
    assert [c.output_ids for c in four] == [c.output_ids for c in again]
    assert all(len(c.output_ids) == 8 and len(c.logprobs) == 8 for c in four)
    assert len({tuple(c.output_ids) for c in four}) > 1, "four seeds, one stream"
    greedy = run(e, prompt, SamplingParams(max_tokens=8, n=4, ignore_eos=True))
    assert [c.output_ids for c in greedy[1:]] == [greedy[0].output_ids] * 3
    assert e.bm.num_free == e.bm.num_blocks


# ------------------------------------------------------------------------------ numerics
def _by_id(entry):
    lp, top = entry
    return dict(top)


def _max_diff(a, b):
    """Largest |difference| between two logprob records of one position: over the ids both top-5 lists
    hold -- at least 4 of the 5: one entry may change places with the sixth, a reshuffled list may not
    pass -- and the sampled token's own logprob where both runs sampled the same token (``a`` and ``b``
    are (token, record) pairs)."""
    (ta, (lpa, _)), (tb, (lpb, _)) = a, b
    da, db = _by_id(a[1]), _by_id(b[1])
    common = set(da) & set(db)
    assert len(common) >= 4, (da, db)
    d = max(abs(da[i] - db[i]) for i in common)
    return max(d, abs(lpa - lpb)) if ta == tb else d


def two_bf16_ulps(x: float) -> float:
    return 2.0 * 2.0 ** (math.floor(math.log2(x)) - 7)


def check_numerics(make):
    """-> (d_twin, d_fork, bound, differing tokens fork on vs off, tokens compared).  Asserts
    d_fork <= bound = max(3 x d_twin, two bf16 ulps at the forked row's largest |logit|)."""
    prompt = prompt_of(71)
    e = make()
    e.runner.keep_logits = True
    # d_twin, on code the fork does not touch: position P - 1 from the prompt's prefill (a) against the
    # same position computed by a one-row step (b: prompt X[:-1], forced by logit_bias to emit X[-1])
    a = run(e, prompt, SamplingParams(max_tokens=1, logprobs=5, ignore_eos=True))[0]
    a = (a.output_ids[0], a.logprobs[0])
    b = run(e, prompt[:-1], SamplingParams(max_tokens=2, logprobs=5, ignore_eos=True,
                                           logit_bias={prompt[-1]: 100.0}))[0]
    assert b.output_ids[0] == prompt[-1]
    d_twin = _max_diff(a, (b.output_ids[1], b.logprobs[1]))
    # the forked choices' first tokens, and the largest |logit| of their rows
    sp = dict(max_tokens=6, temperature=1.0, seed=5, logprobs=5, n=4, ignore_eos=True)
    s0 = e.add_request(prompt, SamplingParams(**sp))
    step_until_forked(e, s0)
    outs = e.step()
    logits = e.runner.last_logits.float().cpu()
    peak = {o.index: float(logits[r].abs().max()) for r, o in enumerate(outs)}
    assert all(c.forked_tokens == 70 and len(c.output_ids) == 1 for c in s0.choices[1:])
    drain(e)
    off = make(kv_fork=False)
    plain = run(off, prompt, SamplingParams(**sp))
    assert off.kv_forks == 0 and all(c.forked_tokens == 0 for c in plain)
    d_fork, bound = 0.0, 0.0
    for c, p in zip(s0.choices[1:], plain[1:]):
        d = _max_diff((c.output_ids[0], c.logprobs[0]), (p.output_ids[0], p.logprobs[0]))
        lim = max(3.0 * d_twin, two_bf16_ulps(peak[c.index]))
        print(f"choice {c.index}: first-token top-5 logprob diff fork on/off {d:.6g}, d_twin {d_twin:.6g}, "
              f"peak |logit| {peak[c.index]:.4g}, bound {lim:.6g}")
        assert d <= lim, (c.index, d, lim)
        d_fork, bound = max(d_fork, d), max(bound, lim)
    differing = sum(x != y for c, p in zip(s0.choices, plain) for x, y in zip(c.output_ids, p.output_ids))
    total = sum(len(c.output_ids) for c in s0.choices)
    print(f"d_twin {d_twin:.6g}  d_fork {d_fork:.6g}  bound {bound:.6g}  tokens differing fork on/off: "
          f"{differing} of {total}")
    return d_twin, d_fork, bound, differing, total


# ------------------------------------------------------------------------------ fallbacks
def check_no_block_at_fork_time(make):
    """A pool of exactly the 3 blocks choice 0 holds: no fork, the choices still complete."""
    e = make(num_kv_blocks=3, watermark=0.0)
    choices = run(e, prompt_of(71), SamplingParams(max_tokens=5, temperature=1.0, seed=2, n=3, ignore_eos=True))
    assert e.kv_fork_fallbacks == 1 and e.kv_forks == 0 and e.kv_fork_shared_tokens == 0
    assert all(len(c.output_ids) == 5 and c.forked_tokens == 0 for c in choices)
    assert e.bm.num_free == 3


def check_fork_off(make):
    e = make(kv_fork=False)
    choices = run(e, prompt_of(71), SamplingParams(max_tokens=5, temperature=1.0, seed=2, n=3, ignore_eos=True))
    assert e.kv_forks == 0 and e.kv_fork_fallbacks == 1 and e.runner.stats.get("kv_copy_launches", 0) == 0
    assert all(len(c.output_ids) == 5 and c.forked_tokens == 0 for c in choices)
    on = run(make(), prompt_of(71), SamplingParams(max_tokens=5, temperature=1.0, seed=2, n=3, ignore_eos=True))
    assert on[0].output_ids[0] == choices[0].output_ids[0]
    assert e.bm.num_free == e.bm.num_blocks


def check_abort(make):
    e = make()
    nb = e.bm.num_blocks
    sp = SamplingParams(max_tokens=30, temperature=1.0, seed=4, n=4, ignore_eos=True)
    s0 = e.add_request(prompt_of(71), sp, request_id="parked")   # aborted while the others are parked
    assert e.abort("parked") is s0
    assert all(c.is_finished() and c.finish_reason.value == "abort" for c in s0.choices)
    assert not e.has_unfinished() and e.bm.num_free == nb and not e.scheduler.parked
    s0 = e.add_request(prompt_of(71), sp, request_id="forked")   # aborted right after the fork: the
    step_until_forked(e, s0)                                      # others wait, owning blocks
    assert e.bm.num_free < nb - 3
    e.abort("forked")
    assert not e.has_unfinished() and e.bm.num_free == nb
    s0 = e.add_request(prompt_of(71), sp, request_id="running")  # aborted mid-flight
    other = e.add_request(prompt_of(40), SamplingParams(max_tokens=12, ignore_eos=True), request_id="other")
    for _ in range(5):
        e.step()
    e.abort("running")
    assert all(c.is_finished() for c in s0.choices) and not other.is_finished()
    drain(e)
    assert len(other.output_ids) == 12
    assert e.bm.num_free == nb and e.bm.num_seqs == 0 and not e.scheduler.groups and not e.scheduler.by_request


def check_preemption(make):
    """8 blocks: 3 of choice 0 + 3 private ones, and every choice needs a fourth at token 97: the
    youngest (forked) choices are preempted, recompute like any sequence, and still complete."""
    e = make(num_kv_blocks=8, watermark=0.0)
    choices = run(e, prompt_of(71), SamplingParams(max_tokens=40, temperature=1.0, seed=9, n=4, ignore_eos=True))
    assert e.kv_forks == 1 and e.scheduler.num_preemptions > 0
    assert any(c.num_preemptions > 0 and c.forked_tokens for c in choices[1:])
    assert all(len(c.output_ids) == 40 for c in choices)
    assert e.bm.num_free == 8 and e.bm.num_seqs == 0


# ------------------------------------------------------ prompts whose last token is a decode row
def step_at_most(e, n):
    """Step until nothing is left, ``n`` times at the most (a request that never ends must fail, not hang)."""
    for _ in range(n):
        if not e.has_unfinished():
            return
        e.step()
    raise AssertionError(f"still unfinished after {n} steps: parked {e.scheduler.parked}")


def check_short_and_chunk_tail_prompts(make):
    """A prompt's last token runs as a decode row when exactly one token is pending: a one-token prompt
    (nothing to fork: the choices fall back), and a chunked prefill whose last chunk is one token (a fork
    like any other).  P = 2 is the smallest prompt that forks."""
    e = make()
    nb = e.bm.num_blocks
    sp = dict(max_tokens=3, temperature=1.0, seed=6, ignore_eos=True)
    s0 = e.add_request(prompt_of(1), SamplingParams(n=3, **sp))
    step_at_most(e, 20)
    assert all(len(c.output_ids) == 3 and c.forked_tokens == 0 for c in s0.choices)
    assert e.kv_forks == 0 and e.kv_fork_fallbacks == 1 and not e.scheduler.parked
    s0 = e.add_request(prompt_of(2), SamplingParams(n=3, **sp))
    step_at_most(e, 20)
    assert all(len(c.output_ids) == 3 for c in s0.choices) and [c.forked_tokens for c in s0.choices] == [0, 1, 1]
    assert e.kv_forks == 1 and e.bm.num_free == nb and not e.scheduler.by_request
    e = make(max_num_batched_tokens=70)  # 71 tokens: a chunk of 70, then the last token as a decode row
    s0 = e.add_request(prompt_of(71), SamplingParams(n=3, **sp))
    e.step()
    assert s0.num_computed == 70 and s0.seq_id in e.scheduler.parked
    step_at_most(e, 20)
    assert all(len(c.output_ids) == 3 for c in s0.choices) and [c.forked_tokens for c in s0.choices] == [0, 70, 70]
    assert e.kv_forks == 1 and e.kv_fork_fallbacks == 0 and e.bm.num_free == e.bm.num_blocks
