"""Per-token logprobs end to end on the GPU: the kernel inside the decode graphs and the pipelined
continuations, next to requests that did not ask for them."""
import copy

import pytest
import torch

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
from polykey_service_amd.models import build_model, get_config
from polykey_service_amd.ops import reference as ref
from polykey_service_amd.ops import sampler
from polykey_service_amd.parallel.state import ParallelState

pytestmark = pytest.mark.gpu

MODEL = "tiny-llama"
PROMPTS = [[1] + list(range(5, 5 + n)) for n in (3, 17, 40, 9, 6)]
# (logprobs, temperature): None / 0 / 3 mixed with greedy and seeded sampling
ASKS = [(None, 0.0), (0, 0.0), (3, 0.0), (3, 0.8), (None, 1.0)]
ATOL = 1e-4


@pytest.fixture(scope="module")
def gpu_model():
    cpu = build_model(get_config(MODEL), ParallelState(), torch.bfloat16, torch.device("cpu")).init_random(3)
    gpu = copy.deepcopy(cpu).to("cuda")
    gpu.device = torch.device("cuda")
    return gpu


def _engine(model, graphs, overlap):
    return LLMEngine(EngineConfig(model=MODEL, max_num_seqs=8, max_num_batched_tokens=256, max_model_len=512,
                                  hip_graphs=graphs, device="cuda", overlap=overlap),
                     ParallelState(device=torch.device("cuda")), model=model)


def _params(asks, max_tokens=12):
    return [SamplingParams(max_tokens=max_tokens + i, temperature=t, seed=7, ignore_eos=True, logprobs=lp)
            for i, (lp, t) in enumerate(asks)]


def _run(e, asks):
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(asks))]
    while e.has_unfinished():
        e.step()
    return seqs


@pytest.fixture(scope="module")
def runs(gpu_model):
    """Each engine configuration once; the tests share the results."""
    graphed = _engine(gpu_model, graphs=True, overlap=True)
    with_lp = _run(graphed, ASKS)
    cont = graphed.continuation_steps
    graph_steps = graphed.runner.stats["graph_steps"]
    without = _run(_engine(gpu_model, graphs=True, overlap=True), [(None, t) for _, t in ASKS])
    eager = _run(_engine(gpu_model, graphs=False, overlap=False), ASKS)
    return {"with": with_lp, "without": without, "eager": eager, "cont": cont, "graph_steps": graph_steps}


def test_token_ids_do_not_depend_on_logprobs(runs):
    assert [s.output_ids for s in runs["with"]] == [s.output_ids for s in runs["without"]]
    assert all(s.logprobs is None for s in runs["without"])


def test_one_entry_per_token_with_graphs_and_continuations(runs):
    assert runs["cont"] > 0 and runs["graph_steps"] > 0
    for s, (lp, t) in zip(runs["with"], ASKS):
        if lp is None:
            assert s.logprobs is None
            continue
        assert len(s.logprobs) == len(s.output_ids) > 0
        for tok, (v, top) in zip(s.output_ids, s.logprobs):
            assert v <= 0.0 and len(top) == lp
            assert [x for _, x in top] == sorted((x for _, x in top), reverse=True)
            if t == 0.0 and lp:  # greedy: the sampled token heads its own top list
                assert top[0] == (tok, v)


def test_graph_and_eager_engines_return_identical_logprobs(runs):
    assert [s.output_ids for s in runs["with"]] == [s.output_ids for s in runs["eager"]]
    assert [s.logprobs for s in runs["with"]] == [s.logprobs for s in runs["eager"]]


def test_each_step_matches_the_reference_on_the_step_logits(gpu_model, monkeypatch):
    """Graphs on, overlap off, POLYKEY_DEBUG_LOGITS=1 (every step's logits are kept, graphed steps
    included): each returned entry equals the float64 reference on that step's logits."""
    monkeypatch.setenv("POLYKEY_DEBUG_LOGITS", "1")
    e = _engine(gpu_model, graphs=True, overlap=False)
    assert e.runner.debug_logits
    seqs = [e.add_request(p, sp) for p, sp in zip(PROMPTS, _params(ASKS, max_tokens=5))]
    by_id = {s.request_id: s for s in seqs}
    checked = 0
    while e.has_unfinished():
        outs = e.step()
        logits = e.runner.last_logits.float().cpu()
        # rows of this step = its sampling sequences in order = the order of the outputs
        assert len(outs) <= logits.shape[0]
        toks = torch.tensor([o.new_token_ids[0] for o in outs], dtype=torch.int32)
        n_top = torch.tensor([-1 if by_id[o.request_id].params.logprobs is None else by_id[o.request_id].params.logprobs
                              for o in outs], dtype=torch.int32)
        want = ref.logprobs(logits[:len(outs)], toks, n_top)
        for r, o in enumerate(outs):
            n = int(n_top[r])
            if n < 0:
                assert o.logprobs is None
                continue
            (lp, top), = o.logprobs
            wlp, wtop = sampler.logprob_entry(want[r].numpy(), n)
            assert abs(lp - wlp) <= ATOL
            assert [i for i, _ in top] == [i for i, _ in wtop]
            assert all(abs(a - b) <= ATOL for (_, a), (_, b) in zip(top, wtop))
            checked += 1
    assert e.runner.stats["graph_steps"] > 0 and checked >= 3 * 5
