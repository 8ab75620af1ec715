"""Prompt logprobs: the kernel next to pk_logprobs, and the time to first token of a scored prompt.

``kernel``: 256 rows x V = 128,256 bf16 logits (one LM-head chunk of the runner), every row at the same
``n_top`` (0 / 1 / 20), ``pk_prompt_logprobs`` against ``pk_logprobs`` of the same build on the same
rows with ``tokens = targets``.  Device-event times per call (graph replays of back-to-back calls, as
tools/bench_logprobs.py), ``--repeats`` runs each, min / median / max printed, plus the bytes a row
costs (V x 2 per pass) and the rate the n_top = 0 form achieves over its two passes.

``step``: Llama-3-8B shapes, random-init weights, one request at a time: device time (events) from the
first step to the step that yields the first token, with ``prompt_logprobs`` off / 0 / 20, for prompts
of 512 / 4096 / 8192 tokens, next to the LM-head FLOPs and logits bytes the extra work needs
(computed from the shapes).  ``--layers`` keeps only that many decoder layers (the extra work does
not depend on the depth).

Prints markdown tables (profiles/prompt_logprobs.md).

Usage: ``python tools/bench_prompt_logprobs.py kernel [--rows 256] [--vocab 128256] [--repeats 5]``
       ``python tools/bench_prompt_logprobs.py step [--prompts 512,4096,8192] [--repeats 3] [--layers 0]``
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.ops import sampler  # noqa: E402

CALLS_PER_GRAPH = 10


def timed(fn, iters):
    """us per call from device events around replays of a graph of CALLS_PER_GRAPH back-to-back calls."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS_PER_GRAPH):
            fn()
    reps = max(1, iters // CALLS_PER_GRAPH)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (reps * CALLS_PER_GRAPH)


def spread(xs):
    return f"{min(xs):.1f} / {statistics.median(xs):.1f} / {max(xs):.1f}"


def kernel(a):
    R, V = a.rows, a.vocab
    torch.manual_seed(0)
    x = (torch.randn(R, V, device="cuda") * 3).to(torch.bfloat16)
    targets = torch.randint(0, V, (R,), dtype=torch.int32, device="cuda")
    out_p = torch.zeros((R, sampler.PROMPT_LOGPROB_WORDS), dtype=torch.int32, device="cuda")
    out_l = torch.zeros((R, sampler.LOGPROB_WORDS), dtype=torch.int32, device="cuda")
    row_bytes = V * 2
    print(f"R = {R}, V = {V}, bf16 logits ({R * row_bytes / 1e6:.1f} MB, {row_bytes} bytes per row and pass), "
          f"{a.iters} calls per run (graphs of {CALLS_PER_GRAPH}), {a.repeats} runs, device events\n")
    print("| n_top | pk_logprobs us / call (min / median / max) | pk_prompt_logprobs us / call (min / median / max) | "
          "median ratio |\n|---|---|---|---|")
    med0 = None
    for n in (0, 1, 20):
        nt = torch.full((R,), n, dtype=torch.int32, device="cuda")
        base, new = [], []
        for _ in range(a.repeats):  # alternate, so that drift hits both alike
            base.append(timed(lambda: sampler.logprobs(x, targets, nt, out_l), a.iters))
            new.append(timed(lambda: sampler.prompt_logprobs(x, targets, nt, out_p), a.iters))
        if n == 0:
            med0 = statistics.median(new)
        print(f"| {n} | {spread(base)} | {spread(new)} | {statistics.median(new) / statistics.median(base):.3f} |")
    print(f"\nn_top = 0 reads every row twice: {2 * R * row_bytes / 1e6:.1f} MB per call, "
          f"{2 * R * row_bytes / (med0 * 1e-6) / 1e12:.2f} TB/s at the median (the second pass is served from L2 / "
          f"MALL where the row still is there)")


def step(a):
    from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from polykey_service_amd.parallel.state import ParallelState
    prompts = [int(p) for p in a.prompts.split(",")]
    budget = max(prompts)
    e = LLMEngine(EngineConfig(model="llama3-8b", max_num_seqs=8, max_num_batched_tokens=budget,
                               max_model_len=budget + 64, hip_graphs=False, device="cuda:0", num_layers=a.layers,
                               num_kv_blocks=(budget + 64) // 32 * 2 + 16, prefix_caching=False),
                  ParallelState(device=torch.device("cuda:0")))
    V, H = e.mcfg.vocab_size, e.mcfg.hidden_size
    g = torch.Generator().manual_seed(1)

    def ttft(P, n):
        ids = torch.randint(3, V, (P,), generator=g).tolist()
        e.add_request(ids, SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=n))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        while e.has_unfinished():
            e.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    print(f"llama3-8b shapes, random-init, {len(e.model.layers)} layers, one request at a time, one prefill chunk, "
          f"{a.repeats} runs after one warm run per shape, device events\n")
    print("| prompt | off ms (min / median / max) | prompt_logprobs = 0 ms | prompt_logprobs = 20 ms | "
          "extra LM-head GFLOP | logits bytes written + read (n = 0) |\n|---|---|---|---|---|---|")
    for P in prompts:
        res = {}
        for n in (None, 0, 20):
            ttft(P, n)  # warm the shape
        for _ in range(a.repeats):
            for n in (None, 0, 20):
                res.setdefault(n, []).append(ttft(P, n))
        flop = 2.0 * (P - 1) * H * V / 1e9
        lbytes = (P - 1) * V * 2 * 3  # written once by the GEMM, read twice by the kernel
        print(f"| {P} | {spread(res[None])} | {spread(res[0])} | {spread(res[20])} | {flop:.0f} | {lbytes / 1e6:.0f} MB |")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rows", type=int, default=256)
    k.add_argument("--vocab", type=int, default=128256)
    k.add_argument("--iters", type=int, default=200)
    k.add_argument("--repeats", type=int, default=5)
    s = sub.add_parser("step")
    s.add_argument("--prompts", default="512,4096,8192")
    s.add_argument("--repeats", type=int, default=3)
    s.add_argument("--layers", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernel": kernel, "step": step}[a.cmd](a)


if __name__ == "__main__":
    main()
