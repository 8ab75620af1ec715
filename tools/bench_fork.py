"""Parallel sampling (n > 1): what the KV fork costs and saves on one GPU (Llama-3-8B shapes, random init).

Two measurements, written as a markdown report (default ``profiles/kv_fork.md``):

* ``copy``: device time (events on the stream, no graph, a synchronise at the end of each window) of one
  ``pk_kv_copy_blocks`` launch for 1, 7 and 15 (src, dst) pairs on caches of the model's shape, against
  the same copy done as ``2 x layers`` ``copy_`` calls per pair.
* ``e2e``: an ``n = 4, 8, 16`` request on 512- and 4096-token prompts, fork on against fork off
  (``kv_fork=False``, what ``POLYKEY_KV_FORK=0`` selects) on the same weights: wall time from
  ``add_request`` to the step that gave the last choice its first token (a host clock around steps that
  end in the read-back of their tokens), and output tokens per second of the whole request.

    python tools/bench_fork.py [--model llama3-8b] [--layers 0] [--n 4,8,16] [--prompts 512,4096] [--out FILE]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams  # noqa: E402
from polykey_service_amd.models import get_config  # noqa: E402
from polykey_service_amd.ops import kv as kv_ops  # noqa: E402
from polykey_service_amd.parallel.state import ParallelState  # noqa: E402


def event_us(fn, reps=50, windows=7):
    """Device microseconds per call of ``fn`` over ``windows`` windows of ``reps`` calls (3 warm-up calls)
    -> (median, min, max)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) / reps * 1000)
    got.sort()
    return got[len(got) // 2], got[0], got[-1]


def bench_copy(mcfg, layers, bs=32, num_blocks=64):
    dev = torch.device("cuda")
    hd = mcfg.hidden_size // mcfg.num_heads
    caches = [(torch.randn((num_blocks, mcfg.num_kv_heads, bs, hd), device=dev).to(torch.bfloat16),
               torch.randn((num_blocks, mcfg.num_kv_heads, hd, bs), device=dev).to(torch.bfloat16))
              for _ in range(layers)]
    table = kv_ops.pointer_table(caches)
    bb = kv_ops.block_bytes(caches)
    rows = []
    for n_pairs in (1, 7, 15):
        pairs = [(0, 1 + i) for i in range(n_pairs)]

        def tensor_copies():
            for k, v in caches:
                for s, d in pairs:
                    k[d].copy_(k[s])
                    v[d].copy_(v[s])
        t_kernel = event_us(lambda: kv_ops.copy_blocks(caches, pairs, table))
        t_copies = event_us(tensor_copies, reps=20)
        moved = 2 * layers * n_pairs * bb  # bytes written (as many read)
        rows.append((n_pairs, 2 * layers * n_pairs, moved, t_kernel, t_copies))
    return bb, rows


def request(e, prompt, n, max_tokens):
    """-> (seconds to the last choice's first token, output tokens / s, forks, fallbacks)."""
    # (wall clock around steps that end in the read-back of their tokens)
    f0, b0 = e.kv_forks, e.kv_fork_fallbacks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s0 = e.add_request(prompt, SamplingParams(max_tokens=max_tokens, temperature=1.0, seed=1, n=n, ignore_eos=True))
    t_first = None
    while e.has_unfinished():
        e.step()
        if t_first is None and all(c.output_ids for c in s0.choices):
            t_first = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e.bm.reset_prefix_cache()  # the next request prefills its prompt again
    return t_first, sum(len(c.output_ids) for c in s0.choices) / dt, e.kv_forks - f0, e.kv_fork_fallbacks - b0


def bench_e2e(args, ns, prompt_lens, max_tokens=64):
    dev = torch.device("cuda")
    rows = []
    model = None
    for fork in (True, False):
        e = LLMEngine(EngineConfig(model=args.model, num_layers=args.layers, max_num_seqs=16,
                                   max_num_batched_tokens=8192, max_model_len=8192, device="cuda", kv_fork=fork,
                                   graph_batch_sizes=(1, 2, 4, 8, 16)), ParallelState(device=dev), model=model)
        model = e.model  # the same weights for both engines
        vocab = e.mcfg.vocab_size
        g = torch.Generator().manual_seed(7)
        for P in prompt_lens:
            prompt = [1] + torch.randint(3, vocab, (P - 1,), generator=g).tolist()
            for n in ns:
                request(e, prompt, n, 4)  # warm-up of every shape of the timed request
                runs = sorted(request(e, prompt, n, max_tokens) for _ in range(5))
                med = runs[2]
                rows.append((fork, P, n, med[0], runs[0][0], runs[-1][0], sorted(r[1] for r in runs)[2], med[2], med[3]))
        del e
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=0, help="> 0: keep only that many layers")
    ap.add_argument("--n", default="4,8,16")
    ap.add_argument("--prompts", default="512,4096")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "kv_fork.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fork.py measures on a GPU; none found")
    mcfg = get_config(args.model)
    layers = args.layers or mcfg.num_layers
    lines = [f"# KV fork (parallel sampling): {args.model}, {layers} layers, {torch.cuda.get_device_name(0)}", ""]
    bb, rows = bench_copy(mcfg, layers)
    lines += [f"## Copy launch (bf16 caches, {bb} bytes per block and tensor; device time, stream events, no graph)", "",
              "Median of 7 windows (min - max).", "",
              "| pairs | tensor copies replaced | bytes written | pk_kv_copy_blocks us | copy_ calls us | GB/s written |",
              "|---|---|---|---|---|---|"]
    for n_pairs, n_copies, moved, tk, tc in rows:
        lines.append(f"| {n_pairs} | {n_copies} | {moved} | {tk[0]:.1f} ({tk[1]:.1f} - {tk[2]:.1f}) | "
                     f"{tc[0]:.1f} ({tc[1]:.1f} - {tc[2]:.1f}) | {moved / tk[0] / 1e3:.0f} |")
    if not args.skip_e2e:
        ns = [int(x) for x in args.n.split(",")]
        pls = [int(x) for x in args.prompts.split(",")]
        lines += ["", "## One request with n choices, 64 tokens each (median of 5 runs, min - max)", "",
                  "| fork | prompt | n | last first token ms | output tokens/s | forks | fallbacks |", "|---|---|---|---|---|---|---|"]
        for fork, P, n, t_med, t_min, t_max, tps, forks, fb in bench_e2e(args, ns, pls):
            lines.append(f"| {'on' if fork else 'off'} | {P} | {n} | {t_med * 1e3:.1f} ({t_min * 1e3:.1f} - "
                         f"{t_max * 1e3:.1f}) | {tps:.0f} | {forks} | {fb} |")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
