"""Micro-benchmark of the weight-only FP8 (W8) decode GEMM against the bf16 packed kernel of the
same build, on the Llama-3 8B and 70B projection shapes with cold weights, plus the prefill
path's widen / column-scale overhead, the kernel / wide-path crossover, and the logit drift of a
W8 tiny model against its bf16 twin.  Needs a GPU; writes a markdown report (``--out``).

Cold weights: each shape rotates over enough copies (> 1 GiB per dtype) that nothing is served
from the 256 MiB Infinity Cache, as in a decode step where every layer's weights are cold.  The
two kernels are timed alternately (bf16, W8, bf16, W8, ...) and the median of the repeats is
reported, so drift of the shared machine hits both alike.  Times are device time: the launches of
one repeat are captured into a HIP graph once and the graph's replays are timed with device
events, so the host's cost of issuing a launch (about 10 us through these Python wrappers, more
than the small kernels take) is not in them.  Each launch is the op the decode chain
runs for that projection: split-K slabs for qkv / o / down (64-row n-blocks where the chain uses
them), the SiLU epilogue for gate_up.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from polykey_service_amd.ops import gemm, gemm_w8

SHAPES = {
    "8b": [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)],
    "70b": [("qkv", 10240, 8192), ("o", 8192, 8192), ("gate_up", 57344, 8192), ("down", 8192, 28672)],
}


REPLAYS = 5


def timeit(fn, n, iters):
    """us per call of ``fn`` (device time): ``iters`` calls captured into one graph, REPLAYS replays timed."""
    for i in range(3):
        fn(i % n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            fn(i % n)
    graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPLAYS):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    del graph
    return s.elapsed_time(e) / (iters * REPLAYS) * 1000.0  # us


def ab(fa, fb, n_a, n_b, iters, repeats):
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timeit(fa, n_a, iters))
        tb.append(timeit(fb, n_b, iters))
    return statistics.median(ta), statistics.median(tb), max(ta) - min(ta), max(tb) - min(tb)


def make_weights(N, K, copies_bf16, copies_w8):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    bf, w8 = [], []
    for _ in range(copies_bf16):
        w = (torch.randn((N, K), device="cuda", generator=g) * 0.02).to(torch.bfloat16)
        bf.append(gemm.pack_weight(w))
        del w
    for _ in range(copies_w8):
        w = (torch.randn((N, K), device="cuda", generator=g) * 0.02).to(torch.bfloat16)
        w8.append(gemm_w8.W8.from_weight(w))
        del w
    return bf, w8


def ops_for(name, x, ws, meta, bf, w8, M):
    """(bf16 launch, W8 launch) of projection ``name`` as the decode chain runs it."""
    if name == "gate_up":
        return (lambda i: gemm.linear_silu(x, meta, packed=bf[i], max_m=gemm.DECODE_MAX_M),
                lambda i: gemm_w8.linear_silu(x, w8[i]))
    if name == "down":
        return lambda i: gemm.linear_down(x, meta, ws, bf[i]), lambda i: gemm_w8.linear_down(x, w8[i], ws)
    half = M <= gemm.SKINNY_MAX_M
    return (lambda i: gemm.linear_partial(x, meta, ws, packed=bf[i], half=half),
            lambda i: gemm_w8.linear_partial(x, w8[i], ws, half=half))


def kernel_table(models, rows, iters, repeats, out):
    out.append("## Kernel: W8 vs bf16 packed, cold weights\n")
    out.append("Device microseconds per launch (median of %d alternating repeats; a repeat is %d replays of a "
               "captured graph of %d launches; `+-` is max - min of the repeats).  TB/s = weight bytes streamed / "
               "time.\n" % (repeats, REPLAYS, iters))
    out.append("| model | proj | N | K | M | bf16 us | +- | bf16 TB/s | W8 us | +- | W8 TB/s | bf16 / W8 |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|")
    ws = torch.empty(16 * 256 * 57344 // 2, dtype=torch.float32, device="cuda")
    for model in models:
        for name, N, K in SHAPES[model]:
            nb = max(2, (1 << 30) // (2 * N * K) + 1)
            n8 = max(2, (1 << 30) // (N * K) + 1)
            bf, w8 = make_weights(N, K, nb, n8)
            meta = torch.empty((N, K), dtype=torch.bfloat16, device="meta")
            for M in rows:
                x = torch.randn((M, K), device="cuda").to(torch.bfloat16)
                fa, fb = ops_for(name, x, ws, meta, bf, w8, M)
                ta, tb, sa, sb = ab(fa, fb, nb, n8, iters, repeats)
                out.append(f"| {model} | {name} | {N} | {K} | {M} | {ta:.1f} | {sa:.1f} | {2 * N * K / ta / 1e6:.2f} | "
                           f"{tb:.1f} | {sb:.1f} | {N * K / tb / 1e6:.2f} | {ta / tb:.2f} |")
                print(out[-1], flush=True)
            del bf, w8
            torch.cuda.empty_cache()
    out.append("")


def wide_table(models, iters, repeats, out, rows=(256, 512, 1024, 2048, 8192)):
    out.append("## Prefill path: widen + column scale, and the kernel / wide-path crossover\n")
    out.append("`widen` is once per projection per step; `col_scale` and `mm` (the library GEMM on the widened "
               "scratch) depend on the rows M.  `kernel` is the W8 decode GEMM (bf16 out) at the same M where it "
               "takes it (the ops send M > %d to the wide path).\n" % gemm_w8.KERNEL_MAX_M)
    out.append("| model | proj | M | widen us | mm us | col_scale us | wide total us | kernel us |")
    out.append("|---|---|---|---|---|---|---|---|")
    for model in models:
        for name, N, K in SHAPES[model]:
            g = torch.Generator(device="cuda").manual_seed(N + K)
            h = gemm_w8.W8.from_weight((torch.randn((N, K), device="cuda", generator=g) * 0.02).to(torch.bfloat16))
            scratch = torch.empty(N * K, dtype=torch.bfloat16, device="cuda")
            tw = statistics.median(timeit(lambda i: gemm_w8.widen(h, scratch), 1, iters) for _ in range(repeats))
            wb = gemm_w8.widen(h, scratch)
            for M in rows:
                x = torch.randn((M, K), device="cuda").to(torch.bfloat16)
                y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
                tm = statistics.median(timeit(lambda i: torch.mm(x, wb.t(), out=y), 1, iters) for _ in range(repeats))
                tc = statistics.median(timeit(lambda i: gemm_w8.col_scale(y, h.scale), 1, iters) for _ in range(repeats))
                tk = "-"
                if M <= gemm_w8.KERNEL_MAX_M:
                    tk = "%.1f" % statistics.median(
                        timeit(lambda i: gemm_w8._launch(gemm.MODE_BF16, x, h, 1, out=y), 1, iters) for _ in range(repeats))
                out.append(f"| {model} | {name} | {M} | {tw:.1f} | {tm:.1f} | {tc:.1f} | {tw + tm + tc:.1f} | {tk} |")
                print(out[-1], flush=True)
            del h, wb
            torch.cuda.empty_cache()
    out.append("")


def drift(out, names=("tiny-llama", "tiny-llama-gqa4", "small-llama")):
    """rms(logits_W8 - logits_bf16) / rms(logits_bf16) of the first decode position of one prompt."""
    import copy

    from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from polykey_service_amd.models import build_model, get_config
    from polykey_service_amd.parallel.state import ParallelState
    out.append("## Logit drift: W8 model against its bf16 twin (random-init weights)\n")
    out.append("| model | layers | rms(diff) / rms(logits) | same greedy token |")
    out.append("|---|---|---|---|")
    dev = torch.device("cuda")
    for name in names:
        cfg = get_config(name)
        base = build_model(cfg, ParallelState(device=dev), torch.bfloat16, dev).init_random(3)
        logits = {}
        for wd in ("bf16", "fp8"):
            e = LLMEngine(EngineConfig(model=name, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=512,
                                       hip_graphs=False, device="cuda", weight_dtype=wd),
                          ParallelState(device=dev), model=copy.deepcopy(base))
            e.runner.keep_logits = True
            e.generate([[1] + list(range(40, 90))], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
            logits[wd] = e.runner.last_logits.float().clone()
            del e
        d = logits["fp8"] - logits["bf16"]
        r = float(d.pow(2).mean().sqrt() / logits["bf16"].pow(2).mean().sqrt())
        out.append(f"| {name} | {cfg.num_layers} | {r:.4f} | {int(logits['fp8'].argmax()) == int(logits['bf16'].argmax())} |")
        print(out[-1], flush=True)
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b,70b")
    ap.add_argument("--rows", default="1,16,64,256")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of: kernel, wide, drift")
    ap.add_argument("--out", default="profiles/w8_gemm.md")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gemm_w8.py measures on a GPU"
    models = [m for m in a.models.split(",") if m]
    rows = [int(r) for r in a.rows.split(",")]
    skip = set(a.skip.split(","))
    out = ["# W8 (weight-only FP8) projections: measurements\n",
           f"Command: `python tools/bench_gemm_w8.py --models {a.models} --rows {a.rows} --iters {a.iters} "
           f"--repeats {a.repeats}` on {torch.cuda.get_device_name(0)}.\n"]
    if "kernel" not in skip:
        kernel_table(models, rows, a.iters, a.repeats, out)
    if "wide" not in skip:
        wide_table(models, max(10, a.iters // 3), a.repeats, out)
    if "drift" not in skip:
        drift(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
