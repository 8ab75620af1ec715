"""Micro-benchmark of the weight-only MXFP4 (W4) decode GEMM against the W8 and the bf16 packed
kernels of the same build, on the Llama-3 8B and 70B projection shapes with cold weights, plus the
prefill path's widen overhead, the kernel / wide-path crossover, and the logit drift of W4 and W8
tiny models against their bf16 twin.  Needs a GPU; writes a markdown report (``--out``).

Cold weights: each shape rotates over enough copies (> 1 GiB per format) that nothing is served
from the 256 MiB Infinity Cache, as in a decode step where every layer's weights are cold.  The
three kernels are timed alternately (bf16, W8, W4, bf16, ...) and the median of the repeats is
reported, so drift of the shared machine hits all alike.  Times are device time: the launches of
one repeat are captured into a HIP graph once and the graph's replays are timed with device
events, so the host's cost of issuing a launch is not in them.  Each launch is the op the decode
chain runs for that projection: split-K slabs for qkv / o / down (64-row n-blocks where the chain
uses them), the SiLU epilogue for gate_up.  The quantised copies hold random bytes (every nibble,
scale bytes 119..126; every finite e4m3 byte): the kernels' time does not depend on the values.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from polykey_service_amd.ops import gemm, gemm_w4, gemm_w8

SHAPES = {
    "8b": [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)],
    "70b": [("qkv", 10240, 8192), ("o", 8192, 8192), ("gate_up", 57344, 8192), ("down", 8192, 28672)],
}
REPLAYS = 5
FORMATS = ("bf16", "w8", "w4")
BYTES = {"bf16": 2.0, "w8": 1.0, "w4": 0.5 + 1.0 / 32}  # per weight, scales included


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


def make_weights(N, K):
    """{format: copies}, each format more than 1 GiB in all."""
    g = torch.Generator(device="cuda").manual_seed(N + K)
    out = {f: [] for f in FORMATS}
    for _ in range(max(2, (1 << 30) // (2 * N * K) + 1)):
        out["bf16"].append(gemm.pack_weight((torch.randn((N, K), device="cuda", generator=g) * 0.02).to(torch.bfloat16)))
    ones = torch.ones(N, device="cuda")
    for _ in range(max(2, (1 << 30) // (N * K) + 1)):
        b = torch.randint(0, 256, (N, K), device="cuda", generator=g, dtype=torch.uint8)
        b = torch.where((b & 0x7F) == 0x7F, b & 0x80, b)  # no NaN encodings
        out["w8"].append(gemm_w8.W8.from_bytes(b, ones))
    for _ in range(max(2, (1 << 30) // (N * K // 2) + 1)):
        nib = torch.randint(0, 256, (N, K // 2), device="cuda", generator=g, dtype=torch.uint8)
        xs = torch.randint(119, 127, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8)
        out["w4"].append(gemm_w4.W4.from_bytes(nib, xs))
    return out


def ops_for(name, x, ws, meta, w, M):
    """{format: launch} of projection ``name`` as the decode chain runs it."""
    if name == "gate_up":
        return {"bf16": lambda i: gemm.linear_silu(x, meta, packed=w["bf16"][i], max_m=gemm.DECODE_MAX_M),
                "w8": lambda i: gemm_w8.linear_silu(x, w["w8"][i]), "w4": lambda i: gemm_w4.linear_silu(x, w["w4"][i])}
    if name == "down":
        return {"bf16": lambda i: gemm.linear_down(x, meta, ws, w["bf16"][i]),
                "w8": lambda i: gemm_w8.linear_down(x, w["w8"][i], ws), "w4": lambda i: gemm_w4.linear_down(x, w["w4"][i], ws)}
    half = M <= gemm.SKINNY_MAX_M
    return {"bf16": lambda i: gemm.linear_partial(x, meta, ws, packed=w["bf16"][i], half=half),
            "w8": lambda i: gemm_w8.linear_partial(x, w["w8"][i], ws, half=half),
            "w4": lambda i: gemm_w4.linear_partial(x, w["w4"][i], ws, half=half)}


def kernel_table(models, rows, iters, repeats, out):
    out.append("## Kernel: W4 vs W8 vs bf16 packed, cold weights\n")
    out.append("Device microseconds per launch (median of %d alternating repeats; a repeat is %d replays of a "
               "captured graph of %d launches; `+-` is max - min of the repeats).  TB/s = weight bytes streamed "
               "(scales included) / time.  A row is marked `slower` when W4 takes longer than W8 by more than the "
               "spread of the W8 repeats.\n" % (repeats, REPLAYS, iters))
    out.append("| model | proj | N | K | M | bf16 us | +- | W8 us | +- | W4 us | +- | W4 TB/s | W8 / W4 | bf16 / W4 | |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ws = torch.empty(16 * 256 * 57344 // 2, dtype=torch.float32, device="cuda")
    for model in models:
        for name, N, K in SHAPES[model]:
            w = make_weights(N, K)
            meta = torch.empty((N, K), dtype=torch.bfloat16, device="meta")
            for M in rows:
                x = torch.randn((M, K), device="cuda").to(torch.bfloat16)
                fns = ops_for(name, x, ws, meta, w, M)
                t = {f: [] for f in FORMATS}
                for _ in range(repeats):
                    for f in FORMATS:
                        t[f].append(timeit(fns[f], len(w[f]), iters))
                med = {f: statistics.median(t[f]) for f in FORMATS}
                spr = {f: max(t[f]) - min(t[f]) for f in FORMATS}
                mark = "slower" if med["w4"] - med["w8"] > spr["w8"] else ""
                out.append(f"| {model} | {name} | {N} | {K} | {M} | {med['bf16']:.1f} | {spr['bf16']:.1f} | "
                           f"{med['w8']:.1f} | {spr['w8']:.1f} | {med['w4']:.1f} | {spr['w4']:.1f} | "
                           f"{BYTES['w4'] * N * K / med['w4'] / 1e6:.2f} | {med['w8'] / med['w4']:.2f} | "
                           f"{med['bf16'] / med['w4']:.2f} | {mark} |")
                print(out[-1], flush=True)
            del w
            torch.cuda.empty_cache()
    out.append("")


def wide_table(models, iters, repeats, out, rows=(256, 512, 1024, 8192)):
    out.append("## Prefill path: widen, and the kernel / wide-path crossover\n")
    out.append("`widen` is once per projection per step; `mm` (the library GEMM on the widened scratch) depends on "
               "the rows M.  `kernel` is the W4 decode GEMM (bf16 out) at the same M where it takes it (the ops send "
               "M > %d to the wide path).\n" % gemm_w4.KERNEL_MAX_M)
    out.append("| model | proj | M | widen us | mm us | wide total us | kernel us |")
    out.append("|---|---|---|---|---|---|---|")
    for model in models:
        for name, N, K in SHAPES[model]:
            g = torch.Generator(device="cuda").manual_seed(N + K)
            h = gemm_w4.W4.from_bytes(torch.randint(0, 256, (N, K // 2), device="cuda", generator=g, dtype=torch.uint8),
                                      torch.randint(119, 127, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8))
            scratch = torch.empty(N * K, dtype=torch.bfloat16, device="cuda")
            tw = statistics.median(timeit(lambda i: gemm_w4.widen(h, scratch), 1, iters) for _ in range(repeats))
            wb = gemm_w4.widen(h, scratch)
            for M in rows:
                x = torch.randn((M, K), device="cuda").to(torch.bfloat16)
                y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
                tm = statistics.median(timeit(lambda i: torch.mm(x, wb.t(), out=y), 1, iters) for _ in range(repeats))
                tk = "-"
                if M <= gemm_w4.KERNEL_MAX_M:
                    tk = "%.1f" % statistics.median(
                        timeit(lambda i: gemm_w4._launch(gemm.MODE_BF16, x, h, 1, out=y), 1, iters) for _ in range(repeats))
                out.append(f"| {model} | {name} | {M} | {tw:.1f} | {tm:.1f} | {tw + tm:.1f} | {tk} |")
                print(out[-1], flush=True)
            del h, wb
            torch.cuda.empty_cache()
    out.append("")


def drift(out, names=("tiny-llama", "tiny-llama-gqa4", "small-llama")):
    """rms(logits_q - logits_bf16) / rms(logits_bf16) of the first decode position of one prompt."""
    import copy

    from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from polykey_service_amd.models import build_model, get_config
    from polykey_service_amd.parallel.state import ParallelState
    out.append("## Logit drift: W8 and W4 models against their bf16 twin (random-init weights)\n")
    out.append("| model | layers | fp8: rms(diff) / rms(logits) | mxfp4: rms(diff) / rms(logits) | mxfp4: max abs diff / rms | "
               "same greedy token (fp8, mxfp4) |")
    out.append("|---|---|---|---|---|---|")
    dev = torch.device("cuda")
    for name in names:
        cfg = get_config(name)
        base = build_model(cfg, ParallelState(device=dev), torch.bfloat16, dev).init_random(3)
        logits = {}
        for wd in ("bf16", "fp8", "mxfp4"):
            e = LLMEngine(EngineConfig(model=name, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=512,
                                       hip_graphs=False, device="cuda", weight_dtype=wd),
                          ParallelState(device=dev), model=copy.deepcopy(base))
            e.runner.keep_logits = True
            e.generate([[1] + list(range(40, 90))], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
            logits[wd] = e.runner.last_logits.float().clone()
            del e
        rms = float(logits["bf16"].pow(2).mean().sqrt())
        r = {wd: float((logits[wd] - logits["bf16"]).pow(2).mean().sqrt()) / rms for wd in ("fp8", "mxfp4")}
        mx = float((logits["mxfp4"] - logits["bf16"]).abs().max()) / rms
        same = tuple(int(logits[wd].argmax()) == int(logits["bf16"].argmax()) for wd in ("fp8", "mxfp4"))
        out.append(f"| {name} | {cfg.num_layers} | {r['fp8']:.4f} | {r['mxfp4']:.4f} | {mx:.3f} | {same} |")
        print(out[-1], flush=True)
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b,70b")
    ap.add_argument("--rows", default="1,16,64,256,512")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of: kernel, wide, drift")
    ap.add_argument("--out", default="profiles/w4_gemm.md")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gemm_w4.py measures on a GPU"
    models = [m for m in a.models.split(",") if m]
    rows = [int(r) for r in a.rows.split(",")]
    skip = set(a.skip.split(","))
    out = ["# W4 (weight-only MXFP4) projections: measurements\n",
           f"Command: `python tools/bench_gemm_w4.py --models {a.models} --rows {a.rows} --iters {a.iters} "
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
