"""Micro-benchmark of the multi-LoRA shrink / expand kernels and of the LoRA form of the engine's
steps.  Needs a GPU; writes a markdown report (``--out``).

(a) shrink + expand per projection on the Llama-3-8B shapes, rank 16 and 64 (stored padded to 64),
    1 / 16 / 64 / 256 rows, all rows on one adapter and 8 adapters mixed row by row;
(b) one decode step of an 8B-shaped model at 64 rows in three modes of ONE engine: the base graph,
    the LoRA-form graph with no adapter rows (every index -1) and with all rows on adapters;
(c) one 8,192-row prefill step with and without an adapter.

Times are device time: (a) and (b) replay captured graphs between device events; (c) is one eager
step between device events (milliseconds long: the host's launch cost is hidden behind it).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from polykey_service_amd.ops import lora as lora_ops

# (name, K, N, segments) of the 8B projections
SHAPES_8B = [("qkv", 4096, 6144, lora_ops.Segments(4096, 5120, 0)), ("o", 4096, 4096, None),
             ("gate_up", 4096, 28672, lora_ops.Segments(28672, 28672, 16)), ("down", 14336, 4096, None)]
SEG_R = 64
REPLAYS = 5


def timeit(fn, iters):
    """us per call of ``fn`` (device time): ``iters`` calls captured into one graph, REPLAYS replays timed."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return time_graph(graph) / iters


def time_graph(graph, replays=REPLAYS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / replays * 1000.0  # us


def kernel_table(rows, iters, repeats, out):
    out.append("## (a) shrink + expand per projection, Llama-3-8B shapes\n")
    out.append("Device microseconds per launch (median of %d repeats; a repeat is %d replays of a captured graph of "
               "%d launches).  8 resident slots, stored padded to rank 64; `one` = every row on slot 0, `mixed` = "
               "row m on slot m %% 8.  The expand adds into an fp32 slab (the decode chain's form).\n"
               % (repeats, REPLAYS, iters))
    out.append("| proj | K | N | rank | M | shrink one | shrink mixed | expand one | expand mixed | pair one | pair mixed |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|")
    S = 8
    for name, K, N, seg in SHAPES_8B:
        seg = seg or lora_ops.Segments.single(N)
        R = seg.count(N) * SEG_R
        A = (torch.randn((S, R, K), device="cuda") * K ** -0.5).to(torch.bfloat16)
        B = (torch.randn((S, N, SEG_R), device="cuda") * 0.02).to(torch.bfloat16)
        scale = torch.ones(S, dtype=torch.float32, device="cuda")
        for rank in (16, 64):
            ranks = torch.full((S,), rank, dtype=torch.int32, device="cuda")
            for M in rows:
                x = torch.randn((M, K), device="cuda").to(torch.bfloat16)
                t = torch.zeros(M * R, dtype=torch.bfloat16, device="cuda")
                slab = torch.zeros((M, N), dtype=torch.float32, device="cuda")
                res = {}
                for tag, idx in (("one", torch.zeros(M, dtype=torch.int32, device="cuda")),
                                 ("mixed", (torch.arange(M, device="cuda") % S).to(torch.int32))):
                    tv = lora_ops.shrink(x, A, idx, t, SEG_R, ranks=ranks)
                    med = lambda f: statistics.median(timeit(f, iters) for _ in range(repeats))
                    res[tag] = (med(lambda: lora_ops.shrink(x, A, idx, t, SEG_R, ranks=ranks)),
                                med(lambda: lora_ops.expand(slab, tv, B, scale, idx, seg, ranks=ranks)))
                out.append(f"| {name} | {K} | {N} | {rank} | {M} | {res['one'][0]:.1f} | {res['mixed'][0]:.1f} | "
                           f"{res['one'][1]:.1f} | {res['mixed'][1]:.1f} | {sum(res['one']):.1f} | "
                           f"{sum(res['mixed']):.1f} |")
                print(out[-1], flush=True)
        del A, B
        torch.cuda.empty_cache()
    out.append("")


def build_engine(layers, rank, max_tokens, graphs):
    from polykey_service_amd.engine import EngineConfig, LLMEngine
    from polykey_service_amd.models import get_config
    from polykey_service_amd.models.lora import LoraAdapter
    from polykey_service_amd.parallel.state import ParallelState
    import dataclasses
    cfg = dataclasses.replace(get_config("llama3-8b"), num_layers=layers)
    mods = tuple((f"a{i}", LoraAdapter.random(cfg, rank=rank, alpha=2 * rank, seed=i, b_std=0.01)) for i in range(8))
    dev = torch.device("cuda")
    return LLMEngine(EngineConfig(model="llama3-8b", num_layers=layers, max_num_seqs=64, max_num_batched_tokens=max_tokens,
                                  max_model_len=max_tokens, num_kv_blocks=2048, device="cuda", hip_graphs=graphs,
                                  graph_batch_sizes=(64,), lora_modules=mods), ParallelState(device=dev))


def step_table(layers, rank, out):
    out.append(f"## (b) decode step at 64 rows, Llama-3-8B shapes, {layers} layers, 8 adapters of rank {rank}\n")
    e = build_engine(layers, rank, 512, True)
    r = e.runner
    g = 64
    key = "short" if r.short_graphs else "long"
    base = (r.short_graphs or r.graphs)[g]
    lora = (r.lora_short_graphs or r.lora_graphs)[g]
    idx = r.d["lora_idx"]
    times = {"base": [], "lora_none": [], "lora_all": []}
    for _ in range(5):  # alternating
        times["base"].append(time_graph(base, 10))
        idx[:g] = -1
        times["lora_none"].append(time_graph(lora, 10))
        idx[:g] = (torch.arange(g, device="cuda") % 8).to(torch.int32)
        times["lora_all"].append(time_graph(lora, 10))
        idx[:g] = -1
    med = {k: statistics.median(v) for k, v in times.items()}
    out.append(f"Graph replays ({key}-context variant; the captured dummy state: context 1), device us per step, median "
               "of 5 alternating repeats of 10 replays (min .. max).  The step includes the LM head and the sampler.\n")
    out.append("| mode | us per step | min .. max | vs base |")
    out.append("|---|---|---|---|")
    for k, label in (("base", "base step of the LoRA-enabled engine"), ("lora_none", "LoRA form, no adapter rows (forced)"),
                     ("lora_all", "LoRA form, all 64 rows on 8 adapters")):
        out.append(f"| {label} | {med[k]:.0f} | {min(times[k]):.0f} .. {max(times[k]):.0f} | {med[k] / med['base']:.2f} |")
        print(out[-1], flush=True)
    out.append("")
    del e
    torch.cuda.empty_cache()


def prefill_table(layers, rank, out, T=8192):
    from polykey_service_amd.engine import SamplingParams
    out.append(f"## (c) one {T}-row prefill step, Llama-3-8B shapes, {layers} layers, rank {rank}\n")
    e = build_engine(layers, rank, T, False)
    prompt = [1] + [(7 * i) % 30000 + 2 for i in range(T - 1)]
    res = {}
    for rep in range(3):
        for tag, lora in (("base", None), ("adapter", "a0")):
            s, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            e.generate([prompt], SamplingParams(max_tokens=1, lora=lora, cache_salt=f"{tag}{rep}"))
            en.record()
            torch.cuda.synchronize()
            res.setdefault(tag, []).append(s.elapsed_time(en))
    out.append("One eager step (generate of 1 token from a prompt of %d tokens), device ms, median of 3 alternating "
               "runs after none discarded (min .. max).\n" % T)
    out.append("| mode | ms | min .. max |")
    out.append("|---|---|---|")
    for tag in ("base", "adapter"):
        out.append(f"| {tag} | {statistics.median(res[tag]):.1f} | {min(res[tag]):.1f} .. {max(res[tag]):.1f} |")
        print(out[-1], flush=True)
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,16,64,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--skip", default="", help="comma list of: kernel, step, prefill")
    ap.add_argument("--out", default="profiles/lora_kernel.md")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py measures on a GPU"
    skip = set(a.skip.split(","))
    out = ["# Multi-LoRA shrink / expand: measurements\n",
           f"Command: `python tools/bench_lora.py --rows {a.rows} --iters {a.iters} --repeats {a.repeats} "
           f"--layers {a.layers} --rank {a.rank}` on {torch.cuda.get_device_name(0)}.\n"]
    if "kernel" not in skip:
        kernel_table([int(r) for r in a.rows.split(",")], a.iters, a.repeats, out)
    if "step" not in skip:
        step_table(a.layers, a.rank, out)
    if "prefill" not in skip:
        prefill_table(a.layers, a.rank, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
