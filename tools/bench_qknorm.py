"""Times the two QK-norm kernels (Qwen3) against their no-norm parents of the same build.
Needs a GPU; writes a markdown report (``--out``).

Shape: Qwen3-8B / Llama-3-8B attention (32 q heads, 8 kv heads, head_dim 128), block size 32.

* ``rope_and_cache`` with and without the norm at 64 rows and at 8192 rows, bf16 and FP8 caches;
* ``qkv_reduce_rope_cache`` with and without the norm at 64 rows, at the K split the folded decode
  chain picks for the 8B QKV projection (``gemm._rowscale_tiling``).

Times are device time: ``--iters`` launches captured into one graph, replays timed between device
events; the two variants alternate, ``--repeats`` times, and the table gives the median and the
range.  Inputs are re-used across launches (``rope_and_cache`` rotates its buffer in place: values
drift but stay finite, and neither kernel's time depends on values)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from polykey_service_amd.ops import attention as A
from polykey_service_amd.ops import gemm, reference

NQ, NKV, BS, HIDDEN = 32, 8, 32, 4096
N = (NQ + 2 * NKV) * 128
REPLAYS = 5
DEV = "cuda"


def graph_of(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPLAYS):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / (REPLAYS * iters) * 1000.0  # us per launch


def ab(parent, normed, iters, repeats):
    """Alternating repeats -> {name: [us per launch]}."""
    gs = {"parent": graph_of(parent, iters), "qknorm": graph_of(normed, iters)}
    t = {k: [] for k in gs}
    for _ in range(repeats):
        for k, g in gs.items():
            t[k].append(time_graph(g, iters))
    return t


def row(out, label, rows, t, bytes_moved):
    mp, mn = statistics.median(t["parent"]), statistics.median(t["qknorm"])
    out.append(f"| {label} | {rows} | {mp:.2f} ({min(t['parent']):.2f} .. {max(t['parent']):.2f}) | "
               f"{mn:.2f} ({min(t['qknorm']):.2f} .. {max(t['qknorm']):.2f}) | {mn / mp:.3f} | "
               f"{bytes_moved / mn / 1e6:.2f} |")
    print(out[-1], flush=True)


def common(T):
    cs = reference.rope_cos_sin_cache(T + 64, 128, 1e6).to(DEV)
    pos = torch.arange(T, dtype=torch.int32, device=DEV)
    slots = torch.arange(T, dtype=torch.int32, device=DEV)  # whole aligned blocks: the prefill case
    g = torch.Generator().manual_seed(0)
    qw, kw = ((0.5 + torch.rand(128, generator=g)).to(torch.bfloat16).to(DEV) for _ in range(2))
    return cs, pos, slots, qw, kw


def caches(T, fp8):
    nb = (T + BS - 1) // BS
    dt = A.FP8 if fp8 else torch.bfloat16
    return (torch.zeros((nb, NKV, BS, 128), dtype=torch.uint8 if fp8 else dt, device=DEV).view(dt),
            torch.zeros((nb, NKV, 128, BS), dtype=torch.uint8 if fp8 else dt, device=DEV).view(dt))


def bench_rope(out, T, iters, repeats):
    cs, pos, slots, qw, kw = common(T)
    for fp8 in (False, True):
        kc, vc = caches(T, fp8)
        x = torch.randn((T, N), device=DEV).to(torch.bfloat16)
        t = ab(lambda: A.rope_and_cache(x, pos, cs, kc, vc, slots, NQ, NKV),
               lambda: A.rope_and_cache(x, pos, cs, kc, vc, slots, NQ, NKV, q_norm=qw, k_norm=kw, eps=1e-6), iters, repeats)
        # q and k read and written in place, v read, k and v written to the cache, the cos|sin rows read
        moved = T * ((NQ + NKV) * 128 * 4 + NKV * 128 * 2 + 2 * NKV * 128 * (1 if fp8 else 2) + 128 * 4)
        row(out, f"rope_and_cache, {'FP8' if fp8 else 'bf16'} cache", T, t, moved)


def bench_slab(out, M, iters, repeats):
    cs, pos, slots, qw, kw = common(M)
    S, _ = gemm._rowscale_tiling(N, HIDDEN, M, torch.empty((N, HIDDEN), dtype=torch.bfloat16, device="meta"),
                                 gemm.QKV_HALF and M <= gemm.SKINNY_MAX_M, None)
    kc, vc = caches(M, False)
    p = gemm.Partial(torch.randn(S * M * N, device=DEV), S, M, N)
    t = ab(lambda: gemm.qkv_reduce_rope_cache(p, pos, cs, kc, vc, slots, NQ, NKV),
           lambda: gemm.qkv_reduce_rope_cache(p, pos, cs, kc, vc, slots, NQ, NKV, q_norm=qw, k_norm=kw, eps=1e-6),
           iters, repeats)
    moved = M * (S * N * 4 + N * 2 + 128 * 4)  # S fp32 slabs read; q, k, v written as bf16; cos|sin rows
    row(out, f"qkv_reduce_rope_cache, S = {S}", M, t, moved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/qwen3_qknorm.md")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qknorm.py measures on a GPU"
    out = ["# QK-norm fused into the RoPE / KV-write kernels: measurements\n",
           f"Command: `python tools/bench_qknorm.py --iters {a.iters} --repeats {a.repeats}` on "
           f"{torch.cuda.get_device_name(0)}.\n",
           f"Shape: {NQ} q heads, {NKV} kv heads, head_dim 128 (Qwen3-8B / Llama-3-8B), block size {BS}.  Device "
           f"microseconds per launch: a graph of {a.iters} launches (8192 rows: {max(1, a.iters // 10)}), {REPLAYS} replays "
           f"between device events; parent and QK-norm variant alternate, median of {a.repeats} repeats (min .. max).  "
           "`TB/s` is the bytes the QK-norm launch must move (from shapes) over its median time; the launches of a "
           "graph re-use their buffers, so at 64 rows they are served from cache and the figure is not an HBM rate.\n",
           "| kernel | rows | parent us | qknorm us | qknorm / parent | TB/s |", "|---|---|---|---|---|---|"]
    bench_rope(out, 64, a.iters, a.repeats)
    bench_slab(out, 64, a.iters, a.repeats)
    bench_rope(out, 8192, max(1, a.iters // 10), a.repeats)
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
