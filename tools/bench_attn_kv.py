"""Micro-benchmark: paged decode attention over a bf16 and an FP8 (e4m3) KV cache, same process.

Llama-3-8B shapes (32 q / 8 kv heads, d 128, block 32).  Per shape (rows x keys) the two dtypes
are timed alternately, ``--rounds`` times each, rotating over ``--layers`` layers' caches so that
even the FP8 working set exceeds the 256 MiB Infinity Cache; the bf16 caches hold the
dequantised FP8 values, so the two outputs are the same computation and their largest
difference is printed as a check.  Reported: median / min microseconds per launch and the
effective TB/s of KV bytes (rows x keys x 8 x 128 x 2 tensors x element size).

    python tools/bench_attn_kv.py [--out FILE.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.ops import attention as A  # noqa: E402

NQ, NKV, D, BS = 32, 8, 128, 32
SHAPES = ((64, 384), (64, 4096), (512, 384))   # 512 x 384: the wide-batch decode of profiles/r6_wide_512_kgrid.md
FP8 = torch.float8_e4m3fn


def caches(nblk, layers, gen):
    out = []
    for _ in range(layers):
        k8 = torch.randn(nblk, NKV, BS, D, device="cuda", generator=gen).clamp(-448, 448).to(FP8)
        v8 = torch.randn(nblk, NKV, D, BS, device="cuda", generator=gen).clamp(-448, 448).to(FP8)
        out.append(((k8, v8), (k8.to(torch.bfloat16), v8.to(torch.bfloat16))))
    return out


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_kv needs the GPU: no timing is taken on the CPU")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows_out = []
    for B, ctx in SHAPES:
        maxb = (ctx + BS - 1) // BS
        layers = caches(B * maxb + 1, a.layers, gen)
        bt = torch.arange(B * maxb, dtype=torch.int32, device="cuda").view(B, maxb)
        cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        q = torch.randn(B, NQ, D, device="cuda", generator=gen).to(torch.bfloat16)
        o, ml = A.decode_workspace(B, NQ, maxb, BS, "cuda", n_kv=NKV)
        md = A.AttnMetadata(num_decode=B, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0, slot_mapping=None,
                            decode_block_tables=bt, decode_context_lens=cl, decode_part_o=o, decode_part_ml=ml)
        run = {"fp8": lambda i: A.paged_attention(q, *layers[i % a.layers][0], md, 0.088),
               "bf16": lambda i: A.paged_attention(q, *layers[i % a.layers][1], md, 0.088)}
        diff = float((run["fp8"](0).float() - run["bf16"](0).float()).abs().max())
        for f in run.values():      # warm-up: every layer's caches once per dtype
            for i in range(a.layers):
                f(i)
        torch.cuda.synchronize()
        t = {"bf16": [], "fp8": []}
        for _ in range(a.rounds):   # alternate the two within one call
            for name in ("bf16", "fp8"):
                t[name].append(timed(run[name], a.iters))
        rec = {"rows": B, "keys": ctx, "max_abs_diff": diff}
        for name, size in (("bf16", 2), ("fp8", 1)):
            med, gb = statistics.median(t[name]), B * ctx * NKV * D * 2 * size / 1e9
            rec[name] = {"us_median": round(med, 1), "us_min": round(min(t[name]), 1), "us_max": round(max(t[name]), 1),
                         "kv_tb_s": round(gb / med * 1e3, 2), "kv_mb": round(gb * 1e3, 1)}
        rec["speedup"] = round(rec["bf16"]["us_median"] / rec["fp8"]["us_median"], 3)
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
        del layers, run
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("| rows x keys | bf16 us (min-max) | bf16 TB/s | FP8 us (min-max) | FP8 TB/s | bf16 / FP8 | max abs diff |\n")
            f.write("|---|---|---|---|---|---|---|\n")
            for r in rows_out:
                b, e = r["bf16"], r["fp8"]
                f.write(f"| {r['rows']} x {r['keys']} | {b['us_median']} ({b['us_min']}-{b['us_max']}) | {b['kv_tb_s']} | "
                        f"{e['us_median']} ({e['us_min']}-{e['us_max']}) | {e['kv_tb_s']} | {r['speedup']} | "
                        f"{r['max_abs_diff']:.3g} |\n")


if __name__ == "__main__":
    main()
