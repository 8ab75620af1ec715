"""Micro-benchmark: verify attention (pk_paged_verify, speculative decoding) against decode attention
(pk_paged_decode) of the same build, same sequences and contexts, Llama-3-8B shape (32 q / 8 kv
heads, d 128).  Device time from graph replays: each graph holds one launch per layer over 8 layers'
KV caches (more than the 256 MiB Infinity Cache at every shape here, so K/V come from HBM as in a real
step), replayed and timed with device events.  Both kernels read the same K/V bytes once; the
verify launch carries QR query rows per sequence in the tile columns decode leaves as padding.

    python tools/bench_attn_verify.py [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.ops import attention as A  # noqa: E402

NQ, NKV, D, BS, LAYERS = 32, 8, 128, 32, 8
SHAPES = ((64, 384), (64, 4096), (512, 384))   # (sequences, keys)
SCALE = D ** -0.5


def graph_time_us(fn, replays=30):
    """Mean device time of one call of ``fn`` (LAYERS launches) in microseconds per launch."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / (replays * LAYERS) * 1000)
    return min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_verify needs the GPU")
    rows = []
    for B, ctx in SHAPES:
        maxb = (ctx + BS - 1) // BS
        nblk = B * maxb + 1
        layers = [(torch.randn(nblk, NKV, BS, D, device="cuda").to(torch.bfloat16),
                   torch.randn(nblk, NKV, D, BS, device="cuda").to(torch.bfloat16)) for _ in range(LAYERS)]
        kv_bytes = B * ctx * NKV * D * 2 * 2
        bt = torch.arange(B * maxb, dtype=torch.int32, device="cuda").view(B, maxb)
        cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        q1 = torch.randn(B, NQ, D, device="cuda").to(torch.bfloat16)
        ws = A.decode_workspace(B, NQ, maxb, BS, "cuda", kv_heads=NKV)
        md = A.AttnMetadata(num_decode=B, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0, slot_mapping=None,
                            decode_block_tables=bt, decode_context_lens=cl, decode_part_o=ws[0], decode_part_ml=ws[1])
        out1 = torch.empty(B, NQ * D, dtype=torch.bfloat16, device="cuda")
        lo, hi = graph_time_us(lambda: [A.paged_attention(q1, k, v, md, SCALE, out=out1) for k, v in layers])
        rec = {"seqs": B, "keys": ctx, "kv_mb_per_launch": round(kv_bytes / 1e6, 1), "decode_us": round(lo, 2),
               "decode_us_max": round(hi, 2), "decode_tb_s": round(kv_bytes / lo / 1e6, 2)}
        for qr in (2, 4):
            q = torch.randn(B * qr, NQ, D, device="cuda").to(torch.bfloat16)
            vws = A.verify_workspace(B, qr, NQ, maxb, BS, "cuda", kv_heads=NKV)
            vmd = A.AttnMetadata(num_decode=B * qr, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0,
                                 slot_mapping=None, decode_part_o=vws[0], decode_part_ml=vws[1], verify_qr=qr,
                                 verify_rows=torch.full((B,), qr, dtype=torch.int32, device="cuda"),
                                 verify_block_tables=bt, verify_context_lens=cl)
            out = torch.empty(B * qr, NQ * D, dtype=torch.bfloat16, device="cuda")
            lo_v, hi_v = graph_time_us(lambda: [A.paged_verify(q, k, v, vmd, SCALE, out=out) for k, v in layers])
            rec.update({f"verify_qr{qr}_us": round(lo_v, 2), f"verify_qr{qr}_us_max": round(hi_v, 2),
                        f"ratio_qr{qr}": round(lo_v / lo, 3)})
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del layers
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
