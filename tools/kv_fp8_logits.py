"""Largest |logit difference| between an FP8 (e4m3) and a bf16 KV cache on the same weights:
the last prefill row and ``--steps`` decode steps of a few prompts, eager GPU engines.

    python tools/kv_fp8_logits.py [--model tiny-llama-gqa4] [--model-path DIR] [--steps 8]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polykey_service_amd.engine import EngineConfig, LLMEngine, SamplingParams  # noqa: E402


def logits_of(a, dtype, prompts):
    e = LLMEngine(EngineConfig(model=a.model, model_path=a.model_path, num_layers=a.layers, max_num_seqs=8,
                               max_num_batched_tokens=1024, max_model_len=1024, hip_graphs=False, device="cuda:0",
                               kv_cache_dtype=dtype))
    e.runner.keep_logits = True
    seqs = [e.add_request(p, SamplingParams(max_tokens=a.steps, temperature=0.0, ignore_eos=True)) for p in prompts]
    out = []
    while e.has_unfinished():
        e.step()
        out.append(e.runner.last_logits.float().cpu().clone())
    return out, [s.output_ids for s in seqs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="tiny-llama-gqa4")
    ap.add_argument("--model-path", default="")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    prompts = [[1] + torch.randint(3, 900, (n,), generator=g).tolist() for n in (5, 60, 300, 600)]
    b, tb = logits_of(a, "bf16", prompts)
    f, tf = logits_of(a, "fp8", prompts)
    # compare while both engines are on the same token history (the prefill step always is)
    same = 0
    for i in range(a.steps):
        if any(x[:i] != y[:i] for x, y in zip(tb, tf)):
            break
        same = i + 1
    d = [float((x - y).abs().max()) for x, y in zip(b[:same], f[:same])]
    print(json.dumps({"model": a.model_path or a.model, "steps_compared": same, "max_abs_dlogit": max(d),
                      "prefill_abs_dlogit": d[0], "logit_abs_max": float(b[0].abs().max()),
                      "tokens_equal": tb == tf}), flush=True)


if __name__ == "__main__":
    main()
