"""Perplexity of a token stream under the served model: teacher-forced prompt logprobs.

Cuts the input -- a ``.npy`` file of token ids, or a text file run through the model's tokenizer --
into windows of ``--window`` tokens, sends each through the engine with ``prompt_logprobs = 0`` and
reports the mean negative log-likelihood per scored token, the perplexity ``exp(mean NLL)`` and the
share of greedy tokens (``rank == 1``).  The first token of a window has no context and is not scored.
``--compare bf16,fp8,mxfp4`` runs the weight formats one after another on the same windows and prints
them side by side (``--kv-cache-dtype`` applies to each).

On random-init weights (no ``--model-path``) the numbers exercise the path and measure nothing about
a trained model: every format scores noise.

Usage: ``python tools/eval_ppl.py --model llama3-8b --model-path /ckpt --input ids.npy --window 2048``
       ``python tools/eval_ppl.py --model tiny-llama --input text.txt --window 64 --compare bf16,fp8 --device cpu``
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def load_ids(path: str, tokenizer, vocab: int):
    if path.endswith(".npy"):
        ids = np.load(path).astype(np.int64).reshape(-1).tolist()
    else:
        with open(path, encoding="utf-8") as f:
            ids = tokenizer.encode(f.read())
    if not ids or min(ids) < 0 or max(ids) >= vocab:
        raise SystemExit(f"{path}: empty, or token ids outside [0, {vocab})")
    return ids


def windows_of(ids, window: int, limit: int):
    out = [ids[i:i + window] for i in range(0, len(ids), window)]
    out = [w for w in out if len(w) >= 2]
    return out[:limit] if limit else out


def score(engine, windows, batch: int):
    """-> (sum of NLL, scored tokens, greedy tokens, tokens whose logprob is -inf)."""
    from polykey_service_amd.engine import SamplingParams
    nll, n, greedy, ninf = 0.0, 0, 0, 0
    for b0 in range(0, len(windows), batch):
        seqs = [engine.add_request(w, SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=0))
                for w in windows[b0:b0 + batch]]
        got = {}
        while engine.has_unfinished():
            for o in engine.step():
                if o.prompt_logprobs is not None:
                    got[o.request_id] = o.prompt_logprobs
        for s in seqs:
            for lp, rank, _ in got[s.request_id][1:]:
                if math.isinf(lp):
                    ninf += 1
                    continue
                nll -= lp
                n += 1
                greedy += rank == 1
    return nll, n, greedy, ninf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, help=".npy of token ids, or a text file")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--max-windows", type=int, default=0, help="0 = all")
    ap.add_argument("--batch", type=int, default=4, help="windows in flight")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--model-path", default="")
    ap.add_argument("--tokenizer", default="")
    ap.add_argument("--kv-cache-dtype", default="auto")
    ap.add_argument("--weight-dtype", default="bf16")
    ap.add_argument("--compare", default="", help="comma-separated weight dtypes, run one after another")
    ap.add_argument("--device", default="")
    ap.add_argument("--num-layers", type=int, default=0)
    a = ap.parse_args()

    import torch

    from polykey_service_amd.engine import EngineConfig, LLMEngine
    from polykey_service_amd.engine.llm_engine import tokenizer_for
    from polykey_service_amd.parallel.state import ParallelState

    formats = [f.strip() for f in a.compare.split(",") if f.strip()] or [a.weight_dtype]
    results, windows = [], None
    for wd in formats:
        cfg = EngineConfig(model=a.model, model_path=a.model_path, tokenizer=a.tokenizer, max_num_seqs=max(a.batch, 1),
                           max_num_batched_tokens=min(max(a.window, 32), 8192), max_model_len=a.window + 32,
                           kv_cache_dtype=a.kv_cache_dtype, weight_dtype=wd, device=a.device,
                           hip_graphs=False, num_layers=a.num_layers, prefix_caching=False)
        st = ParallelState(device=torch.device(a.device)) if a.device else ParallelState()
        engine = LLMEngine(cfg, st)
        if windows is None:
            ids = load_ids(a.input, tokenizer_for(cfg, engine.mcfg), engine.mcfg.vocab_size)
            windows = windows_of(ids, a.window, a.max_windows)
        nll, n, greedy, ninf = score(engine, windows, a.batch)
        mean = nll / max(n, 1)
        results.append({"weight_dtype": wd, "kv_cache_dtype": cfg.kv_cache_dtype, "windows": len(windows),
                        "scored_tokens": n, "zero_probability_tokens": ninf, "mean_nll": mean,
                        "perplexity": math.exp(mean), "greedy_share": greedy / max(n, 1),
                        "random_init": not a.model_path})
        engine.shutdown()
        del engine
    for r in results:
        print(json.dumps(r))
    if not a.model_path:
        print("random-init weights: these figures say nothing about a trained model", file=sys.stderr)


if __name__ == "__main__":
    main()
