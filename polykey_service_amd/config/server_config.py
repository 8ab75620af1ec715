"""Server configuration.

The reference server reads only ``LISTEN_ADDR`` (``cmd/polykey/main.go:57-60``) even though
``POLYKEY_ENV`` / ``POLYKEY_LOG_LEVEL`` are set for it.  Here the server
uses the same mechanism as the client loader (defaults < flags < env) and also consumes
the engine options that the on-node backend needs.
"""
from __future__ import annotations

import dataclasses
import os
import sys
from typing import Mapping, Optional, Sequence

from .goflag import FlagSet


@dataclasses.dataclass
class ServerConfig:
    listen_addr: str = ":50051"
    http_addr: str = ""            # OpenAI-compatible route; "" disables
    metrics_addr: str = ""         # Prometheus exporter; "" disables
    log_level: str = "info"
    environment: str = "development"
    backend: str = "mock"          # mock | local
    model: str = "llama3-8b"
    # several models behind this one front end, each on its own GPU(s) of the node:
    # "<model>[@<gpu>|@<first>-<last>][,...]", e.g. "llama3-8b@0-3,mixtral-8x7b@4" (a device range
    # = replicas of that model); "llm.chat:<model>" / OpenAI "model" pick one.  "" -> ``model``
    serve_models: str = ""
    model_path: str = ""           # directory of safetensors shards; "" → random init
    tokenizer: str = ""            # tokenizer.json path; "" → byte-level tokenizer
    dtype: str = "bfloat16"
    tp: int = 1
    ep: int = 1
    replicas: int = 1
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 8192
    num_layers: int = 0            # > 0: truncate the preset's depth (rehearsals)
    kv_block_size: int = 32
    gpu_mem_fraction: float = 0.90
    num_kv_blocks: int = 0         # 0 → size from free HBM
    kv_cache_dtype: str = "auto"   # auto | bf16 | fp8 (alias fp8_e4m3): KV-cache element type
    weight_dtype: str = "auto"     # auto | bf16 | fp8 (alias fp8_e4m3) | mxfp4: projection weight element type
    # LoRA adapters served next to the model: "name=path[,name=path...]" (PEFT directories), all
    # resident; OpenAI "model": "<name>" / "llm.chat:<name>" / parameters.lora pick one
    lora_modules: str = ""
    max_lora_rank: int = 64
    # speculative decoding: "" = off, "ngram" = prompt-lookup drafts verified in one step (dense
    # models, one GPU, bf16 KV cache); k draft tokens per sequence and step, n-gram lengths tried
    speculative: str = ""
    num_speculative_tokens: int = 3
    ngram_max: int = 4
    ngram_min: int = 2
    # parallel sampling (n > 1): fork choice 0's prompt KV for the other choices (False: they prefill it)
    kv_fork: bool = True
    hip_graphs: bool = True
    device: str = "cuda"
    seed: int = 0
    shutdown_grace: float = 10.0
    tls_cert: str = ""             # PEM certificate chain; with tls_key: TLS instead of insecure
    tls_key: str = ""              # PEM private key

    @property
    def random_init(self) -> bool:
        return self.model_path == ""


_ENV = {
    "listen_addr": "LISTEN_ADDR",
    "http_addr": "POLYKEY_HTTP_ADDR",
    "metrics_addr": "POLYKEY_METRICS_ADDR",
    "log_level": "POLYKEY_LOG_LEVEL",
    "environment": "POLYKEY_ENV",
    "backend": "POLYKEY_BACKEND",
    "model": "POLYKEY_MODEL",
    "serve_models": "POLYKEY_SERVE_MODELS",
    "model_path": "POLYKEY_MODEL_PATH",
    "tokenizer": "POLYKEY_TOKENIZER",
    "dtype": "POLYKEY_DTYPE",
    "tp": "POLYKEY_TP",
    "ep": "POLYKEY_EP",
    "replicas": "POLYKEY_REPLICAS",
    "max_num_seqs": "POLYKEY_MAX_NUM_SEQS",
    "max_num_batched_tokens": "POLYKEY_MAX_BATCHED_TOKENS",
    "max_model_len": "POLYKEY_MAX_MODEL_LEN",
    "num_layers": "POLYKEY_NUM_LAYERS",
    "kv_block_size": "POLYKEY_KV_BLOCK_SIZE",
    "gpu_mem_fraction": "POLYKEY_GPU_MEM_FRACTION",
    "num_kv_blocks": "POLYKEY_NUM_KV_BLOCKS",
    "kv_cache_dtype": "POLYKEY_KV_CACHE_DTYPE",
    "weight_dtype": "POLYKEY_WEIGHT_DTYPE",
    "lora_modules": "POLYKEY_LORA_MODULES",
    "max_lora_rank": "POLYKEY_MAX_LORA_RANK",
    "speculative": "POLYKEY_SPECULATIVE",
    "num_speculative_tokens": "POLYKEY_NUM_SPECULATIVE_TOKENS",
    "ngram_max": "POLYKEY_NGRAM_MAX",
    "ngram_min": "POLYKEY_NGRAM_MIN",
    "kv_fork": "POLYKEY_KV_FORK",
    "hip_graphs": "POLYKEY_HIP_GRAPHS",
    "device": "POLYKEY_DEVICE",
    "seed": "POLYKEY_SEED",
    "shutdown_grace": "POLYKEY_SHUTDOWN_GRACE",
    "tls_cert": "POLYKEY_TLS_CERT",
    "tls_key": "POLYKEY_TLS_KEY",
}


KV_CACHE_DTYPES = ("auto", "bf16", "fp8")


def normalize_kv_cache_dtype(value: str) -> str:
    """``--kv-cache-dtype`` / ``POLYKEY_KV_CACHE_DTYPE`` -> "bf16" or "fp8".  "auto" means bf16 and
    "fp8_e4m3" is an alias of "fp8" (OCP e4m3, per-layer scales); anything else is an error."""
    v = str(value).strip().lower()
    if v in ("auto", "bf16"):
        return "bf16"
    if v in ("fp8", "fp8_e4m3"):
        return "fp8"
    raise ValueError(f"kv_cache_dtype must be one of {', '.join(KV_CACHE_DTYPES)} (got {value!r})")


WEIGHT_DTYPES = ("auto", "bf16", "fp8", "mxfp4")


def normalize_weight_dtype(value: str) -> str:
    """``--weight-dtype`` / ``POLYKEY_WEIGHT_DTYPE`` -> "bf16", "fp8" or "mxfp4".  "auto" means bf16,
    "fp8_e4m3" is an alias of "fp8" (weight-only OCP e4m3, one scale per output channel) and "mxfp4"
    (weight-only OCP Microscaling FP4: e2m1 elements, one e8m0 scale per 32) has no alias; anything
    else is an error."""
    v = str(value).strip().lower()
    if v in ("auto", "bf16"):
        return "bf16"
    if v in ("fp8", "fp8_e4m3"):
        return "fp8"
    if v == "mxfp4":
        return "mxfp4"
    raise ValueError(f"weight_dtype must be one of {', '.join(WEIGHT_DTYPES)} (got {value!r})")


def env_weight_dtype(environ: Optional[Mapping[str, str]] = None) -> str:
    """The weight dtype a config built without the field takes: ``POLYKEY_WEIGHT_DTYPE`` (the
    variable of :data:`_ENV`), else "auto".  Explicit values always win."""
    return (os.environ if environ is None else environ).get(_ENV["weight_dtype"], "") or "auto"


SPECULATIVE_METHODS = ("ngram",)


def normalize_speculative(value) -> str:
    """``--speculative`` / ``POLYKEY_SPECULATIVE`` -> "" (off) or "ngram"; anything else is an error."""
    v = str(value or "").strip().lower()
    if v in ("", "none", "off"):
        return ""
    if v in SPECULATIVE_METHODS:
        return v
    raise ValueError(f"speculative must be one of {', '.join(SPECULATIVE_METHODS)} (got {value!r})")


def parse_lora_modules(spec) -> tuple:
    """``--lora-modules`` / ``POLYKEY_LORA_MODULES``: "name=path[,name=path...]" -> ((name, path), ...);
    a tuple of pairs passes through."""
    if not isinstance(spec, str):
        return tuple((str(n), p) for n, p in (spec or ()))
    out = []
    for item in filter(None, (s.strip() for s in spec.split(","))):
        name, sep, path = item.partition("=")
        if not sep or not name.strip() or not path.strip():
            raise ValueError(f"lora_modules entries must be name=path (got {item!r})")
        out.append((name.strip(), path.strip()))
    if len({n for n, _ in out}) != len(out):
        raise ValueError(f"lora_modules names must be unique (got {[n for n, _ in out]})")
    return tuple(out)


def _flag_name(field: str) -> str:
    return field.replace("_", "-")


def load_server_config(argv: Optional[Sequence[str]] = None,
                       environ: Optional[Mapping[str, str]] = None) -> ServerConfig:
    environ = os.environ if environ is None else environ
    cfg = ServerConfig()
    fs = FlagSet("polykey")
    for f in dataclasses.fields(ServerConfig):
        d = getattr(cfg, f.name)
        name = _flag_name(f.name)
        if isinstance(d, bool):
            fs.bool(name, d, f.name)
        elif isinstance(d, int):
            fs.int(name, d, f.name)
        elif isinstance(d, float):
            fs.float(name, d, f.name)
        else:
            fs.string(name, d, f.name)
    fs.parse(sys.argv[1:] if argv is None else argv)
    for f in dataclasses.fields(ServerConfig):
        setattr(cfg, f.name, fs[_flag_name(f.name)])
    for fname, env in _ENV.items():
        raw = environ.get(env, "")
        if raw == "":
            continue
        cur = getattr(cfg, fname)
        try:
            if isinstance(cur, bool):
                val = raw.lower() in ("1", "true", "t", "yes", "on")
            elif isinstance(cur, int):
                val = int(raw, 0)
            elif isinstance(cur, float):
                val = float(raw)
            else:
                val = raw
        except ValueError:
            continue
        setattr(cfg, fname, val)
    cfg.kv_cache_dtype = normalize_kv_cache_dtype(cfg.kv_cache_dtype)
    cfg.weight_dtype = normalize_weight_dtype(cfg.weight_dtype)
    parse_lora_modules(cfg.lora_modules)  # a malformed list fails at start-up
    cfg.speculative = normalize_speculative(cfg.speculative)
    if cfg.speculative and (cfg.num_speculative_tokens < 1 or not 1 <= cfg.ngram_min <= cfg.ngram_max):
        raise ValueError("speculative decoding needs num_speculative_tokens >= 1 and 1 <= ngram_min <= ngram_max "
                         f"(got {cfg.num_speculative_tokens}, {cfg.ngram_min}, {cfg.ngram_max})")
    return cfg
