"""Synchronous engine: add requests, ``step()`` until done (the L5 engine of SURVEY.md §3.6).

``step()`` = schedule → model runner (pack, H2D, forward / graph replay, sample, D2H) →
append tokens, detect stop conditions, free finished sequences → per-request outputs.
The async/gRPC face is :mod:`polykey_service_amd.engine.async_llm`.
"""
from __future__ import annotations

import dataclasses
import logging
import os
import time
import uuid
from typing import Callable, Dict, Iterable, List, Optional

import torch

from .._native.loader import load_extension
from ..config.server_config import (env_weight_dtype, normalize_kv_cache_dtype, normalize_weight_dtype,
                                    parse_lora_modules)
from ..models import build_model
from ..models.config import ModelConfig, get_config
from ..models.llama import QUANT_FORMATS
from ..ops.sampler import logprob_entry
from ..parallel.state import ParallelState, get_state
from . import grammar, spec
from .model_runner import ModelRunner, RunnerConfig
from .scheduler import ScheduledBatch, Scheduler
from .sequence import FinishReason, RequestOutput, SamplingParams, Sequence, seq_metrics
from .tokenizer import get_tokenizer


@dataclasses.dataclass
class EngineConfig:
    model: str = "llama3-8b"
    model_path: str = ""
    tokenizer: str = ""
    dtype: str = "bfloat16"
    seed: int = 0
    block_size: int = 32
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 8192
    num_kv_blocks: int = 0
    gpu_mem_fraction: float = 0.90
    hip_graphs: bool = True
    # KV-cache element type: "auto" | "bf16" | "fp8" ("fp8_e4m3"): OCP e4m3 bytes with per-layer
    # k_scale / v_scale, half the bytes per token (README "KV cache dtype")
    kv_cache_dtype: str = "auto"
    # projection weight element type: "auto" | "bf16" | "fp8" ("fp8_e4m3"): weight-only OCP e4m3 with
    # one fp32 scale per output channel | "mxfp4": weight-only OCP Microscaling FP4 (e2m1, one e8m0
    # scale per 32 elements), quantised at set-up (README "Weight dtype").  Opt-in; a
    # config built without it takes POLYKEY_WEIGHT_DTYPE (config/server_config.py env_weight_dtype),
    # so with that variable set to fp8 every engine of the process asks for FP8 weights, and one
    # that cannot have them (MoE, TP, EP) raises instead of quietly serving bf16
    weight_dtype: str = dataclasses.field(default_factory=env_weight_dtype)
    graph_batch_sizes: tuple = ()
    watermark: float = 0.01
    device: str = ""
    overlap: bool = False  # pipelined steps (see LLMEngine.step); AsyncLLM turns it on
    # scheduler policy (engine/scheduler.py): prefill_first | decode_first (decode_first measured
    # slower on the headline wave: profiles/r2_decode_ab.txt "scheduler policy")
    sched_policy: str = "prefill_first"
    max_decode_stall: int = 4
    # > 0: keep only the first num_layers decoder layers of the preset (rehearsals of a large
    # model's per-rank shapes with fewer layers, tests); 0: the preset's depth
    num_layers: int = 0
    # automatic prefix caching (csrc/runtime/block_manager.h); POLYKEY_PREFIX_CACHING=0 disables
    prefix_caching: bool = dataclasses.field(
        default_factory=lambda: os.environ.get("POLYKEY_PREFIX_CACHING", "1") != "0")
    # LoRA adapters served next to the base model: (name, PEFT directory) pairs -- or (name,
    # models.lora.LoraAdapter) for adapters built in memory -- all resident, one slot each (README
    # "LoRA adapters"); a request picks one with SamplingParams.lora.  () = off: nothing changes
    lora_modules: tuple = ()
    max_lora_rank: int = 64
    # speculative decoding (README "Speculative decoding"): None = off, "ngram" = prompt-lookup drafts
    # verified in one step; num_speculative_tokens = k drafts per sequence and step (k + 1 query rows)
    speculative: Optional[str] = None
    num_speculative_tokens: int = 3
    ngram_max: int = 4
    ngram_min: int = 2
    # parallel sampling (README "Parallel sampling"): choices 1 .. n-1 of an n > 1 request take choice
    # 0's prompt KV by a fork (shared full blocks, one copied partial block) instead of prefilling
    # it again; False / POLYKEY_KV_FORK=0: they prefill it themselves (prefix cache as usual)
    kv_fork: bool = dataclasses.field(default_factory=lambda: os.environ.get("POLYKEY_KV_FORK", "1") != "0")

    @classmethod
    def from_server_config(cls, sc) -> "EngineConfig":
        return cls(model=sc.model, model_path=sc.model_path, tokenizer=sc.tokenizer, dtype=sc.dtype, seed=sc.seed,
                   block_size=sc.kv_block_size, max_num_seqs=sc.max_num_seqs,
                   max_num_batched_tokens=sc.max_num_batched_tokens, max_model_len=sc.max_model_len,
                   num_kv_blocks=sc.num_kv_blocks, gpu_mem_fraction=sc.gpu_mem_fraction, hip_graphs=sc.hip_graphs,
                   num_layers=getattr(sc, "num_layers", 0), kv_cache_dtype=getattr(sc, "kv_cache_dtype", "auto"),
                   weight_dtype=getattr(sc, "weight_dtype", "auto"),
                   lora_modules=parse_lora_modules(getattr(sc, "lora_modules", "")),
                   max_lora_rank=getattr(sc, "max_lora_rank", 64),
                   speculative=getattr(sc, "speculative", "") or None,
                   num_speculative_tokens=getattr(sc, "num_speculative_tokens", 3),
                   ngram_max=getattr(sc, "ngram_max", 4), ngram_min=getattr(sc, "ngram_min", 2),
                   kv_fork=bool(getattr(sc, "kv_fork", True)) and os.environ.get("POLYKEY_KV_FORK", "1") != "0")


def tokenizer_for(cfg: EngineConfig, mcfg: Optional[ModelConfig] = None):
    """The tokenizer an engine for ``cfg`` uses (a front end routing to an engine in another
    process builds the same one without the engine)."""
    from .chat_template import family_for
    mcfg = mcfg or get_config(cfg.model_path or cfg.model)
    return get_tokenizer(cfg.tokenizer, mcfg.vocab_size, mcfg.bos_token_id, mcfg.eos_token_id,
                         family_for(mcfg.name, mcfg.is_moe, mcfg.qk_norm))


class LLMEngine:
    def __init__(self, cfg: EngineConfig, st: Optional[ParallelState] = None, model=None):
        cfg = dataclasses.replace(cfg, kv_cache_dtype=normalize_kv_cache_dtype(cfg.kv_cache_dtype),
                                  weight_dtype=normalize_weight_dtype(cfg.weight_dtype))
        self.cfg = cfg
        self.st = st or get_state()
        mcfg: ModelConfig = get_config(cfg.model_path or cfg.model)
        wd = cfg.weight_dtype
        quantised = wd in QUANT_FORMATS
        if quantised:
            # weight-only FP8 / MXFP4 cover the dense Llama projections on one GPU; no silent fallback
            label = QUANT_FORMATS[wd].label
            if mcfg.is_moe:
                raise ValueError(f"weight_dtype={wd} does not support MoE models ({mcfg.name}): the grouped "
                                 "expert GEMMs are bf16-only")
            if self.st.tp_size > 1:
                raise ValueError(f"weight_dtype={wd} does not support tp={self.st.tp_size}: {label} weights are "
                                 "not sharded")
            if self.st.ep_size > 1:
                raise ValueError(f"weight_dtype={wd} does not support ep={self.st.ep_size}: {label} weights are "
                                 "not sharded")
        if cfg.lora_modules:
            # adapters cover the dense Llama projections in bf16 on one GPU; no silent fallback
            if mcfg.is_moe:
                raise ValueError(f"LoRA adapters do not support MoE models ({mcfg.name}) yet: the expert "
                                 "projections have no adapter path (a follow-up)")
            if self.st.tp_size > 1:
                raise ValueError(f"LoRA adapters do not support tp={self.st.tp_size} yet: adapters are not "
                                 "sharded (a follow-up)")
            if self.st.ep_size > 1:
                raise ValueError(f"LoRA adapters do not support ep={self.st.ep_size} yet: adapters are not "
                                 "sharded (a follow-up)")
            if quantised:
                raise ValueError(f"LoRA adapters do not support weight_dtype={wd} yet: the "
                                 f"{'W8' if wd == 'fp8' else 'W4'} chain has no "
                                 "adapter path (a follow-up; use weight_dtype=bf16)")
        if cfg.speculative:
            self._check_speculative(cfg, mcfg)
        if cfg.num_layers > 0 and cfg.num_layers != mcfg.num_layers:
            mcfg = dataclasses.replace(mcfg, num_layers=cfg.num_layers)
        if cfg.max_model_len > mcfg.max_position:
            cfg = dataclasses.replace(cfg, max_model_len=mcfg.max_position)
            self.cfg = cfg
        if cfg.block_size <= 0 or cfg.block_size % 32:
            # the K cache stores 32-token fragment-native tiles (csrc/kernels/common.h kcache_off)
            raise ValueError(f"block_size must be a positive multiple of 32, got {cfg.block_size}")
        # DP attention + EP (ParallelState.dp_attention): every rank schedules its own requests
        # and the ranks step in lockstep because each MoE layer is an all-to-all over all of
        # them.  Steps are synchronous (no overlap / continuations).  With the IPC expert
        # all-to-all (parallel/ep_ipc.py: device-side counts) decode steps replay HIP graphs;
        # without it (multi-node, CPU) the dispatch sizes are read back per layer: eager only.
        self.lockstep = self.st.dp_attention
        if self.lockstep:
            if not mcfg.is_moe:
                raise ValueError("DP attention + EP (tp=1, ep>1) needs an MoE model")
            from ..parallel import ep_ipc
            if self.st.ep_a2a is None:
                self.st.ep_a2a = ep_ipc.maybe_create(self.st, cfg.max_num_seqs * mcfg.experts_per_token,
                                                     mcfg.hidden_size)
            if self.st.ep_a2a is not None and self.st.ep_a2a_prefill is None:
                # prefill-sized steps: a second set of regions sized for the token budget (eager,
                # host-free counts too: no per-layer read-back of the split sizes)
                self.st.ep_a2a_prefill = ep_ipc.maybe_create(
                    self.st, max(cfg.max_num_batched_tokens, cfg.max_num_seqs) * mcfg.experts_per_token,
                    mcfg.hidden_size)
            if self.st.ep_a2a is not None and os.environ.get("POLYKEY_PREFLIGHT", "1") != "0":
                from ..parallel import preflight  # dispatch / return checked once; a failure -> RCCL path
                preflight.run(self.st, paths=("ep_ipc",))
            cfg = dataclasses.replace(cfg, overlap=False,
                                      hip_graphs=cfg.hip_graphs and self.st.ep_a2a is not None)
            self.cfg = cfg
        self.mcfg = mcfg
        dev = torch.device(cfg.device) if cfg.device else self.st.device
        self.device = dev
        dtype = getattr(torch, cfg.dtype)
        if model is None:
            model = build_model(mcfg, self.st, dtype, dev)
            if cfg.model_path:
                model.load_hf(cfg.model_path)
            else:
                model.init_random(cfg.seed)
        self.model = model
        held = getattr(model, "quantised_dtype", None)  # the format a handed-over model already holds
        if held is not None and held != wd:
            raise ValueError(f"weight_dtype={wd} with a model whose projections are already "
                             f"{QUANT_FORMATS[held].label}: pass weight_dtype={held}")
        if quantised:
            if not hasattr(model, "weight_dtype"):
                raise ValueError(f"weight_dtype={wd} is not supported by {type(model).__name__}")
            model.weight_dtype = wd  # before pack_decode_weights, which quantises
        if hasattr(model, "pack_decode_weights"):
            model.pack_decode_weights()
        self.weight_bytes = model.projection_bytes() if hasattr(model, "projection_bytes") else 0
        if not quantised:
            logging.getLogger(__name__).info("weights: dtype %s, %d projection bytes, 0 widen-scratch bytes",
                                             cfg.weight_dtype, self.weight_bytes)
        # LoRA adapters: loaded and made resident here, before the KV cache is sized
        self.lora_names: List[str] = []
        self.lora_bytes = 0
        if cfg.lora_modules:
            self._load_adapters(model, mcfg)
        elif getattr(model, "lora", None) is not None:
            model.lora = None  # a model handed over from an engine that served adapters
        self.tokenizer = tokenizer_for(cfg, mcfg)
        rcfg = RunnerConfig(block_size=cfg.block_size, max_num_seqs=cfg.max_num_seqs,
                            max_num_batched_tokens=cfg.max_num_batched_tokens, max_model_len=cfg.max_model_len,
                            num_kv_blocks=cfg.num_kv_blocks, gpu_mem_fraction=cfg.gpu_mem_fraction,
                            hip_graphs=cfg.hip_graphs, graph_batch_sizes=tuple(cfg.graph_batch_sizes),
                            kv_cache_dtype=cfg.kv_cache_dtype,
                            spec_qr=cfg.num_speculative_tokens + 1 if cfg.speculative else 0)
        self.runner = ModelRunner(model, rcfg, dev)
        # guided decoding: the byte string of every vocabulary id, built once and kept on the device
        off, data = grammar.token_bytes(self.tokenizer, mcfg.vocab_size)
        self._single_bytes = grammar.single_byte_tokens(off, data)
        self.runner.init_grammar(off, data)
        self._serving_preflight(mcfg)
        nblocks = self.runner.allocate_kv_cache()
        self.kv_bytes_per_token = self.runner.kv_bytes_per_block() // cfg.block_size
        logging.getLogger(__name__).info("KV cache: dtype %s, %d bytes per block (%d per token), %d blocks",
                                         cfg.kv_cache_dtype, self.runner.kv_bytes_per_block(),
                                         self.kv_bytes_per_token, nblocks)
        rt = load_extension("_pk_runtime")
        self.bm = rt.BlockManager(nblocks, cfg.block_size, int(nblocks * cfg.watermark), cfg.prefix_caching)
        self.runner.bm = self.bm
        self.scheduler = Scheduler(self.bm, cfg.max_num_seqs, cfg.max_num_batched_tokens, cfg.max_model_len,
                                   policy=cfg.sched_policy, max_decode_stall=cfg.max_decode_stall)
        # (the runner's own method and the scheduler's registry, not a method of this engine: a
        # reference back to the engine would be a cycle, and an engine that only the cyclic
        # collector can free may be torn down in the middle of a later engine's graph capture)
        self.runner.live_requests = self.scheduler.by_request
        self.scheduler.on_free = self.runner.release_penalty_slot
        if cfg.hip_graphs and dev.type == "cuda":
            self.runner.capture_graphs()
        self.step_count = 0
        self.total_output_tokens = 0
        self.overlap = cfg.overlap
        self._inflight = None
        # called between completing a step and scheduling the next (AsyncLLM: admit the requests
        # that arrived meanwhile)
        self.before_schedule: Optional[Callable[[], None]] = None
        self.continuation_steps = 0
        # speculative decoding: the proposer (a plain attribute: tests install scripted ones), and
        # counters of verify steps, draft tokens fed to them and draft tokens accepted
        self.proposer: Optional[spec.Proposer] = None
        self.spec_k = 0
        self.spec_steps = self.spec_draft_tokens = self.spec_accepted_tokens = 0
        # parallel sampling: the fork needs every rank to copy, and workers have no fork message.
        # Counters, taken when the choices are released: n > 1 requests whose choices were forked,
        # requests with a choice released without a fork (no block, fork off, TP / EP), prompt tokens
        # the forked choices were handed.  A forked choice that loses its blocks again before it first
        # runs (Scheduler._unmatch) is counted by the scheduler's num_unforked / num_unforked_tokens
        self.kv_fork = cfg.kv_fork and self.st.tp_size == 1 and self.st.ep_size == 1 and not self.lockstep
        self.kv_forks = self.kv_fork_fallbacks = self.kv_fork_shared_tokens = 0
        self.prompt_logprob_tokens = 0  # prompt-logprob entries computed (polykey_engine_prompt_logprob_tokens_total)
        if cfg.speculative:
            self.spec_k = cfg.num_speculative_tokens
            self.proposer = spec.NgramProposer(cfg.ngram_max, cfg.ngram_min)
            logging.getLogger(__name__).info(
                "speculative decoding: method %s, k %d, QR %d, verify graph buckets %s", cfg.speculative, self.spec_k,
                self.spec_k + 1, sorted(self.runner.verify_graphs) or "none (eager)")

    def _check_speculative(self, cfg: "EngineConfig", mcfg: ModelConfig) -> None:
        """What speculative decoding covers: dense Llama / Qwen3 on one GPU with a bf16 KV cache and
        k + 1 query rows that fit the verify attention's 16-column tile.  No silent fallback."""
        opt = f"speculative={cfg.speculative}"
        if cfg.speculative not in spec.METHODS:
            raise ValueError(f"speculative must be one of {', '.join(spec.METHODS)} (got {cfg.speculative!r})")
        if mcfg.is_moe:
            raise ValueError(f"{opt} does not support MoE models ({mcfg.name})")
        if self.st.tp_size > 1:
            raise ValueError(f"{opt} does not support tp={self.st.tp_size}")
        if self.st.ep_size > 1 or self.st.dp_attention:
            raise ValueError(f"{opt} does not support ep={self.st.ep_size} / DP attention")
        if cfg.lora_modules:
            raise ValueError(f"{opt} does not support LoRA adapters (lora_modules)")
        if cfg.kv_cache_dtype == "fp8":
            raise ValueError(f"{opt} does not support kv_cache_dtype=fp8: the verify attention reads a bf16 cache")
        k = cfg.num_speculative_tokens
        group = mcfg.num_heads // mcfg.num_kv_heads
        k_max = spec.max_draft_tokens(group)
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"num_speculative_tokens must be an integer >= 1 (got {k!r})")
        if k > k_max:
            raise ValueError(f"num_speculative_tokens={k} does not fit {mcfg.name}: (k + 1) x {group} query heads per "
                             f"kv head exceed the verify attention's {spec.VERIFY_COLUMNS} columns; the largest k for "
                             f"this model is {k_max}")
        if not 1 <= cfg.ngram_min <= cfg.ngram_max:
            raise ValueError(f"ngram_min / ngram_max must satisfy 1 <= min <= max (got {cfg.ngram_min}, {cfg.ngram_max})")

    def _load_adapters(self, model, mcfg: ModelConfig) -> None:
        from ..models.lora import MAX_SLOTS, LoraAdapter
        cfg = self.cfg
        if not hasattr(model, "enable_lora"):
            raise ValueError(f"LoRA adapters are not supported by {type(model).__name__}")
        if len(cfg.lora_modules) > MAX_SLOTS:
            raise ValueError(f"at most {MAX_SLOTS} LoRA adapters can be served by one engine "
                             f"(got {len(cfg.lora_modules)})")
        adapters = []
        for name, src in cfg.lora_modules:
            ad = src if isinstance(src, LoraAdapter) else LoraAdapter.load(str(src), mcfg, cfg.max_lora_rank)
            adapters.append((str(name), ad))
        state = model.enable_lora(adapters, cfg.max_lora_rank, max(cfg.max_num_batched_tokens, cfg.max_num_seqs))
        self.lora_names = list(state.names)
        self.lora_bytes = state.nbytes
        logging.getLogger(__name__).info("LoRA adapters: %d resident (%s), max rank %d, %d bytes",
                                         len(state.names), ", ".join(state.names), cfg.max_lora_rank, state.nbytes)

    def _serving_preflight(self, mcfg: ModelConfig) -> None:
        """TP: the fused decode collective checked at the shape serving will replay it at (the
        largest decode graph bucket x hidden, 16 back-to-back calls, graph-replayed) before any
        graph captures it; a mismatch switches the group to the fenced slot protocol or disables
        the custom collectives on every rank (parallel/preflight.py check_custom_ar_serving)."""
        car = self.st.custom_ar
        if car is None or self.st.tp_size < 2 or os.environ.get("POLYKEY_PREFLIGHT", "1") == "0":
            return
        rows = [g for g in self.runner.default_graph_sizes() if car.supports_reduce_residual(g, mcfg.hidden_size)]
        if rows:
            from ..parallel import preflight
            self.preflight_report = preflight.run(self.st, paths=("custom_ar_serving",),
                                                  serving=(max(rows), mcfg.hidden_size))

    # ------------------------------------------------------------------ API
    @property
    def is_leader(self) -> bool:
        return self.st.tp_rank == 0

    def add_request(self, prompt_ids: List[int], params: SamplingParams, request_id: Optional[str] = None,
                    user=None) -> Sequence:
        params.validate(self.cfg.max_model_len)
        if not prompt_ids:
            raise ValueError("empty prompt")
        if max(prompt_ids) >= self.mcfg.vocab_size or min(prompt_ids) < 0:
            raise ValueError("prompt token id out of range")
        if any(not 0 <= t < self.mcfg.vocab_size for t, _ in params.logit_bias):
            raise ValueError("logit_bias token id out of range")
        if params.lora is not None and params.lora not in self.lora_names:
            raise ValueError(f"unknown LoRA adapter {params.lora!r}: this engine serves "
                             f"{', '.join(self.lora_names) if self.lora_names else 'no adapters'}")
        if params.prompt_logprobs is not None:
            # the workers of a TP / EP group have no step message naming the rows (out of scope)
            if self.st.tp_size > 1:
                raise ValueError(f"prompt_logprobs does not support tp={self.st.tp_size}")
            if self.st.ep_size > 1 or self.lockstep:
                raise ValueError(f"prompt_logprobs does not support ep={self.st.ep_size} / DP attention")
        if params.n > self.cfg.max_num_seqs:
            raise ValueError(f"n must be at most max_num_seqs ({self.cfg.max_num_seqs}), got {params.n}")
        g = self._grammar(params)
        rid = request_id or uuid.uuid4().hex
        # parallel sampling: all n choices exist from here; choice 0 is queued, the others are parked
        # behind it until its prompt is computed (_fork).  -> choice 0 (``.choices`` holds them all)
        seqs = [Sequence(rid, prompt_ids, params, self.mcfg.eos_token_id, user, index=i) for i in range(params.n)]
        for seq in seqs:
            if params.n > 1:
                seq.choices = seqs
            if self.spec_k:
                seq.spec_drafted = seq.spec_accepted = 0
            seq.grammar = g
        try:
            if g is not None:  # the choices share the table; each holds its own reference to it
                for seq in seqs:
                    self.runner.acquire_grammar(seq)
            for seq in seqs:
                self.scheduler.add(seq, behind=seqs[0] if seq.index else None)
        except Exception:
            if self.scheduler.by_request.get(rid) is seqs[0]:
                self.scheduler.abort(rid)  # the choices already queued
            for seq in seqs:
                self.runner.release_grammar(seq)
            raise
        return seqs[0]

    def _grammar(self, params: SamplingParams):
        """The compiled constraint of a guided request (from the LRU), checked against this
        engine's vocabulary; ValueError for what cannot be served."""
        if not params.guided:
            return None
        V = self.mcfg.vocab_size
        if not 0 <= self.mcfg.eos_token_id < V:
            raise ValueError("guided decoding needs a model with an eos_token_id")
        if any(not 0 <= t < V for t in params.stop_token_ids):
            raise ValueError("stop_token_ids out of range")
        g = grammar.grammar_for(params)
        grammar.check_vocab(g, self._single_bytes)
        return g

    def abort(self, request_id: str) -> Optional[Sequence]:
        seq = self.scheduler.abort(request_id)
        if seq is not None and seq.prompt_logprobs is not None:
            seq.prompt_logprobs, seq.prompt_lp_missing = None, 0  # the entries gathered so far
        return seq

    def has_unfinished(self) -> bool:
        return self.scheduler.has_work() or self._inflight is not None

    def idle_with_waiting(self) -> bool:
        sch = self.scheduler
        return (not sch.running and self._inflight is None and bool(sch.waiting)
                and len(sch.waiting) < sch.max_num_seqs)

    def first_step_unfilled(self) -> bool:
        """Idle engine (nothing running or in flight) whose waiting requests do not yet fill one
        prefill step (token budget and sequence cap): a burst of arrivals may still be landing."""
        sch = self.scheduler
        if sch.running or self._inflight is not None or not sch.waiting:
            return False
        if len(sch.waiting) >= sch.max_num_seqs:
            return False
        return sum(s.num_pending for s in sch.waiting) < sch.max_num_batched_tokens

    def step(self) -> List[RequestOutput]:
        """One engine iteration.  With ``overlap`` the step is pipelined: the batch launched by
        the previous call is completed (wait for its sampled ids, advance sequence state, free
        finished sequences), the next batch is scheduled and launched, and only then are the
        completed batch's :class:`RequestOutput` objects built and returned — so output
        construction and the caller's delivery of them run while the GPU executes the next
        step.  Without ``overlap`` each call launches and completes its own batch."""
        if self.lockstep:
            return self._step_lockstep()
        done = None
        if self._inflight is not None:
            batch, sampling, handle = self._inflight
            nxt = self._continuation(batch, handle)
            done, redone = self._complete_or_redo(batch, sampling, handle)
            self._inflight = None
            if nxt is not None and not redone:  # a redone step's continuation ran on its bad tokens
                self._inflight = (batch, batch.decodes, nxt)
                self.continuation_steps += 1
                return self._outputs(done)
        if self.before_schedule is not None and done is not None:
            # requests that landed while the completed step ran join the next one (a burst whose
            # tail arrived during the first prefill step is prefilled in the second instead of a
            # straggler third step that delays the whole cohort by a prefill, profiles/r6_gc.md)
            self.before_schedule()
            # a request aborted by it loses the completed step's output too (as an abort while
            # a step is in flight does)
            done = [d for d in done if d[2] is not None or d[0].finish_reason is not FinishReason.ABORT]
        batch = self.scheduler.schedule()
        if self.spec_k:
            self._propose(batch)
        if not batch.empty:
            sampling = batch.sampling_seqs()
            self._inflight = (batch, sampling, self.runner.launch(batch))
            if not self.overlap:
                done, _ = self._complete_or_redo(*self._inflight)
                self._inflight = None
        return self._outputs(done) if done else []

    def _complete_or_redo(self, batch, sampling, handle):
        """``_complete`` of a launched step; if a fused decode launch of it lost its in-launch
        hand-off (FusedHandoffError: co-tenant on the GPU), the runner falls back to the
        two-launch path and the step is launched again -- the sequences' state is untouched until
        a step completes and the re-run rewrites the same KV slots.  A TP / lockstep group cannot
        re-run one rank alone, so TP ranks that share a GPU (where a co-tenant can starve a
        hand-off) never take the fused launches (models/llama.py _qkv_attn_fused_ok, the fused
        MLP's shared_device check); on a dedicated GPU a lost hand-off is a fault and stays fatal.
        Returns (done, redone)."""
        from ..ops.gemm import FusedHandoffError
        try:
            return self._complete(batch, sampling, handle), False
        except FusedHandoffError:
            if self.st.tp_size > 1 or self.lockstep:
                raise
            self.runner.fallback_unfused()  # drains the GPU: an in-flight continuation is finished
            return self._complete(batch, sampling, self.runner.launch(batch)), True

    def _step_lockstep(self) -> List[RequestOutput]:
        """DP attention + EP step: one lockstep vote (shared memory on one node) per step decides
        whether the EP group runs a forward and -- from the largest token count -- which expert
        all-to-all every rank uses (IPC slots, graph-capturable, for decode-sized steps; RCCL
        for prefill-sized ones); a rank with nothing scheduled joins through the idle pass."""
        from ..parallel import comm
        batch = self.scheduler.schedule()
        ntok = len(batch.decodes) + sum(n for _, n in batch.prefills)
        busy, _, max_tok = comm.ep_vote(not batch.empty, False, ntok)
        if not busy:
            return []
        # (graph buckets pad decode rows, but only buckets within the IPC capacity are captured)
        a2a = self.st.ep_a2a
        ipc = a2a is not None and a2a.fits(max_tok * self.mcfg.experts_per_token)
        # every rank sees the same max: the same regions (decode-sized, prefill-sized or none) on all
        self.st.ep_step_rows = max_tok
        self.runner.allow_graphs = ipc  # a replay holds the IPC path: only when every rank takes it
        if batch.empty:
            self.model.idle_forward()
            self.runner.stats["idle_steps"] = self.runner.stats.get("idle_steps", 0) + 1
            return []
        done = self._complete(batch, batch.sampling_seqs(), self.runner.launch(batch))
        return self._outputs(done)

    def lockstep_vote(self, stopping: bool):
        """DP attention + EP loop vote → (any rank has work, every rank is stopping)."""
        from ..parallel import comm
        busy, all_stop, _ = comm.ep_vote(self.has_unfinished(), stopping)
        return busy, all_stop

    def any_unfinished(self) -> bool:
        """Whether the engine loop must keep stepping: its own work, or (DP attention + EP) any
        rank's -- a collective vote every rank makes once per loop iteration."""
        local = self.has_unfinished()
        if not self.lockstep:
            return local
        from ..parallel import comm
        return comm.ep_any(local)

    def _continuation(self, batch, handle):
        """Launch the next decode step of ``batch`` before its current step has been read back
        (see ModelRunner.launch_continuation) when nothing else could change the batch: pure
        decode, every running sequence in it and alive, no request waiting for admission."""
        sch = self.scheduler
        if self.spec_k:  # the proposer needs the sampled tokens on the host before the next step is packed
            return None
        if (not self.overlap or batch.prefills or sch.waiting or len(batch.decodes) != len(sch.running)
                or any(s.is_finished() for s in batch.decodes)):
            return None
        if all(len(s.output_ids) + 1 >= s.params.max_tokens for s in batch.decodes):
            return None  # the in-flight step ends every sequence: a continuation would be discarded
        return self.runner.launch_continuation(batch, handle)

    def _propose(self, batch: ScheduledBatch) -> None:
        """After ``schedule()`` returned a pure-decode batch: ask the proposer for every sequence that
        may speculate and reserve KV for the drafts.  With at least one draft the batch becomes a
        verify step (``batch.drafts``); otherwise -- no draft, prefill in the batch, more rows than a
        decode step may have -- it stays today's step.  Drafts are clipped to k, to the tokens the
        request may still emit after this step's own, to the model length, and to what the KV pool
        grants: dropped one by one, never preempting anyone."""
        seqs = batch.decodes
        if batch.prefills or not seqs or len(seqs) > self.runner.verify_max_seqs:
            return
        k, bm, any_draft = self.spec_k, self.bm, False
        drafts: List[List[int]] = []
        for s in seqs:
            p = s.params
            room = min(k, p.max_tokens - len(s.output_ids) - 1, self.cfg.max_model_len - s.num_tokens - 1)
            d: List[int] = []
            if room > 0 and p.speculative is not False and not p.has_penalties and s.grammar is None:
                d = list(self.proposer.propose(s, room))[:room]
                while d and not bm.allocate(s.seq_id, s.num_computed + 1 + len(d)):
                    d.pop()
            drafts.append(d)
            any_draft = any_draft or bool(d)
        if any_draft:
            batch.drafts = drafts

    def _complete_verify(self, batch, handle):
        """A verify step read back.  Sequence i sampled rows ``i * QR + j``; ``n_acc`` is the number of
        leading drafts that equal the sample of the row before them, and the sequence emits samples
        ``0 .. n_acc`` -- one token at a time, stopping at the first finish reason -- and advances by
        ``1 + n_acc`` computed positions (the KV of rejected drafts lies beyond and is overwritten)."""
        toks = self.runner.fetch(handle)
        lp_rows = self.runner.fetch_logprobs(handle) if len(handle) > 4 and handle[4] is not None else None
        now = time.monotonic()
        qr = self.spec_k + 1
        done = []
        self.spec_steps += 1
        for i, (s, d) in enumerate(zip(batch.decodes, batch.drafts)):
            if s.is_finished():  # aborted while its step was in flight
                continue
            row = toks[i * qr:i * qr + 1 + len(d)]
            n_acc = 0
            while n_acc < len(d) and row[n_acc] == d[n_acc]:
                n_acc += 1
            s.num_computed += 1 + n_acc
            self._fork_if_prompt_done(s)
            s.spec_drafted += len(d)
            s.spec_accepted += n_acc
            self.spec_draft_tokens += len(d)
            self.spec_accepted_tokens += n_acc
            emitted, reason = [], None
            for j in range(n_acc + 1):
                if s.logprobs is not None:
                    s.logprobs.append(logprob_entry(lp_rows[i * qr + j], s.params.logprobs))
                emitted.append(row[j])
                reason = s.append_token(row[j], now)
                if reason is not None:
                    self.scheduler.finish(s, reason)
                    break
            done.append((s, emitted, reason))
            self.total_output_tokens += len(emitted)
        self.scheduler.remove_finished()
        self.step_count += 1
        return done

    def _complete(self, batch, sampling, handle):
        if batch.drafts is not None:
            return self._complete_verify(batch, handle)
        toks = self.runner.fetch(handle)
        # packed logprob rows in sampling order, fetched only when a sequence of the step asked
        lp_rows = self.runner.fetch_logprobs(handle) if len(handle) > 4 and handle[4] is not None else None
        for s, i, entry in self.runner.fetch_prompt_logprobs(handle):
            # (an entry is computed once: prompt_targets skips those on record, also in a recompute)
            if s.prompt_logprobs is not None and s.prompt_logprobs[i] is None:
                s.prompt_logprobs[i] = entry
                s.prompt_lp_missing -= 1
                self.prompt_logprob_tokens += 1
        now = time.monotonic()
        for s, n in batch.prefills:
            s.num_computed += n
            self.scheduler.commit_prefix(s)  # the step that wrote these blocks' KV has completed
            self._fork_if_prompt_done(s)
        for s in batch.decodes:
            s.num_computed += 1
            # (a prompt's last token runs as a decode row when one token is pending: a one-token
            # prompt, or a chunked prefill whose last chunk is one token)
            self._fork_if_prompt_done(s)
        done = []
        for r, (s, tok) in enumerate(zip(sampling, toks)):
            if s.is_finished():  # aborted while its step was in flight
                continue
            if s.logprobs is not None:
                s.logprobs.append(logprob_entry(lp_rows[r], s.params.logprobs))
            reason = s.append_token(tok, now)
            if reason is not None:
                self.scheduler.finish(s, reason)
            done.append((s, [tok], reason))
        self.scheduler.remove_finished()
        self.step_count += 1
        self.total_output_tokens += len(toks)
        return done

    def _fork_if_prompt_done(self, s: Sequence) -> None:
        """After ``s.num_computed`` advanced and before the step's token is appended (``s`` may finish
        in this very step): release the choices parked behind ``s`` once its prompt is computed,
        whichever list of the batch its last prompt token ran in."""
        if self.scheduler.parked and s.seq_id in self.scheduler.parked and s.num_computed >= len(s.prompt_ids):
            self._fork(s)

    def _fork(self, leader: Sequence) -> None:
        """Choice 0's prompt is computed: its parked siblings take the KV of its first P - 1 tokens --
        the (P - 1) // bs full blocks by reference, the partial block (if any) by one copy launch for
        all of them -- and go to the front of ``waiting`` with one pending token: each recomputes the
        last prompt token as a one-row step and samples its own first token there.  Shared blocks
        are never written again (every later write is at a position >= P - 1, in the private block or
        beyond); the copied block's bytes beyond slot (P - 1) % bs are overwritten before any read.
        A choice the pool cannot grant its block, or an engine without the fork (kv_fork off, TP /
        EP), leaves the choices plain waiting sequences: full prefill, prefix cache as usual."""
        m = len(leader.prompt_ids) - 1
        pairs, forked = [], 0
        parked = self.scheduler.release_parked(leader)  # (an aborted request has none left)
        if self.kv_fork and m > 0:
            for c in parked:
                got = self.bm.fork(leader.seq_id, c.seq_id, m)
                if got is None:
                    break  # no free block: this choice and the rest prefill
                pairs += got
                c.num_computed = c.forked_tokens = m
                forked += 1
        if pairs:
            self.runner.copy_kv_blocks(pairs)
        if forked:
            self.kv_forks += 1
            self.kv_fork_shared_tokens += forked * m
        if forked < len(parked):
            self.kv_fork_fallbacks += 1

    @staticmethod
    def _outputs(done) -> List[RequestOutput]:
        outs = []
        for s, toks, reason in done:
            out = RequestOutput(s.request_id, toks, reason is not None, reason.value if reason else None,
                                len(s.prompt_ids), len(s.output_ids), seq_metrics(s) if reason else None,
                                index=s.index, logprobs=s.logprobs[-len(toks):] if s.logprobs is not None else None)
            if s.prompt_logprobs is not None and not s.prompt_lp_delivered:
                # once, with the first generated token (the prompt is computed: every entry exists)
                out.prompt_logprobs = list(s.prompt_logprobs)
                s.prompt_lp_delivered = True
            outs.append(out)
        return outs

    def generate(self, prompts: List[List[int]], params: SamplingParams) -> List[List[int]]:
        seqs = [self.add_request(p, dataclasses.replace(params)) for p in prompts]
        while self.any_unfinished():
            self.step()
        return [s.output_ids for s in seqs]

    def shutdown(self) -> None:
        self.runner.stop_workers()
