"""Model runner: step inputs → device, forward, logits, sampling; HIP graphs for decode.

Per step the CPU work is one native call (``BlockManager.pack_step`` writes token ids,
positions, slot mapping, block tables, context lengths and query offsets into a pinned
int32 staging buffer), one H2D copy of that buffer, the forward, and one D2H copy of the
sampled ids.  The device-side copy of the staging buffer has fixed section offsets, so its
views are stable and a decode step can be *captured once per batch-size bucket* and replayed
with ``hipGraphLaunch`` (torch.cuda.CUDAGraph on ROCm) — the launch-bound decode loop of
32–80 layers × ~10 kernels collapses into one graph launch (guide: "capture launch-bound
inner loops in hipGraphs").

Tensor parallelism: the TP leader schedules; every other rank of its group runs
:meth:`ModelRunner.worker_loop`.  The leader publishes each step's packed staging bytes (header
included) through a shared-memory ring (``_pk_runtime.StepChannel``, csrc/runtime/step_channel.h);
a worker copies them into its own pinned staging buffer, reads the header on the host and
launches the same graph / kernels at once — no collective and no GPU sync per step on the
control plane.  Decode continuations replicate on workers too: every rank samples the same ids
from the all-gathered logits, so a worker feeds its own previous sampled ids forward.

KV cache: one allocation per layer pair, K ``[blocks, n_kv, bs, 128]`` and transposed V
``[blocks, n_kv, 128, bs]`` (see ops/attention.py), sized from free HBM after weights and
a measured activation peak — at 288 GB per MI355X an 8B model gets ~1.9 M cached tokens.
"""
from __future__ import annotations

import contextlib
import dataclasses
import logging
import math
import os
import sys
import threading
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..ops import attention as attn_ops
from ..ops import gemm
from ..ops import native
from ..ops import grammar as gram_ops
from ..ops import kv as kv_ops
from ..ops import penalties as pen_ops
from ..ops import sampler as sampler_ops
from .scheduler import ScheduledBatch
from .sequence import Sequence


@contextlib.contextmanager
def _capture(graph: "torch.cuda.CUDAGraph", pool=None):
    """``torch.cuda.graph(graph, pool=pool)`` for a body that runs under inference mode, begun
    outside it.  Beginning a capture registers the graph with the process-wide CUDA generator, and
    the first graph registered creates the generator's graph-state tensors, which live as long as
    any graph does and which every later capture in the process updates in place.  Created under
    inference mode they are inference tensors, and a capture begun outside inference mode (another
    library, a test) while an engine's graphs are still alive then fails, leaving the generator in
    its capturing state.  Begun here, they are ordinary tensors whoever creates them."""
    cm = torch.cuda.graph(graph, pool=pool)
    with torch.inference_mode(False):
        cm.__enter__()
    try:
        yield
    except BaseException:
        if not cm.__exit__(*sys.exc_info()):
            raise
    else:
        cm.__exit__(None, None, None)


@dataclasses.dataclass
class RunnerConfig:
    block_size: int = 32
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 8192
    num_kv_blocks: int = 0           # 0 → size from free memory
    gpu_mem_fraction: float = 0.90
    hip_graphs: bool = True
    graph_batch_sizes: Tuple[int, ...] = ()
    kv_cache_dtype: str = "bf16"     # "bf16" (the model dtype) | "fp8" (OCP e4m3 + per-layer scales)
    # speculative decoding: query rows per sequence of a verify step (k drafts + 1); 0 = off, and
    # then nothing below differs from a runner that never heard of it
    spec_qr: int = 0


# Long-context decode merges its partitions in a second kernel (an in-kernel last-arriver merge
# needs an agent-scope release per partition and measured 1.7-1.9x slower at 1-4K contexts,
# tools/bench_attn.py).  Step inputs are staged by a kernel reading pinned memory instead of an
# SDMA copy.  Each decode bucket has a second graph for steps whose contexts all fit one attention
# partition (one workgroup per (seq, kv head), no merge kernel).


# Prompt logprobs (SamplingParams.prompt_logprobs): the LM head runs over the asked prompt rows of a
# prefill step in chunks of at most this many rows, so the logits it materialises stay bounded
# (256 x V_padded x 2 bytes: 66 MB at V = 128,256) however long the prompt chunk is.
PROMPT_LP_CHUNK_ROWS = 256


def prompt_targets(chunks) -> List[int]:
    """The prompt-logprob target of every row of a step.  ``chunks``: the step's scheduled
    ``(seq, start, length)`` in row order (a decode row is a chunk of length 1).  The row at
    position ``p`` of a sequence that asks gets ``prompt_ids[p + 1]`` -- the token its logits
    predict, taken from the prompt itself, so the last row of a non-final chunk has its target
    too -- when ``p + 1`` is still inside the prompt and entry ``p + 1`` is not on record yet;
    every other row (decode rows, the prompt's last row, rows of sequences that do not ask, rows of
    a recompute whose entries exist) gets -1."""
    out: List[int] = []
    for seq, start, length in chunks:
        rec = seq.prompt_logprobs
        if rec is None or not seq.prompt_lp_missing:
            out += [-1] * length
            continue
        ids, P = seq.prompt_ids, len(seq.prompt_ids)
        out += [ids[p + 1] if p + 1 < P and rec[p + 1] is None else -1 for p in range(start, start + length)]
    return out


class _Layout:
    """Fixed offsets of every per-step int32 section inside one staging buffer."""

    def __init__(self, max_tokens: int, max_seqs: int, max_blocks: int, lora: bool = False, max_samples: int = 0):
        self.max_tokens, self.max_seqs, self.max_blocks = max_tokens, max_seqs, max_blocks
        off = 0
        self.sections = {}
        # max_samples > 0 (speculative decoding): a verify step samples every row of every sequence,
        # so the per-sampling-row sections hold that many rows, and "verify_rows" holds the real rows
        # of each sequence; 0: one sampling row per sequence, today's sizes and offsets
        ms = max(max_samples, max_seqs)
        # "lora_idx": the adapter slot of every TOKEN row (-1: none); only with adapters configured
        for name, n in (("header", 16), ("input_ids", max_tokens), ("positions", max_tokens), ("slots", max_tokens),
                        ("context_lens", max_seqs), ("cu_q", max_seqs + 1), ("cu_rel", max_seqs + 1), ("sample_idx", ms),
                        ("temperature", ms), ("top_k", ms), ("top_p", ms), ("min_p", ms),
                        ("seeds", ms), ("offsets", ms), ("pen_slot", ms), ("rep", ms),
                        ("freq", ms), ("pres", ms), ("logprobs", ms),
                        *((("verify_rows", max_seqs),) if max_samples else ()),
                        *((("lora_idx", max_tokens),) if lora else ()),
                        ("block_tables", max_seqs * max_blocks)):
            self.sections[name] = (off, n)
            off += (n + 15) // 16 * 16  # 64-byte aligned sections
        self.size = off

    def view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        off, n = self.sections[name]
        v = buf[off:off + n]
        if name in ("temperature", "top_p", "min_p", "rep", "freq", "pres"):
            v = v.view(torch.float32)
        if name == "block_tables":
            v = v.view(self.max_seqs, self.max_blocks)
        return v


class TPPeerError(RuntimeError):
    """A rank of this TP group died or stopped responding: the group cannot continue."""


def peer_timeout_ms() -> int:
    """Bound of every wait on a TP peer (step ring slot, IPC collective): POLYKEY_CUSTOM_AR_TIMEOUT_S."""
    return int(float(os.environ.get("POLYKEY_CUSTOM_AR_TIMEOUT_S", "30")) * 1000)


class ModelRunner:
    def __init__(self, model, cfg: RunnerConfig, device: torch.device, block_manager=None):
        self.model = model
        self.bm = block_manager
        self.mcfg = model.cfg
        self.cfg = cfg
        self.device = device
        self.bs = cfg.block_size
        self.max_blocks = (cfg.max_model_len + self.bs - 1) // self.bs
        self.max_step_tokens = cfg.max_num_batched_tokens  # decodes count toward the budget
        # resident LoRA adapters (models/lora.py LoraState; the engine enables them on the model
        # before it builds the runner): a per-token slot section and a LoRA variant of every graph
        self.lora = getattr(model, "lora", None)
        # speculative decoding: a verify step holds spec_qr rows per sequence, at most as many rows
        # as a decode step may have (the decode chain's row limit, the token budget)
        self.spec_qr = int(cfg.spec_qr)
        self.verify_max_seqs = (min(cfg.max_num_seqs, min(gemm.DECODE_MAX_M, self.max_step_tokens) // self.spec_qr)
                                if self.spec_qr else 0)
        max_samples = max(cfg.max_num_seqs, self.verify_max_seqs * self.spec_qr) if self.spec_qr else 0
        self.layout = _Layout(self.max_step_tokens, cfg.max_num_seqs, self.max_blocks, lora=self.lora is not None,
                              max_samples=max_samples)
        n_samp = max_samples or cfg.max_num_seqs  # sampling rows of the largest step
        pin = device.type == "cuda"
        # two pinned staging buffers used alternately: a step may be packed while the previous
        # step's H2D copy is still queued behind the GPU (continuation launches, LLMEngine.step)
        self._host_bufs = [torch.zeros(self.layout.size, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._hs = [{k: self.layout.view(b, k).numpy() for k in self.layout.sections} for b in self._host_bufs]
        self._hnp = [b.numpy() for b in self._host_bufs]  # whole-buffer views (step channel I/O)
        self._h2d_events = [None, None]
        self._cur = 0
        self.host_buf, self.h = self._host_bufs[0], self._hs[0]
        self.dev_buf = torch.zeros(self.layout.size, dtype=torch.int32, device=device)
        self.d = {k: self.layout.view(self.dev_buf, k) for k in self.layout.sections}
        if self.lora is not None:
            self.lora.idx = self.d["lora_idx"]  # the kernels read the staged section itself
        self._step_lora = 0  # the step being packed has a row with an adapter
        self._tok_hosts = [torch.zeros(n_samp, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._tok_events = [None, None]
        # per-token logprobs (ops/sampler.py logprobs): one packed record per sampling row, written
        # by the kernel right after the sampler (inside every decode graph); rows whose request did
        # not ask (section "logprobs" = -1) cost one early-returning workgroup.  The host copies
        # pair with _tok_hosts and are fetched only for steps in which some sequence asked.
        self.lp_dev = torch.zeros((n_samp, sampler_ops.LOGPROB_WORDS), dtype=torch.int32, device=device)
        self._lp_hosts = [torch.zeros((n_samp, sampler_ops.LOGPROB_WORDS), dtype=torch.int32,
                                      pin_memory=pin) for _ in range(2)]
        self._tok_i = 0
        # prompt logprobs: device records for the asked rows of one step, and their inputs (row
        # index, target id, list length per asked row) in a small pinned buffer of their own, copied
        # only in steps that have such a row -- the staging layout above and the step-channel frame
        # are what they were.  Both are double-buffered like the sampled ids.  Their bytes are reserved
        # here, before the KV cache is sized (activation_reserve_bytes); the buffers themselves are made
        # by the first step that needs them (_prompt_lp_buffers), so an engine that never scores a
        # prompt makes the allocations of an engine without the feature, one for one.
        W = sampler_ops.PROMPT_LOGPROB_WORDS
        self.plp_dev = self.plp_in_dev = self._plp_in_hosts = self._plp_hosts = None
        self._plp_events = [None, None]
        self._plp_i = 0
        self._plp = None      # launch -> _run: (asked rows, owners) of the step being launched
        self._plp_out = None  # _run -> launch: (host records, rows, owners, event)
        # (bytes of one chunk's logits -- reserved before the KV cache is sized -- , bytes of records)
        self.prompt_lp_bytes = (PROMPT_LP_CHUNK_ROWS * self.mcfg.vocab_size * model.dtype.itemsize,
                                (self.max_step_tokens * W + 3 * self.max_step_tokens) * 4)
        logging.getLogger(__name__).info(
            "prompt logprobs: %d bytes of logits per %d-row LM-head chunk, %d bytes of records (%d rows x %d words)",
            self.prompt_lp_bytes[0], PROMPT_LP_CHUNK_ROWS, self.prompt_lp_bytes[1], self.max_step_tokens, W)
        # sampling penalties / logit_bias (ops/penalties.py): device-resident token history, one
        # slot per penalised sequence, allocated before the KV cache is sized.  A sequence gets
        # its slot the first time it samples (launch) and loses it when the scheduler frees its
        # blocks (release_penalty_slot).  Invariant: a freed slot may still receive the update of
        # a discarded in-flight continuation (or of the step that finished its sequence); that is
        # safe because whoever takes the slot next is seeded with clear = 1 by a launch enqueued
        # later on the same stream, and nothing reads a slot before its seed.
        self.pen = pen_ops.PenaltyState(cfg.max_num_seqs, self.mcfg.vocab_size, device)
        self._pen_slot: Dict[int, int] = {}                       # seq_id -> slot
        self._pen_free: List[int] = list(range(cfg.max_num_seqs - 1, -1, -1))
        self._pen_stale: set = set()                              # seq ids to re-seed from host truth
        # guided decoding (ops/grammar.py): a byte DFA per constrained sequence, masked into the
        # penalty slot's fp32 row and advanced on the device.  A guided sequence takes a penalty
        # slot even with neutral penalties; its table and its slot record are (re-)seeded at the
        # same points as the token history.  Tables are shared by grammar hash and refcounted by
        # live sequences; an unreferenced one stays until its pool entry is needed.
        self.gram: Optional[gram_ops.GrammarState] = None         # init_grammar
        self._gram_key: List[Optional[str]] = [None] * gram_ops.N_TABLES  # pool entry -> grammar hash
        self._gram_ref: List[int] = [0] * gram_ops.N_TABLES
        self._gram_used: List[int] = [0] * gram_ops.N_TABLES      # last-use tick per entry (eviction order)
        self._gram_tick = 0
        self._gram_loaded: set = set()                            # entries whose words are on the device
        self._gram_seq: Dict[int, int] = {}                       # seq_id -> the entry it references
        self._gram_slots: set = set()                             # slots whose device record names a table
        self.live_requests: Optional[dict] = None                 # Scheduler.by_request (LLMEngine)
        self.kv_caches: List[Tuple[torch.Tensor, torch.Tensor]] = []
        self.num_blocks = 0
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.graph_out: Dict[int, torch.Tensor] = {}
        self.short_graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.short_graph_out: Dict[int, torch.Tensor] = {}
        # LoRA variants of both, captured only with adapters configured; a step replays them when
        # one of its decode rows has an adapter, today's graphs otherwise
        self.lora_graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.lora_graph_out: Dict[int, torch.Tensor] = {}
        self.lora_short_graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.lora_short_graph_out: Dict[int, torch.Tensor] = {}
        self.short_ctx = attn_ops._PART if cfg.max_model_len > attn_ops._PART else 0
        self.graph_pool = None
        a0 = model.layers[0].attn
        self.part_o, self.part_ml = attn_ops.decode_workspace(cfg.max_num_seqs, a0.nq, self.max_blocks, self.bs, device,
                                                              kv_heads=a0.nkv)
        self.stats = {"steps": 0, "graph_steps": 0, "short_graph_steps": 0, "tokens": 0, "seed_msgs": 0,
                      "lora_steps": 0, "lora_graph_steps": 0, "prompt_lp_rows": 0, "prompt_lp_steps": 0}
        # verify steps of speculative decoding: graphs per sequence-count bucket (captured only when
        # configured) and partition slabs for verify_max_seqs x spec_qr rows
        self.verify_graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.verify_graph_out: Dict[int, torch.Tensor] = {}
        self.vpart_o = self.vpart_ml = None
        if self.spec_qr:
            self.vpart_o, self.vpart_ml = attn_ops.verify_workspace(self.verify_max_seqs, self.spec_qr, a0.nq,
                                                                    self.max_blocks, self.bs, device, kv_heads=a0.nkv)
            self.stats.update(verify_steps=0, verify_graph_steps=0)
        self.keep_logits = False  # tests: keep the last eager step's logits
        self.last_logits = None
        # diagnostics (tools/tp_rehearsal.py): every step's logits, graphed steps included (a copy
        # captured into each graph); read last_logits right after the step, before the next one
        self.debug_logits = os.environ.get("POLYKEY_DEBUG_LOGITS") == "1"
        self._graph_logits: Dict[Tuple[int, int], torch.Tensor] = {}
        self.channel = None
        self._prev_toks = None  # worker: last step's sampled ids (device), for continuations
        self.allow_graphs = True  # DP attention + EP: False for steps whose expert all-to-all is not IPC
        if model.st.tp_size > 1:
            self._open_channel()

    # ------------------------------------------------------------- TP control plane
    def _open_channel(self) -> None:
        """Leader creates the step ring in /dev/shm and tells its group the name (one gloo
        broadcast at start-up); workers attach as consumers tp_rank - 1."""
        import uuid

        from .._native.loader import load_extension
        from ..parallel import comm
        st = self.model.st
        rt = load_extension("_pk_runtime")
        slot_bytes = self.layout.size * 4
        if st.tp_rank == 0:
            name = f"/pk_step_{os.getpid()}_{st.dp_rank}_{uuid.uuid4().hex[:8]}"
            self.channel = rt.StepChannel(name, True, 4, st.tp_size - 1, slot_bytes)
            comm.tp_broadcast_object(name)
        else:
            name = comm.tp_broadcast_object(None)
            self.channel = rt.StepChannel(name, False, consumer_index=st.tp_rank - 1)
        comm.barrier(st.tp_cpu_group)  # every consumer attached before the first publish
        if st.tp_rank == 0:
            self.channel.unlink()  # nothing left in /dev/shm if the group is killed

    # ---------------------------------------------------------------- KV cache
    def kv_dtype(self) -> torch.dtype:
        """Element type of the paged caches: the model's, or e4m3 for ``kv_cache_dtype="fp8"``."""
        if self.cfg.kv_cache_dtype == "fp8":
            return attn_ops.FP8
        if self.cfg.kv_cache_dtype not in ("bf16", "auto"):
            raise ValueError(f"kv_cache_dtype must be one of auto, bf16, fp8 (got {self.cfg.kv_cache_dtype!r})")
        return self.model.dtype

    def kv_bytes_per_block(self) -> int:
        a = self.model.layers[0].attn
        return 2 * len(self.model.layers) * a.nkv * self.bs * a.hd * self.kv_dtype().itemsize

    def allocate_kv_cache(self, num_blocks: int = 0) -> int:
        a = self.model.layers[0].attn
        if num_blocks <= 0:
            num_blocks = self.cfg.num_kv_blocks
        if num_blocks <= 0:
            # a byte budget: a cache of narrower elements gets that many times the blocks (FP8: 2x)
            ratio = max(1, self.model.dtype.itemsize // self.kv_dtype().itemsize)
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
                free, total = torch.cuda.mem_get_info(self.device)
                reserve = self.activation_reserve_bytes()
                usable = free - (1.0 - self.cfg.gpu_mem_fraction) * total - reserve
                num_blocks = int(max(usable, 0) // (self.kv_bytes_per_block() * ratio))
                cap = self.cfg.max_num_seqs * self.max_blocks + 16
                num_blocks = max(16, min(num_blocks, cap)) * ratio
            else:
                num_blocks = max(16, min(self.cfg.max_num_seqs * self.max_blocks, 4096)) * ratio
        self.num_blocks = num_blocks
        self.kv_caches = []
        dt = self.kv_dtype()
        # (every TP rank allocates the same dtype: the ranks build their runner from one engine
        # config; the model routes around its bf16-only launches by the dtype of these tensors)
        raw = torch.uint8 if dt == attn_ops.FP8 else dt
        for _ in self.model.layers:
            k = torch.zeros((num_blocks, a.nkv, self.bs, a.hd), dtype=raw, device=self.device).view(dt)
            v = torch.zeros((num_blocks, a.nkv, a.hd, self.bs), dtype=raw, device=self.device).view(dt)
            self.kv_caches.append((k, v))
        self.kv_ptr_table = kv_ops.pointer_table(self.kv_caches)  # the block copy's 2 x layers base pointers
        return num_blocks

    def copy_kv_blocks(self, pairs) -> None:
        """Block dst := block src in K and V of every layer for the (src, dst) pairs of a prompt fork
        (LLMEngine._fork): one eager launch on the stream the steps run on, ordered after the
        prefill that wrote the sources and before the step that reads the copies; no host wait,
        never captured."""
        kv_ops.copy_blocks(self.kv_caches, pairs, self.kv_ptr_table)  # n <= 16: at most 15 pairs
        self.stats["kv_copy_launches"] = self.stats.get("kv_copy_launches", 0) + 1

    def activation_reserve_bytes(self) -> int:
        m = self.mcfg
        T = self.max_step_tokens
        tp = self.model.st.tp_size
        per_tok = 2 * (m.hidden_size * 4 + (m.q_size + 2 * m.kv_size) // tp + 3 * m.intermediate_size // tp)
        logits = self.cfg.max_num_seqs * m.vocab_size * 4 * 2
        # (+ one LM-head chunk of prompt-logprob logits and the record / target buffers, made on first use)
        return int(T * per_tok * 1.5 + logits + sum(self.prompt_lp_bytes) + (1 << 30))

    # ------------------------------------------------------------------ inputs
    def _pack(self, batch: ScheduledBatch, sampling: List[Sequence]):
        decodes, prefills = batch.decodes, batch.prefills
        seqs = decodes + [s for s, _ in prefills]
        n = len(seqs)
        nnew = np.empty(n, dtype=np.int32)
        ncomp = np.empty(n, dtype=np.int32)
        sids = np.empty(n, dtype=np.int64)
        toks: List[int] = []
        for i, s in enumerate(decodes):
            sids[i], ncomp[i], nnew[i] = s.seq_id, s.num_computed, 1
            toks.append(s.output_ids[-1] if s.output_ids else s.prompt_ids[-1])
        for j, (s, c) in enumerate(prefills):
            i = len(decodes) + j
            sids[i], ncomp[i], nnew[i] = s.seq_id, s.num_computed, c
            toks.extend(s.token_slice(s.num_computed, s.num_computed + c))
        tok_arr = np.asarray(toks, dtype=np.int32)
        h = self.h
        T = self.bm.pack_step(sids, ncomp, nnew, tok_arr, h["input_ids"], h["positions"], h["slots"],
                              h["block_tables"], self.max_blocks, h["context_lens"], h["cu_q"])
        if self.lora is not None:
            self._fill_lora(seqs, T)
        # sampling rows: hidden-state row index of each sampling sequence
        pos_of = {s.seq_id: int(h["cu_q"][i + 1]) - 1 for i, s in enumerate(seqs)}
        h["logprobs"][:len(sampling)] = -1  # rows that ask overwrite theirs below
        self._neutral_penalties(len(sampling))
        pen = self._pen_slot  # empty unless a live sequence is penalised
        want_lp = False
        for r, s in enumerate(sampling):
            p = s.params
            h["sample_idx"][r] = pos_of[s.seq_id]
            if pen and s.seq_id in pen:
                self._fill_penalties(r, s)
            h["temperature"][r] = p.temperature
            h["top_k"][r] = p.top_k
            h["top_p"][r] = p.top_p
            h["min_p"][r] = p.min_p
            h["seeds"][r] = s.seed
            h["offsets"][r] = len(s.output_ids)
            if p.logprobs is not None:
                h["logprobs"][r] = p.logprobs
                want_lp = True
        return T, n, want_lp

    def _pack_verify(self, batch: ScheduledBatch):
        """A verify step (speculative decoding): sequence i owns the ``qr`` rows ``i * qr + j``.  Rows
        ``j < R = 1 + len(drafts)`` carry [last token, drafts...] at positions ``num_computed + j`` with
        their KV slots; the rest are padding (token 0, position 0, slot -1).  Every row samples, with
        its sequence's parameters and ``offset = len(output_ids) + j``; penalty, grammar and logprob
        fields sit on row 0 of a sequence without drafts (the only ones that have them) or are neutral.
        -> (T, n, want_lp)"""
        seqs, drafts, qr = batch.decodes, batch.drafts, self.spec_qr
        n = len(seqs)
        T = n * qr
        sids = np.fromiter((s.seq_id for s in seqs), dtype=np.int64, count=n)
        ncomp = np.fromiter((s.num_computed for s in seqs), dtype=np.int32, count=n)
        nnew = np.fromiter((1 + len(d) for d in drafts), dtype=np.int32, count=n)
        toks: List[int] = []
        for s, d in zip(seqs, drafts):
            toks.append(s.output_ids[-1] if s.output_ids else s.prompt_ids[-1])
            toks.extend(d)
        R_all = len(toks)
        ids, pos, slot = (np.empty(R_all, dtype=np.int32) for _ in range(3))
        h = self.h
        self.bm.pack_step(sids, ncomp, nnew, np.asarray(toks, dtype=np.int32), ids, pos, slot, h["block_tables"],
                          self.max_blocks, h["context_lens"], h["cu_q"])
        cu = h["cu_q"][:n + 1].astype(np.int64)
        dest = np.repeat(np.arange(n, dtype=np.int64) * qr - cu[:-1], nnew) + np.arange(R_all, dtype=np.int64)
        h["input_ids"][:T] = 0
        h["positions"][:T] = 0
        h["slots"][:T] = -1
        h["input_ids"][dest] = ids
        h["positions"][dest] = pos
        h["slots"][dest] = slot
        h["verify_rows"][:n] = nnew
        h["sample_idx"][:T] = np.arange(T, dtype=np.int32)
        h["logprobs"][:T] = -1
        self._neutral_penalties(T)
        # per-sequence sampling parameters, repeated over the sequence's qr rows
        ps = [s.params for s in seqs]
        for name, dt, vals in (("temperature", np.float32, [p.temperature for p in ps]),
                               ("top_k", np.int32, [p.top_k for p in ps]), ("top_p", np.float32, [p.top_p for p in ps]),
                               ("min_p", np.float32, [p.min_p for p in ps]), ("seeds", np.int32, [s.seed for s in seqs])):
            h[name][:T] = np.repeat(np.asarray(vals, dtype=dt), qr)
        h["offsets"][:T] = (np.repeat(np.fromiter((len(s.output_ids) for s in seqs), dtype=np.int32, count=n), qr)
                            + np.tile(np.arange(qr, dtype=np.int32), n))
        pen = self._pen_slot
        want_lp = False
        for i, s in enumerate(seqs):
            if pen and s.seq_id in pen:  # (no drafts: one real row)
                self._fill_penalties(i * qr, s)
            if ps[i].logprobs is not None:
                h["logprobs"][i * qr:i * qr + int(nnew[i])] = ps[i].logprobs
                want_lp = True
        return T, n, want_lp

    def _pad_verify(self, n: int, g: int) -> None:
        """Sequences n..g of a verify graph bucket: no context, every row padding."""
        if g <= n:
            return
        h, qr = self.h, self.spec_qr
        a, b = n * qr, g * qr
        h["input_ids"][a:b] = 0
        h["positions"][a:b] = 0
        h["slots"][a:b] = -1
        h["context_lens"][n:g] = 0
        h["verify_rows"][n:g] = 1
        h["sample_idx"][a:b] = np.arange(a, b, dtype=np.int32)
        h["temperature"][a:b] = 0.0
        h["top_k"][a:b] = 0
        h["top_p"][a:b] = 1.0
        h["min_p"][a:b] = 0.0
        h["logprobs"][a:b] = -1
        h["pen_slot"][a:b] = -1

    def _verify_metadata(self, n: int) -> attn_ops.AttnMetadata:
        """Outside attention a verify step is a decode step of n * qr rows; its attention reads the
        per-sequence block tables, contexts and real-row counts, at the block-table capacity bound
        (eager and replayed steps take the same partition plan)."""
        d, qr = self.d, self.spec_qr
        T = n * qr
        return attn_ops.AttnMetadata(
            num_decode=T, num_prefill=0, num_prefill_tokens=0, max_prefill_q_len=0, slot_mapping=d["slots"][:T],
            decode_part_o=self.vpart_o, decode_part_ml=self.vpart_ml, decode_max_ctx=0, verify_qr=qr,
            verify_rows=d["verify_rows"][:n], verify_block_tables=d["block_tables"][:n],
            verify_context_lens=d["context_lens"][:n])

    def launch_verify(self, batch: ScheduledBatch):
        """:meth:`launch` of a pure-decode batch whose sequences carry drafts (``batch.drafts``): one
        verify step, replayed from the verify graph of the sequence-count bucket when captured."""
        self._seed_penalties(batch.decodes)
        self._next_staging()
        T, n, want_lp = self._pack_verify(batch)
        g = 0
        if self.verify_graphs and self.allow_graphs:
            g = next((b for b in sorted(self.verify_graphs) if b >= n), 0)
            self._pad_verify(n, g)
        qr = self.spec_qr
        h = self.h
        if self.lora is not None:  # (the engine refuses the combination; rows stay base rows)
            h["lora_idx"][:max(n, g) * qr] = -1
        h["header"][:11] = (self.MODE_RUN, T, n, T, T, 0, g, 0, 0, 0, qr)
        self._publish(max(n, g))
        toks = self._run(T, n, T, T, 0, g, 0, 0, qr)
        return self._handle(toks, T, want_lp)

    # ------------------------------------------------------------------ LoRA
    def _fill_lora(self, seqs: List[Sequence], T: int) -> None:
        """Section "lora_idx": the adapter slot of every token row of the packed step (the rows of
        sequence i are cu_q[i] .. cu_q[i + 1]), -1 for base rows.  Sets ``_step_lora``."""
        h = self.h
        li, cu = h["lora_idx"], h["cu_q"]
        li[:T] = -1
        any_lora = 0
        slot_of = self.lora.slot_of
        for i, s in enumerate(seqs):
            name = s.params.lora
            if name is not None:
                li[int(cu[i]):int(cu[i + 1])] = slot_of[name]
                any_lora = 1
        self._step_lora = any_lora

    # ------------------------------------------------------------------ penalties
    def _neutral_penalties(self, n: int) -> None:
        """One vectorised neutral write per step; only rows that ask are overwritten.  Slot -1 is
        the whole neutral state: ``rep`` / ``freq`` / ``pres`` are read for rows with a slot only."""
        self.h["pen_slot"][:n] = -1

    def _fill_penalties(self, r: int, s: Sequence) -> None:
        h, p = self.h, s.params
        h["pen_slot"][r] = self._pen_slot[s.seq_id]
        h["rep"][r] = p.repetition_penalty
        h["freq"][r] = p.frequency_penalty
        h["pres"][r] = p.presence_penalty

    def release_penalty_slot(self, seq: Sequence) -> None:
        """Scheduler.on_free: the sequence's blocks were freed (finish, abort, preemption).  A
        sequence that will not run again (finished, or aborted: no longer in the scheduler's
        registry ``live_requests``) drops its reference to a grammar table too; a preempted one
        keeps it for its readmission."""
        slot = self._pen_slot.pop(seq.seq_id, None)
        self._pen_stale.discard(seq.seq_id)
        if slot is not None:
            self._pen_free.append(slot)
        live = self.live_requests
        if seq.is_finished() or (live is not None and live.get(seq.key) is not seq):
            self.release_grammar(seq)

    # ------------------------------------------------------------------ guided decoding
    def init_grammar(self, off: np.ndarray, data: np.ndarray) -> None:
        """The vocabulary's byte table (engine/grammar.py token_bytes), once, before the KV cache is
        sized and before graphs are captured: from here on every sampling step masks and advances."""
        self.gram = gram_ops.GrammarState(self.cfg.max_num_seqs, off, data, self.device)

    def acquire_grammar(self, seq: Sequence) -> None:
        """LLMEngine.add_request: ``seq.grammar`` gets a pool entry (shared by hash) and holds a
        reference to it until the sequence ends."""
        key = seq.grammar.key
        n = gram_ops.N_TABLES
        entry = next((i for i in range(n) if self._gram_key[i] == key), None)
        if entry is None:
            idle = [i for i in range(n) if self._gram_ref[i] == 0]
            if not idle:
                raise ValueError(f"all {n} grammar tables are held by live sequences: at most {n} distinct "
                                 "guided_regex / guided_choice / guided_json constraints can be live at once")
            entry = min(idle, key=lambda i: (self._gram_key[i] is not None, self._gram_used[i]))
            self._gram_key[entry] = key
            self._gram_loaded.discard(entry)
        self._gram_ref[entry] += 1
        self._gram_tick += 1
        self._gram_used[entry] = self._gram_tick
        self._gram_seq[seq.seq_id] = entry

    def release_grammar(self, seq: Sequence) -> None:
        entry = self._gram_seq.pop(seq.seq_id, None)
        if entry is not None:
            self._gram_ref[entry] -= 1

    def grammar_end_ids(self, seq: Sequence) -> List[int]:
        """The ids on which ``Sequence.append_token`` returns STOP: eos plus the stop_token_ids."""
        return list(dict.fromkeys([seq.eos_token_id, *seq.params.stop_token_ids]))[:gram_ops.MAX_END]

    def grammar_host_state(self, seq: Sequence) -> int:
        """Host truth of a sequence's automaton state: the walk of ``output_ids`` from state 0."""
        g, ends = seq.grammar, set(self.grammar_end_ids(seq))
        off, data = self.gram.off_np, self.gram.data_np
        state = 0
        for t in seq.output_ids:
            if t not in ends and 0 <= t < self.gram.vocab:
                state = g.walk(state, data[off[t]:off[t + 1]].tobytes())
        return state

    def _seed_grammar(self, todo: List[Sequence]) -> None:
        """After the token histories of ``todo`` were seeded (_seed_penalties): tables that are not
        on the device yet are loaded, in chunks of one message each, then every sequence's slot
        record is written: (table entry, host-truth state, end ids) for a guided one, "no table"
        for a slot whose previous owner was guided.  Both travel as messages of their own through
        the staging buffer, so TP workers run the same kernels on the same bytes."""
        if self.gram is None:
            return
        cap = self.layout.max_tokens
        entries: List[int] = []
        for s in todo:
            slot = self._pen_slot[s.seq_id]
            if s.grammar is None:
                if slot in self._gram_slots:
                    self._gram_slots.discard(slot)
                    entries += [slot, -1, -1, 0] + [-1] * gram_ops.MAX_END
                continue
            entry = self._gram_seq[s.seq_id]
            if entry not in self._gram_loaded:
                words = gram_ops.pack(s.grammar.cmap, s.grammar.trans, s.grammar.accept)
                for w0 in range(0, words.size, cap):
                    self._send_grammar(self.MODE_GLOAD, words[w0:w0 + cap], entry, w0)
                self._gram_loaded.add(entry)
            ends = self.grammar_end_ids(s)
            self._gram_slots.add(slot)
            entries += [slot, entry, self.grammar_host_state(s), len(ends)] + ends + [-1] * (gram_ops.MAX_END - len(ends))
        per_msg = max(1, cap // gram_ops.SEED_WORDS) * gram_ops.SEED_WORDS
        for e0 in range(0, len(entries), per_msg):
            chunk = entries[e0:e0 + per_msg]
            self._send_grammar(self.MODE_GSEED, np.asarray(chunk, dtype=np.int32), len(chunk) // gram_ops.SEED_WORDS, 0)

    def _send_grammar(self, mode: int, words: np.ndarray, a: int, b: int) -> None:
        self._next_staging()
        h = self.h
        h["input_ids"][:words.size] = words
        h["header"][:9] = (mode, words.size, a, b, 0, 0, 0, 0, 0)
        off, _ = self.layout.sections["input_ids"]
        self._publish_words((off + words.size + 3) // 4 * 4)
        self._run_grammar(mode, words.size, a, b)

    def _run_grammar(self, mode: int, n_words: int, a: int, b: int) -> None:
        """MODE_GLOAD: ``n_words`` of table entry ``a`` from word ``b``; MODE_GSEED: ``a`` slot records."""
        if mode == self.MODE_GLOAD:
            gram_ops.load(self.gram, a, b, self.d["input_ids"], n_words)
        else:
            gram_ops.seed(self.gram, self.d["input_ids"], a)
        self.stats["grammar_msgs"] = self.stats.get("grammar_msgs", 0) + 1

    def grammar_state(self, seq: Sequence):
        """Audit read-back (tests): the device's (table entry, state) of ``seq``; None when the
        sequence holds no slot or no grammar."""
        slot = self._pen_slot.get(seq.seq_id)
        if slot is None or seq.grammar is None or self.gram is None:
            return None
        return gram_ops.read_slot(self.gram, slot)

    def _seed_penalties(self, sampling: List[Sequence]) -> None:
        """Before a step is packed: every penalised sampling sequence without a slot (first
        sampling step, re-admission after a preemption) or with a stale one gets its slot seeded
        from host truth (prompt ids, generated ids, bias list).  launch() only runs with no step
        in flight, so ``output_ids`` is exactly G.  Seeds travel as MODE_SEED messages of their
        own through the staging buffer (TP workers run the same kernel from the same bytes): the
        id stream in ``input_ids``, the entry table in ``positions``.  A message holds at most
        one entry per slot (entries of one launch run concurrently); a history that does not
        fit continues in the next message with clear = 0."""
        todo = [s for s in sampling if (s.params.has_penalties or s.grammar is not None)
                and (s.seq_id not in self._pen_slot or s.seq_id in self._pen_stale)]
        if not todo:
            return
        self._seed_history(todo)
        self._seed_grammar(todo)

    def _seed_history(self, todo: List[Sequence]) -> None:
        cap = self.layout.max_tokens
        max_entries = max(1, cap // pen_ops.ENTRY_WORDS)
        ids: List[int] = []
        entries: List[int] = []
        for s in todo:
            if s.seq_id not in self._pen_slot:
                self._pen_slot[s.seq_id] = self._pen_free.pop()  # running <= max_num_seqs: never empty
            self._pen_stale.discard(s.seq_id)
            slot = self._pen_slot[s.seq_id]
            bias = s.params.logit_bias
            bias_bits = np.asarray([b for _, b in bias], dtype=np.float32).view(np.int32).tolist()
            ip = io = ib = 0  # consumed prompt ids / generated ids / bias pairs
            clear = 1
            while clear or ip < len(s.prompt_ids) or io < len(s.output_ids) or ib < len(bias):
                room = cap - len(ids)
                if room < 2 or len(entries) // pen_ops.ENTRY_WORDS >= max_entries:
                    self._send_seed(ids, entries)
                    ids, entries = [], []
                    room = cap
                n_p = min(len(s.prompt_ids) - ip, room)
                n_o = min(len(s.output_ids) - io, room - n_p) if ip + n_p == len(s.prompt_ids) else 0
                n_b = (min(len(bias) - ib, (room - n_p - n_o) // 2)
                       if ip + n_p == len(s.prompt_ids) and io + n_o == len(s.output_ids) else 0)
                entries += [slot, len(ids), n_p, n_o, n_b, clear]
                ids += s.prompt_ids[ip:ip + n_p] + s.output_ids[io:io + n_o]
                ids += [t for t, _ in bias[ib:ib + n_b]] + bias_bits[ib:ib + n_b]
                ip, io, ib, clear = ip + n_p, io + n_o, ib + n_b, 0
                if ip < len(s.prompt_ids) or io < len(s.output_ids) or ib < len(bias):
                    self._send_seed(ids, entries)  # the rest of this slot goes in the next message
                    ids, entries = [], []
        if entries:
            self._send_seed(ids, entries)

    def _send_seed(self, ids: List[int], entries: List[int]) -> None:
        self._next_staging()
        h = self.h
        ne = len(entries) // pen_ops.ENTRY_WORDS
        h["input_ids"][:len(ids)] = ids
        h["positions"][:len(entries)] = entries
        h["header"][:9] = (self.MODE_SEED, len(ids), ne, 0, 0, 0, 0, 0, 0)
        off, _ = self.layout.sections["positions"]
        self._publish_words((off + len(entries) + 3) // 4 * 4)
        self._run_seed(len(ids), ne)

    def _run_seed(self, n_ids: int, n_entries: int) -> None:
        pen_ops.seed(self.pen, self.d["positions"], n_entries, self.d["input_ids"], n_ids)
        self.stats["seed_msgs"] += 1

    def penalty_state(self, seq: Sequence):
        """Audit read-back (tests): the device's view of ``seq`` as (set of prompt-flagged ids,
        {id: count among generated tokens}); None when the sequence holds no slot."""
        slot = self._pen_slot.get(seq.seq_id)
        if slot is None:
            return None
        return pen_ops.read_slot(self.pen, slot)

    def _metadata(self, nd: int, n: int, T: int, max_q: int, short: bool = False) -> attn_ops.AttnMetadata:
        """``short``: every decode context is at most ``self.short_ctx`` tokens."""
        d = self.d
        npf = n - nd
        md = attn_ops.AttnMetadata(
            num_decode=nd, num_prefill=npf, num_prefill_tokens=T - nd, max_prefill_q_len=max_q,
            slot_mapping=d["slots"][:T],
            decode_block_tables=d["block_tables"][:nd] if nd else None,
            decode_context_lens=d["context_lens"][:nd] if nd else None,
            decode_part_o=self.part_o, decode_part_ml=self.part_ml,
            decode_max_ctx=self.short_ctx if short else 0)
        if npf:
            md.prefill_block_tables = d["block_tables"][nd:n]
            md.prefill_context_lens = d["context_lens"][nd:n]
            # query offsets relative to the first prefill token
            md.prefill_cu_q = d["cu_rel"][:npf + 1]
        return md

    # ----------------------------------------------------------------- execute
    # header words (section "header"): mode, T, n, nd, ns, max_q, graph bucket, short-context graph,
    # continuation (input ids = the previous step's sampled ids, already on the device), LoRA form
    # (a row of the step has an adapter)
    # MODE_SEED: header = (mode, id words, entries); seeds penalty slots (_seed_penalties)
    # MODE_GLOAD: header = (mode, words, table entry, first word); MODE_GSEED: (mode, words, slot
    # records): guided decoding tables and slot records (_seed_grammar), payload in "input_ids"
    MODE_IDLE, MODE_RUN, MODE_STOP, MODE_SEED, MODE_GLOAD, MODE_GSEED = 0, 1, 2, 3, 4, 5

    @torch.inference_mode()
    def execute(self, batch: ScheduledBatch) -> List[int]:
        """TP leader / single rank: pack, publish, run.  Returns the sampled token ids of
        ``batch.sampling_seqs()`` in order."""
        return self.fetch(self.launch(batch))

    def _next_staging(self) -> None:
        self._cur ^= 1
        ev = self._h2d_events[self._cur]
        if ev is not None:
            ev.synchronize()  # that buffer's last H2D copy has been consumed (normally long ago)
        self.host_buf, self.h = self._host_bufs[self._cur], self._hs[self._cur]

    def launch(self, batch: ScheduledBatch):
        """Enqueue one step (pack → H2D → graph replay / eager forward → sample → async D2H of
        the sampled ids) without waiting for the GPU; :meth:`fetch` returns the ids."""
        if batch.drafts is not None:
            return self.launch_verify(batch)
        sampling = batch.sampling_seqs()
        self._seed_penalties(sampling)
        self._next_staging()
        T, n, want_lp = self._pack(batch, sampling)
        nd = len(batch.decodes)
        ns = len(sampling)
        h = self.h
        max_q = 0
        g = 0
        if batch.prefills:
            rel = h["cu_q"][nd:n + 1] - h["cu_q"][nd]
            h["cu_rel"][:n - nd + 1] = rel
            max_q = int(np.max(np.diff(rel)))
        elif self.graphs and self.allow_graphs:
            st = self.model.st
            # DP attention + EP: every rank replays the bucket of the group's largest token count
            # (the lockstep vote's max): a graph's grouped expert GEMMs tile the rows any expert
            # can receive from the bucket it was captured at, so a rank with fewer sequences than
            # its peers must not replay a smaller one
            g = self._graph_bucket(max(nd, st.ep_step_rows) if st.dp_attention else nd) or 0
            if g:
                self._pad_decode(nd, g)
        short = self._short(g, nd)
        lora = self._step_lora if self.lora is not None else 0
        h["header"][:11] = (self.MODE_RUN, T, n, nd, ns, max_q, g, short, 0, lora, 0)
        self._publish(max(n, g))
        if batch.prefills and any(s.prompt_lp_missing for s, _ in batch.prefills):
            self._stage_prompt_lp(batch)
        toks = self._run(T, n, nd, ns, max_q, g, short, lora)
        handle = self._handle(toks, ns, want_lp)
        if self._plp_out is not None:  # a sixth element, only on steps with prompt-logprob rows
            handle, self._plp_out = handle + (self._plp_out,), None
        return handle

    def _short(self, g: int, nd: int) -> int:
        """1 when every decode context fits one attention partition: the step replays bucket
        ``g``'s short-context graph, or (eager, g = 0) launches the same one-workgroup-per-
        (seq, kv head) decode attention -- so eager and graphed steps compute identical sums."""
        if not (self.short_ctx and nd) or (g and g not in self.short_graphs):
            return 0
        return int(int(self.h["context_lens"][:nd].max()) <= self.short_ctx)

    def _handle(self, toks, ns: int, want_lp: bool = False):
        """→ (host ids, ns, event, device ids, host logprob rows or None)."""
        self.stats["steps"] += 1
        if ns == 0 or toks is None:
            return None, 0, None, None, None
        if not toks.is_cuda:
            return toks, ns, None, None, (self.lp_dev[:ns].clone() if want_lp else None)
        self._tok_i ^= 1
        host = self._tok_hosts[self._tok_i]
        host[:ns].copy_(toks[:ns], non_blocking=True)
        lp_host = None
        if want_lp:
            lp_host = self._lp_hosts[self._tok_i]
            lp_host[:ns].copy_(self.lp_dev[:ns], non_blocking=True)
        ev = self._tok_events[self._tok_i]
        if ev is None:
            ev = self._tok_events[self._tok_i] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return host, ns, ev, toks, lp_host

    def fetch_logprobs(self, handle):
        """After :meth:`fetch` of the same handle: the step's packed logprob rows (numpy int32
        ``[ns, LOGPROB_WORDS]``, a copy) or None when no sequence of the step asked."""
        lp, ns = handle[4], handle[1]
        if lp is None or ns == 0:
            return None
        return lp[:ns].numpy().copy()

    # ------------------------------------------------------------- prompt logprobs
    def _prompt_lp_buffers(self) -> None:
        """First step with a prompt-logprob row: the device records and targets and their pinned twins
        (bytes reserved at start-up, activation_reserve_bytes).  Eager steps only: never under capture."""
        W, n, pin = sampler_ops.PROMPT_LOGPROB_WORDS, self.max_step_tokens, self.device.type == "cuda"
        self.plp_dev = torch.zeros((n, W), dtype=torch.int32, device=self.device)
        self.plp_in_dev = torch.zeros(3 * n, dtype=torch.int32, device=self.device)
        self._plp_in_hosts = [torch.zeros(3 * n, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._plp_hosts = [torch.zeros((n, W), dtype=torch.int32, pin_memory=pin) for _ in range(2)]

    def _stage_prompt_lp(self, batch: ScheduledBatch) -> None:
        """A step with a sequence that still misses prompt-logprob entries: the asked rows, their
        targets and list lengths go to the device through their own pinned buffer (``_run`` scores
        them after the forward).  Leaves ``_plp`` None when no row of the step has a target."""
        chunks = [(s, s.num_computed, 1) for s in batch.decodes] + [(s, s.num_computed, c) for s, c in batch.prefills]
        targets = prompt_targets(chunks)
        rows, tgt, ntop, owners = [], [], [], []
        r = 0
        for s, start, length in chunks:
            for p in range(start, start + length):
                if targets[r] >= 0:
                    rows.append(r)
                    tgt.append(targets[r])
                    ntop.append(s.params.prompt_logprobs)
                    owners.append((s, p + 1))
                r += 1
        R = len(rows)
        if not R:
            return
        if self.plp_dev is None:
            self._prompt_lp_buffers()
        self._plp_i ^= 1
        ev = self._plp_events[self._plp_i]
        if ev is not None:
            ev.synchronize()  # the buffers' last use (two such steps back) is over
        # [rows | targets | list lengths], packed: one contiguous copy of 3 R words from pinned memory
        hin = self._plp_in_hosts[self._plp_i]
        hin[:3 * R] = torch.tensor(rows + tgt + ntop, dtype=torch.int32)
        self.plp_in_dev[:3 * R].copy_(hin[:3 * R], non_blocking=True)
        self._plp = (R, owners)

    def _score_prompt_rows(self, hidden: torch.Tensor) -> None:
        """After the forward of a step staged by :meth:`_stage_prompt_lp`: LM head over the asked
        rows in chunks of PROMPT_LP_CHUNK_ROWS, each scored against its target by the kernel, then
        one async copy of the records to pinned memory behind an event."""
        (R, owners), self._plp = self._plp, None
        rows, tgt, ntop = self.plp_in_dev[:R], self.plp_in_dev[R:2 * R], self.plp_in_dev[2 * R:3 * R]
        for c0 in range(0, R, PROMPT_LP_CHUNK_ROWS):
            c1 = min(R, c0 + PROMPT_LP_CHUNK_ROWS)
            logits = self.model.compute_logits(hidden.index_select(0, rows[c0:c1].long()))
            sampler_ops.prompt_logprobs(logits, tgt[c0:c1], ntop[c0:c1], self.plp_dev[c0:c1])
        self.stats["prompt_lp_rows"] += R
        self.stats["prompt_lp_steps"] += 1
        if self.device.type != "cuda":
            self._plp_out = (self.plp_dev[:R].clone(), R, owners, None)
            return
        host = self._plp_hosts[self._plp_i]
        host[:R].copy_(self.plp_dev[:R], non_blocking=True)
        ev = self._plp_events[self._plp_i]
        if ev is None:
            ev = self._plp_events[self._plp_i] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._plp_out = (host, R, owners, ev)

    def fetch_prompt_logprobs(self, handle):
        """The prompt-logprob entries a step computed: ``[(seq, entry index, (logprob, rank, top
        list))]``, empty for a step without such rows.  Waits for the step's records only."""
        if len(handle) < 6:
            return []
        host, R, owners, ev = handle[5]
        if ev is not None:
            ev.synchronize()
        rec = host[:R].numpy()
        return [(s, i, sampler_ops.prompt_logprob_entry(rec[j], s.params.prompt_logprobs))
                for j, (s, i) in enumerate(owners)]

    def fetch(self, handle) -> List[int]:
        toks, ns, ev = handle[:3]
        if ev is not None:
            ev.synchronize()
        self._check_comm()
        if ns == 0:
            return []
        return toks[:ns].tolist()

    def _check_comm(self) -> None:
        """Fail loudly once a custom all-reduce of this step (or an earlier one) timed out: the
        step's tokens were computed from incomplete sums (parallel/custom_ar.py)."""
        st = self.model.st
        gemm.check_fused()
        if st.custom_ar is not None:
            st.custom_ar.check()
        for rc in (getattr(st, "rccl_tp", None), getattr(st, "rccl_ep", None)):
            if rc is not None:  # RCCL's asynchronous error word (non-blocking poll)
                rc.check()
        for a2a in (getattr(st, "ep_a2a", None), getattr(st, "ep_a2a_prefill", None)):
            if a2a is not None:
                a2a.check()

    def launch_continuation(self, batch: ScheduledBatch, prev) -> Optional[tuple]:
        """Decode step k+1 of ``batch.decodes`` enqueued while step k (``prev``) may still run:
        every sequence advances one position, and step k's sampled ids — still on the GPU —
        are copied into this step's input ids on the stream, so the host never waits between
        the two steps.  Needs a captured graph bucket; returns None (caller falls back to a
        scheduled step) when a sequence cannot get the KV block for its next position."""
        seqs = batch.decodes
        n = len(seqs)
        g = self._graph_bucket(n) if self.graphs else None
        if not g or prev[3] is None or batch.prefills:
            return None
        for s in seqs:
            if s.num_computed + 2 > self.cfg.max_model_len or not self.bm.allocate(s.seq_id, s.num_computed + 2):
                return None
        self._next_staging()
        h = self.h
        sids = np.fromiter((s.seq_id for s in seqs), dtype=np.int64, count=n)
        ncomp = np.fromiter((s.num_computed + 1 for s in seqs), dtype=np.int32, count=n)
        ones = np.ones(n, dtype=np.int32)
        T = self.bm.pack_step(sids, ncomp, ones, np.zeros(n, dtype=np.int32), h["input_ids"], h["positions"],
                              h["slots"], h["block_tables"], self.max_blocks, h["context_lens"], h["cu_q"])
        h["sample_idx"][:n] = np.arange(n, dtype=np.int32)
        h["logprobs"][:n] = -1
        self._neutral_penalties(n)
        pen = self._pen_slot
        want_lp = False
        for r, s in enumerate(seqs):
            p = s.params
            if pen and s.seq_id in pen:
                self._fill_penalties(r, s)
            h["temperature"][r] = p.temperature
            h["top_k"][r] = p.top_k
            h["top_p"][r] = p.top_p
            h["min_p"][r] = p.min_p
            h["seeds"][r] = s.seed
            h["offsets"][r] = len(s.output_ids) + 1
            if p.logprobs is not None:
                h["logprobs"][r] = p.logprobs
                want_lp = True
        lora = 0
        if self.lora is not None:
            self._fill_lora(seqs, T)
            lora = self._step_lora
        self._pad_decode(n, g)
        short = self._short(g, n)
        h["header"][:11] = (self.MODE_RUN, T, n, n, n, 0, g, short, 1, lora, 0)
        self._publish(max(n, g))
        self.d["input_ids"][:n].copy_(prev[3][:n])  # step k's sampled ids, stream-ordered
        return self._handle(self._run(T, n, n, n, 0, g, short, lora), n, want_lp)

    def _staged_words(self, n_bt_rows: Optional[int]) -> int:
        """int32 words of the staging buffer a step uses: everything up to the used block-table
        rows (the last section), rounded to 16 bytes."""
        off, _ = self.layout.sections["block_tables"]
        rows = self.cfg.max_num_seqs if n_bt_rows is None else n_bt_rows
        n = min(self.layout.size, off + rows * self.max_blocks)
        return (n + 3) // 4 * 4

    def _publish(self, n_bt_rows: Optional[int] = None) -> None:
        """Hand the step inputs to the TP workers (shared-memory ring, host to host) and stage
        them on this rank's device.  The wait for a slot is bounded by the collectives' timeout:
        a worker that died (its pid is gone) or stopped consuming fails the step loudly."""
        self._publish_words(self._staged_words(n_bt_rows))

    def _publish_words(self, n: int) -> None:
        if self.channel is not None and self.model.st.tp_rank == 0:
            if not self.channel.publish(self._hnp[self._cur], n * 4, peer_timeout_ms()):
                dead = self.channel.dead_consumer()
                who = f"TP rank {dead + 1} died" if dead >= 0 else "a TP worker stopped consuming steps"
                raise TPPeerError(f"TP step channel: {who}")
        self._stage_local(n)

    def _stage_local(self, n: int) -> None:
        """Copy the first ``n`` words of the current pinned staging buffer to the device.  On
        the GPU a kernel reads the pinned buffer directly (no SDMA hand-off)."""
        if self.device.type == "cuda":
            native.call("pk_copy_from_host", self.dev_buf.data_ptr(), self.host_buf.data_ptr(), n * 4,
                        native.stream_ptr(self.device))
        else:
            self.dev_buf[:n].copy_(self.host_buf[:n], non_blocking=True)
        if self.device.type == "cuda":
            ev = self._h2d_events[self._cur]
            if ev is None:
                ev = self._h2d_events[self._cur] = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))

    def worker_loop(self) -> None:
        """Non-leader TP ranks: take each step from the leader's ring into the next pinned
        staging buffer, read its header on the host and launch the same work — the worker never
        waits for its own GPU (only, through the double-buffered staging, for a step two back)."""
        chan = self.channel
        done = threading.Event()
        watch = threading.Thread(target=self._leader_watch, args=(done,), name="pk-leader-watch", daemon=True)
        watch.start()
        try:
            self._worker_steps(chan)
        finally:
            done.set()
            watch.join(5.0)

    def _leader_watch(self, done: threading.Event, grace_s: float = 10.0) -> None:
        """A worker blocked on its GPU (a collective waiting for the dead leader, an RCCL kernel
        that never times out) cannot reach the step channel's dead-producer check: this thread
        sees the leader's pid vanish, aborts the communicators (the waits return), and if the
        main loop has not ended the process ``grace_s`` later, exits it non-zero itself."""
        while not done.wait(1.0):
            if self.channel.producer_alive:
                continue
            self.abort_comms()
            if done.wait(grace_s):
                return
            import sys
            print("TP leader process died and this worker is still blocked on the GPU: exiting",
                  file=sys.stderr, flush=True)
            os._exit(1)

    def _worker_steps(self, chan) -> None:
        while True:
            self._next_staging()
            nbytes = chan.consume(self._hnp[self._cur], 1000)
            self._check_comm()
            if nbytes == -1:
                continue  # idle leader: poll again (and re-check the comm error word)
            if nbytes == -2:
                return
            if nbytes == -3:  # the leader's process is gone (SIGKILL, OOM, crash): end this rank
                raise TPPeerError("TP leader process died; this worker exits for its supervisor to restart the group")
            mode, T, n, nd, ns, max_q, g, short, cont, lora, qr = (int(v) for v in self.h["header"][:11])
            if mode == self.MODE_STOP:
                return
            if mode == self.MODE_SEED:
                self._stage_local(nbytes // 4)
                with torch.inference_mode():
                    self._run_seed(T, n)
                continue
            if mode in (self.MODE_GLOAD, self.MODE_GSEED):
                self._stage_local(nbytes // 4)
                with torch.inference_mode():
                    self._run_grammar(mode, T, n, nd)
                continue
            if mode != self.MODE_RUN:
                continue
            self._stage_local(nbytes // 4)
            with torch.inference_mode():
                if cont:
                    self.d["input_ids"][:n].copy_(self._prev_toks[:n])
                toks = self._run(T, n, nd, ns, max_q, g, short, lora, qr)
            if toks is not None:
                self._prev_toks = toks
            self.stats["steps"] += 1

    def fallback_unfused(self) -> None:
        """A fused decode launch lost an in-launch hand-off (another process on this GPU kept part
        of its grid from being resident): wait for the GPU, re-arm the sticky word, switch this
        process to the two-launch path for good (WARN) and re-capture the decode graphs that held
        the fused kernels.  The caller re-runs the step (LLMEngine._complete_or_redo)."""
        import logging
        logging.getLogger(__name__).warning(
            "fused decode launch hand-off timed out (GPU shared with another process?): the failed step is "
            "re-run and every later step takes the two-launch path")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        gemm.disable_fused()
        gemm.clear_fused_error()
        self.stats["fused_fallbacks"] = self.stats.get("fused_fallbacks", 0) + 1
        # the failed step and any continuation of it have counted tokens that are discarded: every
        # live slot is re-seeded from host truth by the next launch that samples its sequence
        self._pen_stale.update(self._pen_slot)
        if self.graphs:
            sizes = sorted(self.graphs)
            self.graphs.clear()
            self.graph_out.clear()
            self.short_graphs.clear()
            self.short_graph_out.clear()
            for d in (self.lora_graphs, self.lora_graph_out, self.lora_short_graphs, self.lora_short_graph_out,
                      self.verify_graphs, self.verify_graph_out):
                d.clear()
            self._graph_logits.clear()
            self.graph_pool = None
            self.capture_graphs(sizes)

    def abort_comms(self) -> None:
        """Watchdog / failure path: tear down this rank's RCCL communicators (a collective hung on
        a dead peer returns) and mark the IPC collectives failed (every later call skips its
        waits), so the process can exit instead of blocking in a GPU wait."""
        st = self.model.st
        for rc in {id(c): c for c in (getattr(st, "rccl_tp", None), getattr(st, "rccl_ep", None))
                   if c is not None}.values():
            try:
                rc.abort()
            except Exception:  # noqa: BLE001 - best effort on the way down
                pass
        if st.custom_ar is not None:
            st.custom_ar.fail()
        for a2a in (getattr(st, "ep_a2a", None), getattr(st, "ep_a2a_prefill", None)):
            if a2a is not None:
                a2a.fail()

    def stop_workers(self) -> None:
        if self.channel is not None and self.model.st.tp_rank == 0:
            self._next_staging()
            self.h["header"][:9] = (self.MODE_STOP, 0, 0, 0, 0, 0, 0, 0, 0)
            self.channel.publish(self._hnp[self._cur], 64, 60000)
            self.channel.close()

    def _run(self, T: int, n: int, nd: int, ns: int, max_q: int, g: int, short: int = 0, lora: int = 0, qr: int = 0):
        d = self.d
        if qr:  # a verify step: n sequences x qr rows, every row sampled
            self.stats["verify_steps"] += 1
            if g:
                self.verify_graphs[g].replay()
                self.stats["verify_graph_steps"] += 1
                if self.debug_logits:
                    self.last_logits = self._graph_logits[(g, "verify")]
                return self.verify_graph_out[g]
            hidden = self.model(d["input_ids"][:T], d["positions"][:T], self._verify_metadata(n), self.kv_caches)
            logits = self.model.compute_logits(hidden)
            if self.keep_logits or self.debug_logits:
                self.last_logits = logits
            return self._sample(logits, T)
        if self.lora is not None:
            self.lora.active = bool(lora)  # the model's LoRA form for this step (eager; graphs hold theirs)
            self.stats["lora_steps"] += int(bool(lora))
        if g:
            graphs, outs = ((self.lora_short_graphs, self.lora_short_graph_out) if short else
                            (self.lora_graphs, self.lora_graph_out)) if lora else \
                           ((self.short_graphs, self.short_graph_out) if short else (self.graphs, self.graph_out))
            graphs[g].replay()
            out = outs[g]
            if short:
                self.stats["short_graph_steps"] += 1
            if lora:
                self.stats["lora_graph_steps"] += 1
            self.stats["graph_steps"] += 1
            if self.debug_logits:
                self.last_logits = self._graph_logits[(g, int(bool(short)) + 2 * int(bool(lora)))]
            return out
        md = self._metadata(nd, n, T, max_q, bool(short))
        hidden = self.model(d["input_ids"][:T], d["positions"][:T], md, self.kv_caches)
        if self._plp is not None:
            self._score_prompt_rows(hidden)
        if ns == 0:
            return None
        rows = hidden if ns == T else hidden.index_select(0, d["sample_idx"][:ns].long())
        logits = self.model.compute_logits(rows)
        if self.keep_logits or self.debug_logits:
            self.last_logits = logits
        return self._sample(logits, ns)

    def _sample(self, logits: torch.Tensor, ns: int) -> torch.Tensor:
        """logits → penalised copy of the rows with a slot → grammar mask on that copy → sample (those
        rows from the copy) → logprobs (from the raw logits) → count the sampled ids → advance the
        grammar states.  Eager and inside every graph."""
        d = self.d
        V = logits.shape[-1]
        pen_out = pen_ops.apply(self.pen, logits, d["pen_slot"], d["rep"], d["freq"], d["pres"])
        if self.gram is not None:
            gram_ops.mask(self.gram, pen_out, d["pen_slot"], ns, V)
        toks = sampler_ops.sample(logits, d["temperature"][:ns], d["top_k"][:ns], d["top_p"][:ns],
                                  d["min_p"][:ns], d["seeds"][:ns], d["offsets"][:ns],
                                  alt=pen_out, alt_slots=d["pen_slot"])
        sampler_ops.logprobs(logits, toks, d["logprobs"][:ns], self.lp_dev)
        pen_ops.update(self.pen, d["pen_slot"], toks, ns)
        if self.gram is not None:
            gram_ops.advance(self.gram, d["pen_slot"], toks, ns, V)
        return toks

    # ------------------------------------------------------------------ graphs
    def _graph_bucket(self, nd: int) -> Optional[int]:
        for b in sorted(self.graphs):
            if b >= nd:
                return b
        return None

    def _pad_decode(self, nd: int, g: int) -> None:
        h = self.h
        if g > nd:
            h["input_ids"][nd:g] = 0
            h["positions"][nd:g] = 0
            h["slots"][nd:g] = -1
            h["context_lens"][nd:g] = 0
            h["sample_idx"][nd:g] = np.arange(nd, g, dtype=np.int32)
            h["temperature"][nd:g] = 0.0
            h["top_k"][nd:g] = 0
            h["top_p"][nd:g] = 1.0
            h["min_p"][nd:g] = 0.0
            h["logprobs"][nd:g] = -1
            h["pen_slot"][nd:g] = -1
            if self.lora is not None:
                h["lora_idx"][nd:g] = -1

    def default_graph_sizes(self) -> List[int]:
        if self.cfg.graph_batch_sizes:
            sizes = list(self.cfg.graph_batch_sizes)
        else:
            sizes = [1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 160, 192, 224, 256, 320, 384, 448, 512]
        return [s for s in sizes if s <= self.cfg.max_num_seqs]

    @torch.inference_mode()
    def capture_graphs(self, sizes: Optional[List[int]] = None) -> None:
        if self.device.type != "cuda" or not self.cfg.hip_graphs:
            return
        sizes = sizes or self.default_graph_sizes()
        st = self.model.st
        if st.dp_attention:  # every replay sends bucket x top-k rows per peer: within the IPC capacity
            k = self.mcfg.experts_per_token
            sizes = [g for g in sizes if st.ep_a2a is not None and st.ep_a2a.fits(g * k)]
        d = self.d
        # a valid dummy decode state: every row points at block 0, context 1, no cache writes
        self.host_buf.zero_()
        self.h["slots"][:] = -1
        self.h["context_lens"][: self.cfg.max_num_seqs] = 1
        self.h["top_p"][:] = 1.0
        self.h["logprobs"][:] = -1
        self.h["pen_slot"][:] = -1
        if self.lora is not None:
            self.h["lora_idx"][:] = -1
        self.h["sample_idx"][:] = np.arange(self.h["sample_idx"].shape[0], dtype=np.int32)
        if self.spec_qr:
            self.h["verify_rows"][:] = 1
        self.dev_buf.copy_(self.host_buf)
        torch.cuda.synchronize(self.device)
        stream = torch.cuda.Stream(self.device)
        variants = (False, True) if self.short_ctx else (False,)
        st = self.model.st
        forms = (False, True) if self.lora is not None else (False,)
        for g, short, lora in [(g, v, f) for g in sorted(sizes, reverse=True) for v in variants for f in forms]:
            md = self._metadata(g, g, g, 0, short)
            if self.lora is not None:
                self.lora.active = lora  # which form of the model this graph records
            if st.dp_attention:  # capture the IPC expert all-to-all path (device-side counts)
                st.ep_step_rows = g

            def run():
                hidden = self.model(d["input_ids"][:g], d["positions"][:g], md, self.kv_caches)
                logits = self.model.compute_logits(hidden)
                if self.debug_logits:
                    self._graph_logits[(g, int(short) + 2 * int(lora))] = logits.clone()
                return self._sample(logits, g)

            # warm up on a side stream (allocator + library handles), then capture
            stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(stream):
                run()
            torch.cuda.current_stream(self.device).wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with _capture(graph, self.graph_pool):
                out = run()
            if self.graph_pool is None:
                self.graph_pool = graph.pool()
            if lora:
                (self.lora_short_graphs if short else self.lora_graphs)[g] = graph
                (self.lora_short_graph_out if short else self.lora_graph_out)[g] = out
            else:
                (self.short_graphs if short else self.graphs)[g] = graph
                (self.short_graph_out if short else self.graph_out)[g] = out
        if self.lora is not None:
            self.lora.active = False
        if self.spec_qr:
            self._capture_verify_graphs(sizes, stream)
        torch.cuda.synchronize(self.device)

    def verify_graph_sizes(self, sizes: Optional[List[int]] = None) -> List[int]:
        """The decode buckets a verify graph exists for: those whose rows fit a verify step."""
        return [g for g in (sizes or self.default_graph_sizes()) if g <= self.verify_max_seqs]

    def _capture_verify_graphs(self, sizes: List[int], stream) -> None:
        """One verify graph per decode bucket g with g * qr rows within the decode row limit, on the
        dummy state of capture_graphs (context 1, one real row per sequence, no cache writes)."""
        d, qr = self.d, self.spec_qr
        for g in sorted(self.verify_graph_sizes(sizes), reverse=True):
            T = g * qr
            md = self._verify_metadata(g)

            def run():
                hidden = self.model(d["input_ids"][:T], d["positions"][:T], md, self.kv_caches)
                logits = self.model.compute_logits(hidden)
                if self.debug_logits:
                    self._graph_logits[(g, "verify")] = logits.clone()
                return self._sample(logits, T)

            stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(stream):
                run()
            torch.cuda.current_stream(self.device).wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with _capture(graph, self.graph_pool):
                out = run()
            if self.graph_pool is None:
                self.graph_pool = graph.pool()
            self.verify_graphs[g] = graph
            self.verify_graph_out[g] = out
