"""Paged attention + fused RoPE/KV-cache write (HIP on GPU, fp32 reference on CPU).

Batch layout (see :class:`AttnMetadata`): the first ``num_decode`` tokens are decode tokens
(one per sequence), followed by the prefill tokens of ``num_prefill`` sequences (possibly
chunked, possibly with a cached prefix).  Decode goes through the split-K decode kernel,
prefill through the varlen causal kernel; both read K/V only from the paged cache (new
tokens are written by :func:`rope_and_cache` first).
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Optional

import torch

from . import native, reference


@dataclasses.dataclass
class AttnMetadata:
    num_decode: int
    num_prefill: int
    num_prefill_tokens: int
    max_prefill_q_len: int
    slot_mapping: torch.Tensor              # [T] int32
    decode_block_tables: Optional[torch.Tensor] = None   # [nd, MB] int32
    decode_context_lens: Optional[torch.Tensor] = None   # [nd] int32
    prefill_block_tables: Optional[torch.Tensor] = None  # [np, MB] int32
    prefill_context_lens: Optional[torch.Tensor] = None  # [np] int32
    prefill_cu_q: Optional[torch.Tensor] = None          # [np+1] int32, relative to the first prefill token
    decode_part_o: Optional[torch.Tensor] = None         # split-K workspace
    decode_part_ml: Optional[torch.Tensor] = None
    decode_max_ctx: int = 0  # bound on every decode context of the step (0: block-table capacity)
    # A verify step of speculative decoding (:func:`paged_verify`): ``verify_qr`` > 0 query rows per
    # sequence, ``num_decode`` = n_seqs * verify_qr rows in all, sequence s owning rows s * qr + j
    verify_qr: int = 0
    verify_rows: Optional[torch.Tensor] = None           # [n_seqs] int32: real rows R of each sequence, 1..qr
    verify_block_tables: Optional[torch.Tensor] = None   # [n_seqs, MB] int32
    verify_context_lens: Optional[torch.Tensor] = None   # [n_seqs] int32: keys cached, the R new ones included

    @property
    def num_tokens(self) -> int:
        return self.num_decode + self.num_prefill_tokens


_PART = 512  # must match kDecodePart in csrc/kernels/attn_decode.h
_PART_MIN = 128  # kDecodePartSmall: launches whose (seq, kv head) pairs cannot fill the chip
_FILL_SET = False


def apply_decode_fill() -> None:
    """POLYKEY_DECODE_FILL, applied once per process: the workgroup count below which decode
    attention takes 128-key partitions (csrc attention.hip decode_plan; 0: always 512)."""
    global _FILL_SET
    if not _FILL_SET and os.environ.get("POLYKEY_DECODE_FILL") is not None:
        native.call("pk_set_decode_fill", int(os.environ["POLYKEY_DECODE_FILL"]))
    _FILL_SET = True


# g_decode_fill (csrc attention.hip): fewer (seq, kv head, partition) workgroups than this -> 128-key partitions.
# The library's own default is 64: sizing the slabs for 256 only over-allocates them.
_DECODE_FILL = int(os.environ.get("POLYKEY_DECODE_FILL", "256"))


def decode_workspace(n_seqs: int, n_q: int, max_blocks: int, block_size: int, device, n_kv: int = 0,
                     kv_heads: Optional[int] = None) -> tuple:
    """Partition slabs for split-K decode attention.  A launch
    strides the slabs by its OWN partition count, so they are sized for the largest launch:
    ``n_seqs`` sequences at 512-key partitions, or the few sequences that take 128-key ones
    (csrc attention.hip decode_plan: fewer than 256 (seq, kv head) workgroups, i.e. at most
    255 // kv_heads sequences).  ``kv_heads`` (kv heads per rank; else ``n_kv``) None: every
    launch sized at 128-key partitions (4x the full-batch need: ~4.3 GB at 256 seqs x 128k ctx
    for Llama-3-8B, taken from the KV-cache budget -- ADVICE r4)."""
    ctx = max_blocks * block_size
    n_small = (ctx + _PART_MIN - 1) // _PART_MIN
    if n_small <= 1:
        return None, None
    kvh = kv_heads or n_kv
    if kvh:
        seqs_small = min(n_seqs, (_DECODE_FILL - 1) // kvh)
        rows = max(n_seqs * ((ctx + _PART - 1) // _PART), seqs_small * n_small)
    else:
        rows = n_seqs * n_small
    o = torch.empty((rows * n_q, 128), dtype=torch.float32, device=device)
    ml = torch.empty((rows * n_q, 2), dtype=torch.float32, device=device)
    return o, ml


FP8 = reference.FP8  # the reduced-precision KV-cache element (OCP e4m3, csrc/kernels/kv_fp8.h)


def cache_is_fp8(k_cache: torch.Tensor, v_cache: torch.Tensor) -> bool:
    """Which cache type a layer's launches are told: bf16 or FP8 (e4m3).  K and V of one layer share
    the dtype; anything else is an error, never a silent conversion."""
    if k_cache.dtype != v_cache.dtype:
        raise TypeError(f"K and V cache dtypes differ: {k_cache.dtype} vs {v_cache.dtype}")
    if k_cache.dtype == FP8:
        return True
    if k_cache.dtype != torch.bfloat16:
        raise TypeError(f"unsupported KV-cache dtype {k_cache.dtype}: bfloat16 or float8_e4m3fn")
    return False


def _kv_args(k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: float, v_scale: float) -> tuple:
    """``kv_dtype, k_scale, v_scale``: what every attention entry point takes ahead of the stream."""
    return int(cache_is_fp8(k_cache, v_cache)), float(k_scale), float(v_scale)


def slab_writers_ok(k_cache: torch.Tensor) -> bool:
    """Whether the launches that write k / v rows from the QKV projection's fp32 slabs may serve this
    cache.  Three launches are bf16-only (2-byte rows): the split-K QKV epilogue writer
    (``gemm.qkv_reduce_rope_cache``), the fused QKV -> attention launch (``gemm.qkv_attn_fused``)
    and the carried TP collective (``LlamaForCausalLM._forward_tp_carried``).  An FP8 (e4m3) cache
    bypasses all three, decided from the dtype of the cache at hand and nothing else."""
    return k_cache.dtype == torch.bfloat16


def check_qk_norm(q_norm: torch.Tensor, k_norm: torch.Tensor, hd: int = 128) -> None:
    """What the QK-norm entry points read: two contiguous [128] bf16 weights on the GPU, 16-byte
    aligned (``rope_and_cache_kernel`` loads them as 16-byte vectors)."""
    for w in (q_norm, k_norm):
        if w.dtype != torch.bfloat16 or tuple(w.shape) != (hd,) or hd != 128 or not w.is_contiguous() or not w.is_cuda:
            raise ValueError(f"QK-norm weights are contiguous [128] bfloat16 GPU tensors, got {tuple(w.shape)} "
                             f"{w.dtype} on {w.device}")
        if w.data_ptr() % 16:
            raise ValueError("QK-norm weights must be 16-byte aligned (a view at an odd storage offset is not)")


def rope_and_cache(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor, k_cache: torch.Tensor,
                   v_cache: torch.Tensor, slot_mapping: torch.Tensor, nq: int, nkv: int, hd: int = 128, *,
                   k_scale: float = 1.0, v_scale: float = 1.0, q_norm: Optional[torch.Tensor] = None,
                   k_norm: Optional[torch.Tensor] = None, eps: float = 1e-6) -> None:
    """In place on ``qkv`` [T, (nq+2nkv)*hd]; writes K/V of every token with slot >= 0.  An FP8
    cache stores ``e4m3(clamp(x / scale, -448, 448))`` (the scales are ignored for bf16).
    ``q_norm`` / ``k_norm`` ([128] bf16, both or neither) select the QK-norm entry point: every q and
    k head is RMS-normalised with ``eps`` and weighted before the rotation (Qwen3)."""
    if (q_norm is None) != (k_norm is None):
        raise ValueError("q_norm and k_norm come together")
    if not qkv.is_cuda:
        reference.rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, nq, nkv, hd,
                                 k_scale=k_scale, v_scale=v_scale, q_norm=q_norm, k_norm=k_norm, eps=eps)
        return
    T = qkv.shape[0]
    assert qkv.stride(-1) == 1 and positions.dtype == torch.int32 and slot_mapping.dtype == torch.int32
    assert cos_sin.dtype == torch.float32
    if q_norm is not None:
        check_qk_norm(q_norm, k_norm, hd)
        native.call("pk_rope_and_cache_qknorm", qkv.data_ptr(), positions.data_ptr(), cos_sin.data_ptr(),
                    k_cache.data_ptr(), v_cache.data_ptr(), slot_mapping.data_ptr(), q_norm.data_ptr(),
                    k_norm.data_ptr(), float(eps), T, nq, nkv, hd, k_cache.shape[2], qkv.stride(0),
                    *_kv_args(k_cache, v_cache, k_scale, v_scale), native.stream_ptr())
        return
    native.call("pk_rope_and_cache", qkv.data_ptr(), positions.data_ptr(), cos_sin.data_ptr(), k_cache.data_ptr(),
                v_cache.data_ptr(), slot_mapping.data_ptr(), T, nq, nkv, hd, k_cache.shape[2], qkv.stride(0),
                *_kv_args(k_cache, v_cache, k_scale, v_scale), native.stream_ptr())


def paged_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, md: AttnMetadata,
                    scale: float, out: Optional[torch.Tensor] = None, *, k_scale: float = 1.0,
                    v_scale: float = 1.0) -> torch.Tensor:
    """q: [T, nq, 128] view (row stride may exceed nq*128, e.g. inside the QKV buffer).
    Returns out: [T, nq*128] bf16.  An FP8 cache is read as ``scale * byte`` (k_scale folded into
    the softmax scale, v_scale into the normalisation; both ignored for bf16)."""
    T, nq, hd = q.shape
    nkv = k_cache.shape[1]
    bs = k_cache.shape[2]
    if out is None:
        out = torch.empty((T, nq * hd), dtype=q.dtype, device=q.device)
    if not q.is_cuda:
        _reference(q, k_cache, v_cache, md, scale, out, k_scale, v_scale)
        return out
    assert hd == 128 and q.stride(-1) == 1 and q.stride(1) == hd
    apply_decode_fill()
    kv = _kv_args(k_cache, v_cache, k_scale, v_scale)
    stream = native.stream_ptr()
    nd = md.num_decode
    if nd > 0:
        bt = md.decode_block_tables
        native.call("pk_paged_decode", out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                    bt.data_ptr(), md.decode_context_lens.data_ptr(),
                    native.ptr(md.decode_part_o) or 0, native.ptr(md.decode_part_ml) or 0,
                    nd, nq, nkv, bs, bt.stride(0), q.stride(0), out.stride(0),
                    float(scale), int(md.decode_max_ctx), *kv, stream)
    if md.num_prefill > 0:
        bt = md.prefill_block_tables
        qp = q[nd:]
        op = out[nd:]
        native.call("pk_paged_prefill", op.data_ptr(), qp.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                    bt.data_ptr(), md.prefill_context_lens.data_ptr(), md.prefill_cu_q.data_ptr(),
                    md.num_prefill, nq, nkv, bs, bt.shape[1], q.stride(0), out.stride(0), int(md.max_prefill_q_len),
                    float(scale), *kv, stream)
    return out


def verify_workspace(n_seqs: int, qr: int, n_q: int, max_blocks: int, block_size: int, device, n_kv: int = 0,
                     kv_heads: Optional[int] = None) -> tuple:
    """Partition slabs of :func:`paged_verify`: the launch plan is the decode plan of ``n_seqs``
    sequences and every slab row holds one of the ``n_seqs * qr`` query rows, i.e. the decode
    workspace of ``n_seqs`` sequences with ``qr * n_q`` heads."""
    return decode_workspace(n_seqs, n_q * qr, max_blocks, block_size, device, n_kv, kv_heads)


def paged_verify(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, md: AttnMetadata, scale: float,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of a verify step (speculative decoding).  q: [n_seqs * qr, nq, 128] view, sequence s
    owning rows ``s * qr + j``; the first ``R = md.verify_rows[s]`` (1..qr) are real, and
    ``C = md.verify_context_lens[s]`` counts the keys in the cache *including* the R written this
    step.  Row ``j < R`` attends keys ``0 .. C - R + j``; rows ``j >= R`` and every row of a sequence
    with ``C <= 0`` come out as exact zeros.  Returns out [n_seqs * qr, nq * 128] (contiguous rows).

    bf16 caches only, ``qr * (nq / nkv) <= 16`` (the columns of one MFMA tile): anything else is an
    error.  ``md.decode_part_o`` / ``decode_part_ml`` are sized by :func:`verify_workspace`.  R is
    checked here when ``md.verify_rows`` lives on the host; on the GPU the packer guarantees it (the
    kernel reads rows past qr as qr and R <= 0 as a sequence of padding rows)."""
    T, nq, hd = q.shape
    qr = int(md.verify_qr)
    nkv, bs = k_cache.shape[1], k_cache.shape[2]
    if qr < 1 or T % qr or nq % nkv or qr * (nq // nkv) > 16:
        raise ValueError(f"paged_verify: {T} rows of {qr} per sequence, GQA group {nq // max(nkv, 1)}: "
                         f"needs qr >= 1, whole sequences and qr * group <= 16")
    if k_cache.dtype == FP8 or v_cache.dtype == FP8 or (q.is_cuda and cache_is_fp8(k_cache, v_cache)):
        raise TypeError("paged_verify reads a bfloat16 KV cache only (an FP8 cache has no verify kernel)")
    n_seqs = T // qr
    rows, ctxs, bt = md.verify_rows, md.verify_context_lens, md.verify_block_tables
    assert rows.shape[0] == n_seqs and ctxs.shape[0] == n_seqs and bt.shape[0] == n_seqs
    if out is None:
        out = torch.empty((T, nq * hd), dtype=q.dtype, device=q.device)
    if not q.is_cuda:
        R, C = rows.tolist(), ctxs.tolist()
        if any(not 1 <= r <= qr for r in R):
            raise ValueError(f"paged_verify: verify_rows outside 1..{qr}: {R}")
        out.zero_()
        live = [s for s in range(n_seqs) if C[s] > 0]
        if live:  # the real rows of every live sequence, as R-token chunks ending at key C - 1
            idx = torch.tensor([s * qr + j for s in live for j in range(R[s])], dtype=torch.long)
            cu = torch.tensor([0] + [R[s] for s in live], dtype=torch.int32).cumsum(0).to(torch.int32)
            sel = torch.tensor(live, dtype=torch.long)
            md_r = AttnMetadata(num_decode=0, num_prefill=len(live), num_prefill_tokens=idx.numel(),
                                max_prefill_q_len=max(R[s] for s in live), slot_mapping=md.slot_mapping,
                                prefill_block_tables=bt[sel], prefill_context_lens=ctxs[sel], prefill_cu_q=cu)
            o = torch.empty((idx.numel(), nq * hd), dtype=q.dtype)
            _reference(q[idx].contiguous(), k_cache, v_cache, md_r, scale, o)
            out[idx] = o
        return out
    assert hd == 128 and q.stride(-1) == 1 and q.stride(1) == hd and out.stride(0) == nq * hd
    assert rows.dtype == torch.int32 and ctxs.dtype == torch.int32 and bt.dtype == torch.int32
    apply_decode_fill()
    native.call("pk_paged_verify", out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                bt.data_ptr(), ctxs.data_ptr(), rows.data_ptr(), native.ptr(md.decode_part_o) or 0,
                native.ptr(md.decode_part_ml) or 0, n_seqs, qr, nq, nkv, bs, bt.stride(0), q.stride(0), out.stride(0),
                float(scale), int(md.decode_max_ctx), 0, native.stream_ptr())
    return out


def _reference(q, k_cache, v_cache, md: AttnMetadata, scale, out, k_scale=1.0, v_scale=1.0):
    nd = md.num_decode
    o3 = out.view(out.shape[0], q.shape[1], q.shape[2])
    if nd > 0:
        cu = torch.arange(nd + 1, dtype=torch.int32)
        o3[:nd] = reference.paged_attention(q[:nd].contiguous(), k_cache, v_cache, md.decode_block_tables.cpu(),
                                            md.decode_context_lens.cpu(), cu, scale, k_scale=k_scale, v_scale=v_scale)
    if md.num_prefill > 0:
        o3[nd:] = reference.paged_attention(q[nd:].contiguous(), k_cache, v_cache, md.prefill_block_tables.cpu(),
                                            md.prefill_context_lens.cpu(), md.prefill_cu_q.cpu(), scale, k_scale=k_scale,
                                            v_scale=v_scale)


def default_scale(head_dim: int = 128) -> float:
    return 1.0 / math.sqrt(head_dim)


def paged_decode_from_qkv(p, positions: torch.Tensor, cos_sin: torch.Tensor, k_cache: torch.Tensor,
                          v_cache: torch.Tensor, md: AttnMetadata, scale: float, nq: int, nkv: int, *,
                          k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """Pure-decode attention straight from the fused QKV projection's split-K slabs
    (``gemm.Partial``): the attention kernel reduces the slabs, applies RoPE, writes the new
    k / v into the paged cache and attends — one kernel instead of reduce+RoPE+cache then
    attention.  Returns [T, nq*128] bf16."""
    assert md.num_prefill == 0 and k_cache.shape[-1] == 128
    apply_decode_fill()
    T = p.M
    out = torch.empty((T, nq * 128), dtype=torch.bfloat16, device=p.buf.device)
    bt = md.decode_block_tables
    native.call("pk_paged_decode_qkv", out.data_ptr(), p.buf.data_ptr(), p.S, p.M, positions.data_ptr(),
                cos_sin.data_ptr(), md.slot_mapping.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                bt.data_ptr(), md.decode_context_lens.data_ptr(), native.ptr(md.decode_part_o) or 0,
                native.ptr(md.decode_part_ml) or 0, md.num_decode, nq, nkv, k_cache.shape[2], bt.stride(0),
                out.stride(0), float(scale), int(md.decode_max_ctx), *_kv_args(k_cache, v_cache, k_scale, v_scale),
                native.stream_ptr())
    return out
