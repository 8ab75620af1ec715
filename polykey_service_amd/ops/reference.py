"""fp32 PyTorch reference implementations of every hand-written kernel.

Used (a) as the numerics oracle in ``tests/kernels`` (each HIP kernel is compared against
the op here) and (b) on CPU tensors so the whole engine runs in the GPU-less dev container.
Layouts are the ones the kernels use:

* K cache  ``[num_blocks, n_kv, block_size, head_dim]`` (token rows contiguous)
* V cache  ``[num_blocks, n_kv, head_dim, block_size]`` (stored transposed, so the P·V MFMA
  reads 8 consecutive tokens of one channel as one 16-byte vector)
* slot = block_id * block_size + offset; slot < 0 means "do not write" (padding rows)
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch


# ----------------------------------------------------------------------------- norms
def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return ((xf * r).to(x.dtype).float() * weight.float()).to(x.dtype)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float):
    residual.copy_((x.float() + residual.float()).to(residual.dtype))
    x.copy_(rms_norm(residual, weight, eps))
    return x, residual


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    d = x.shape[-1] // 2
    g, u = x[..., :d].float(), x[..., d:].float()
    return (torch.nn.functional.silu(g).to(x.dtype).float() * u).to(x.dtype)


def silu_and_mul_interleaved(x: torch.Tensor, block: int = 16) -> torch.Tensor:
    """x: [T, 2I] with gate/up interleaved in blocks of ``block`` columns."""
    T, I2 = x.shape[0], x.shape[-1]
    v = x.reshape(-1, I2 // (2 * block), 2, block)
    g, u = v[:, :, 0].reshape(-1, I2 // 2).float(), v[:, :, 1].reshape(-1, I2 // 2).float()
    return (torch.nn.functional.silu(g).to(x.dtype).float() * u).to(x.dtype).view(x.shape[:-1] + (I2 // 2,))


# ------------------------------------------------------------------------------ rope
def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[dict] = None) -> torch.Tensor:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling.get("low_freq_factor", 1.0), scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (1 - smooth) * inv / factor + smooth * inv
        is_mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(is_mid, mid, scaled)
    return inv.float()


def rope_cos_sin_cache(max_pos: int, head_dim: int, theta: float, scaling: Optional[dict] = None,
                       device=None) -> torch.Tensor:
    """[max_pos, head_dim] fp32: cos in [:, :hd/2], sin in [:, hd/2:]."""
    inv = rope_inv_freq(head_dim, theta, scaling).double()
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """Neox/HF ``rotate_half`` RoPE. x: [T, H, D] → rotated, same dtype (fp32 math)."""
    D = x.shape[-1]
    cs = cos_sin[positions.long()].float()
    cos, sin = cs[:, None, : D // 2], cs[:, None, D // 2:]
    xf = x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(x.dtype)


def qk_norm_rope(x: torch.Tensor, w: torch.Tensor, eps: float, positions: torch.Tensor, cos_sin: torch.Tensor,
                 mutant: Optional[str] = None) -> torch.Tensor:
    """QK-norm + RoPE of heads x [T, H, D] (the kernels' contract, csrc/kernels/rope_cache.hip):
    y = x * rsqrt(mean(x^2) + eps) * w in fp32, rotated in fp32, rounded to x.dtype once.  (HF's
    Qwen3 rounds y to the model dtype before rotating it; in fp32 the two agree.)"""
    def norm(t):
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    xf = x.float()
    if mutant == "after_rope":
        return norm(apply_rope(xf, positions, cos_sin)).to(x.dtype)
    return apply_rope(norm(xf), positions, cos_sin).to(x.dtype)


_KIDX: dict = {}


def kcache_index(bs: int, device=None) -> torch.Tensor:
    """[bs, 128] flat position of K element (token, dim) inside one (block, kv head) slab of the
    paged K cache: fragment-native 32-token tiles (csrc/kernels/common.h ``kcache_off``)."""
    if bs % 32:
        raise ValueError(f"the K-cache layout needs a block size that is a multiple of 32, got {bs}")
    key = (bs, str(device))
    if key not in _KIDX:
        k = torch.arange(bs).view(bs, 1)
        d = torch.arange(128).view(1, 128)
        kt = k & 31
        lane = 16 * (d >> 5) + 4 * (kt >> 3) + (kt & 3)
        _KIDX[key] = ((k >> 5) * 4096 + ((((kt >> 2) & 1) * 4 + ((d >> 3) & 3)) * 64 + lane) * 8 + (d & 7)).to(device)
    return _KIDX[key]


_VIDX: dict = {}


def vcache_index(bs: int, device=None) -> torch.Tensor:
    """[bs, 128] flat position of V element (token, dim) inside one (block, kv head) slab of the
    paged V cache: per 32-token tile [d / 16][key / 8][d % 16][key % 8] (common.h ``vcache_off``)."""
    if bs % 32:
        raise ValueError(f"the V-cache layout needs a block size that is a multiple of 32, got {bs}")
    key = (bs, str(device))
    if key not in _VIDX:
        k = torch.arange(bs).view(bs, 1)
        d = torch.arange(128).view(1, 128)
        kt = k & 31
        _VIDX[key] = ((k >> 5) * 4096 + ((((d >> 4) << 2) + (kt >> 3)) * 16 + (d & 15)) * 8 + (kt & 7)).to(device)
    return _VIDX[key]


def v_cache_logical(v_cache: torch.Tensor) -> torch.Tensor:
    """The physical V cache [blocks, n_kv, 128, bs] as logical (token, dim) rows [blocks, n_kv, bs, 128]."""
    nb, nkv, hd, bs = v_cache.shape
    return v_cache.reshape(nb, nkv, bs * hd)[:, :, vcache_index(bs, v_cache.device).view(-1)].view(nb, nkv, bs, hd)


def k_cache_logical(k_cache: torch.Tensor) -> torch.Tensor:
    """The physical K cache [blocks, n_kv, bs, 128] as logical (token, dim) rows."""
    nb, nkv, bs, hd = k_cache.shape
    return k_cache.reshape(nb, nkv, bs * hd)[:, :, kcache_index(bs, k_cache.device).view(-1)].view(nb, nkv, bs, hd)


FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_fp8(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """The FP8 KV-cache byte of ``x``: e4m3 round-to-nearest-even of clamp(x / scale, -448, 448),
    in fp32 (+-inf and anything beyond +-448 store +-448; subnormals down to 2^-9 are kept)."""
    return (x.float() / scale).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def dequantize_fp8(c: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """fp32 values an FP8 cache holds: scale * byte."""
    return c.float() * scale


def quantize_fp8_rows(w: torch.Tensor):
    """Weight-only FP8 of a ``[N, K]`` projection: one fp32 scale per row (output channel),
    ``scale[n] = max|w[n, :]| / 448`` (an all-zero row: 1.0), bytes = :func:`quantize_fp8` of
    ``w / scale``.  Returns (bytes ``[N, K]`` e4m3, scale ``[N]`` fp32).

    Both quotients are formed in float64 and rounded to fp32, which IS the correctly rounded fp32
    quotient (53 >= 2 * 24 + 2 bits: the second rounding is innocuous), so every device produces
    the bytes the CPU's IEEE division does -- a GPU's own fp32 division may be an ulp off."""
    amax = w.float().abs().amax(dim=1)
    scale = torch.where(amax > 0, (amax.double() / FP8_MAX).float(), torch.ones_like(amax))
    out = torch.empty(w.shape, dtype=FP8, device=w.device)
    rows = 2048  # bounds the float64 temporary of a large projection
    for r in range(0, w.shape[0], rows):
        q = (w[r:r + rows].double() / scale[r:r + rows].double()[:, None]).float()
        out[r:r + rows] = q.clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return out, scale


def w8_linear(x: torch.Tensor, b: torch.Tensor, scale: torch.Tensor, rinv: Optional[torch.Tensor] = None,
              dtype=torch.float32) -> torch.Tensor:
    """The function every W8 projection computes, before its epilogue's rounding:
    ``y[m, n] = (sum_k x[m, k] * widen(b[n, k])) * scale[n]`` (times ``rinv[m]`` with the folded
    norm), products and sums in ``dtype`` (fp32: the ops' CPU path; float64: the tests' reference).
    ``b``: row-major e4m3 ``[N, K]``."""
    y = (x.to(dtype) @ b.to(dtype).t()) * scale.to(dtype)[None, :]
    return y if rinv is None else y * rinv.to(dtype)[:, None]


def w8_linear_f64(x, b, scale, rinv=None) -> torch.Tensor:
    return w8_linear(x, b, scale, rinv, dtype=torch.float64)


# MXFP4 (OCP Microscaling v1.0): e2m1 elements, one e8m0 scale byte per block of 32 along K
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)
MX_BLOCK = 32
MX_SCALE_MIN, MX_SCALE_MAX = 2, 252  # scale bytes for which every e2m1 * 2^(X - 127) is a normal bf16 (or 0)
# twice the magnitude (0, 1, 2, 3, 4, 6, 8, 12) -> e2m1 code
_E2M1_CODE = (0, 1, 2, 3, 4, -1, 5, -1, 6, -1, -1, -1, 7)


def quantize_mxfp4_rows(w: torch.Tensor):
    """Weight-only MXFP4 of a ``[N, K]`` projection (K % 32 == 0), the OCP MX v1.0 rule per block of
    32 along K: ``X = clamp(floor(log2(amax)) - 2 + 127, 2, 252)`` (an all-zero block: 127), elements
    ``w / 2^(X - 127)`` rounded to the nearest e2m1 value with ties to even and saturated at +-6
    (quotients in (6, 8) saturate: the standard's behaviour).  Returns (nibbles ``[N, K / 2]`` uint8,
    low nibble = even k; scales ``[N, K / 32]`` uint8): the interchange layout.

    The quotient is formed in float64, where a division by a power of two is exact."""
    N, K = w.shape
    assert K % MX_BLOCK == 0, f"MXFP4 needs K % 32 == 0 (got {K})"
    nib = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    xs = torch.empty((N, K // MX_BLOCK), dtype=torch.uint8, device=w.device)
    code_of = torch.tensor(_E2M1_CODE, dtype=torch.int64, device=w.device)
    rows = 2048  # bounds the float64 temporary of a large projection
    for r in range(0, N, rows):
        v = w[r:r + rows].double().view(-1, K // MX_BLOCK, MX_BLOCK)
        amax = v.abs().amax(dim=-1)
        # floor(log2(amax)) is the float64 exponent field (bit operations: the same on every device)
        e = ((amax.view(torch.int64) >> 52) & 0x7FF) - 1023
        X = torch.where(amax > 0, (e - 2 + 127).clamp(MX_SCALE_MIN, MX_SCALE_MAX), torch.full_like(e, 127))
        q = v * ((1023 + 127 - X) << 52).view(torch.float64)[..., None]  # times 2^(127 - X), as float64 bits
        a = q.abs()
        # round to nearest even on a grid of step 0.5 below 2, 1 below 4, 2 above: torch.round is
        # half-to-even, and an even multiple of the step is an even e2m1 code
        m = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
        code = code_of[(m.clamp(max=6.0) * 2).long()]
        code = torch.where((q < 0) & (code > 0), code + 8, code).view(-1, K // 2, 2)
        nib[r:r + rows] = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
        xs[r:r + rows] = X.to(torch.uint8)
    return nib, xs


def dequantize_mxfp4(nib: torch.Tensor, xs: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``[N, K]`` values of MXFP4 nibbles ``[N, K / 2]`` and scale bytes ``[N, K / 32]``:
    ``E2M1[nibble] * 2^(X - 127)``, exact in fp32 for X in [2, 252]."""
    N, K = nib.shape[0], nib.shape[1] * 2
    table = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=nib.device)
    n = nib.long()
    v = table[torch.stack([n & 15, n >> 4], dim=-1).view(N, K)]
    scale = (xs.to(torch.int32) << 23).view(torch.float32)  # 2^(X - 127) as fp32 bits
    return (v.view(N, K // MX_BLOCK, MX_BLOCK) * scale[..., None]).view(N, K).to(dtype)


def w4_linear(x: torch.Tensor, nib: torch.Tensor, xs: torch.Tensor, rinv: Optional[torch.Tensor] = None,
              dtype=torch.float32) -> torch.Tensor:
    """The function every W4 projection computes, before its epilogue's rounding:
    ``y[m, n] = sum_k x[m, k] * E2M1[nib[n, k]] * 2^(X[n, k / 32] - 127)`` (times ``rinv[m]`` with the
    folded norm), products and sums in ``dtype`` (fp32: the ops' CPU path; float64: the tests')."""
    y = x.to(dtype) @ dequantize_mxfp4(nib, xs, dtype).t()
    return y if rinv is None else y * rinv.to(dtype)[:, None]


def _store(cache_flat: torch.Tensor, index: tuple, rows: torch.Tensor, scale: float) -> None:
    """cache_flat[index] = rows in the cache's dtype (FP8 caches: quantised, indexed as bytes)."""
    if cache_flat.dtype == FP8:
        cache_flat.view(torch.uint8)[index] = quantize_fp8(rows, scale).view(torch.uint8)
    else:
        cache_flat[index] = rows.to(cache_flat.dtype)


def rope_and_cache(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor,
                   k_cache: Optional[torch.Tensor], v_cache: Optional[torch.Tensor],
                   slot_mapping: Optional[torch.Tensor], nq: int, nkv: int, hd: int,
                   k_scale: float = 1.0, v_scale: float = 1.0, q_norm: Optional[torch.Tensor] = None,
                   k_norm: Optional[torch.Tensor] = None, eps: float = 1e-6,
                   mutant: Optional[str] = None) -> torch.Tensor:
    """Rotate q,k of the fused QKV output in place and scatter k,v into the paged cache (an FP8
    cache gets the quantised values of the rotated, already rounded rows).

    ``q_norm`` / ``k_norm`` ([hd] weights, Qwen3 QK-norm): every q / k head is RMS-normalised and
    weighted before the rotation, in fp32 with ONE rounding after norm + rotation
    (:func:`qk_norm_rope`).  ``mutant`` (tests): ``"after_rope"`` normalises the rotated head."""
    T = qkv.shape[0]
    view = qkv.view(T, nq + 2 * nkv, hd)
    q, k, v = view[:, :nq], view[:, nq:nq + nkv], view[:, nq + nkv:]
    if q_norm is not None:
        q.copy_(qk_norm_rope(q, q_norm, eps, positions, cos_sin, mutant))
        k.copy_(qk_norm_rope(k, k_norm, eps, positions, cos_sin, mutant))
    else:
        q.copy_(apply_rope(q, positions, cos_sin))
        k.copy_(apply_rope(k, positions, cos_sin))
    if k_cache is not None and slot_mapping is not None:
        bs = k_cache.shape[2]
        sm = slot_mapping.long()
        valid = sm >= 0
        if valid.any():
            s = sm[valid]
            blk, off = s // bs, s % bs
            n, nkv_ = blk.numel(), k_cache.shape[1]
            kflat = k_cache.view(k_cache.shape[0], nkv_, bs * hd)
            pos = kcache_index(bs, k_cache.device)[off]  # [n, 128] fragment-native positions
            _store(kflat, (blk.view(n, 1, 1), torch.arange(nkv_, device=k_cache.device).view(1, nkv_, 1),
                           pos.view(n, 1, hd)), k[valid], k_scale)
            vflat = v_cache.view(v_cache.shape[0], nkv_, bs * hd)
            vpos = vcache_index(bs, v_cache.device)[off]
            _store(vflat, (blk.view(n, 1, 1), torch.arange(nkv_, device=v_cache.device).view(1, nkv_, 1),
                           vpos.view(n, 1, hd)), v[valid], v_scale)
    return q


def kv_copy_blocks(kv_caches, pairs) -> None:
    """Block ``dst`` := block ``src`` in every K and V cache of ``kv_caches`` ([(k, v)] per layer), for
    every (src, dst) pair, as raw bytes.  ValueError (nothing written) for what pk_kv_copy_blocks
    refuses: more than 32 pairs, an id outside the cache, src == dst, a dst named twice or also a src."""
    pairs = [(int(s), int(d)) for s, d in pairs]
    nb = kv_caches[0][0].shape[0]
    dsts = [d for _, d in pairs]
    if (len(pairs) > 32 or any(not 0 <= s < nb or not 0 <= d < nb or s == d for s, d in pairs)
            or len(set(dsts)) != len(dsts) or set(dsts) & {s for s, _ in pairs}):
        raise ValueError("kv_copy_blocks: invalid (src, dst) pairs")
    for kv in kv_caches:
        for t in kv:
            raw = t.view(torch.uint8)
            for s, d in pairs:
                raw[d].copy_(raw[s])


# ------------------------------------------------------------------------- attention
def gather_kv(k_cache, v_cache, block_table, n_tokens):
    """→ K [n, n_kv, D], V [n, n_kv, D] for one sequence (FP8 caches: the raw bytes, as FP8)."""
    bs = k_cache.shape[2]
    nb = (n_tokens + bs - 1) // bs
    blocks = block_table[:nb].long()
    if k_cache.dtype == FP8:  # index as bytes
        k, v = gather_kv(k_cache.view(torch.uint8), v_cache.view(torch.uint8), block_table, n_tokens)
        return k.view(FP8), v.view(FP8)
    k = k_cache_logical(k_cache[blocks]).permute(0, 2, 1, 3).reshape(nb * bs, k_cache.shape[1], -1)[:n_tokens]
    v = v_cache_logical(v_cache[blocks]).permute(0, 2, 1, 3).reshape(nb * bs, v_cache.shape[1], -1)[:n_tokens]
    return k, v


def paged_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                    context_lens: torch.Tensor, cu_seqlens_q: torch.Tensor, scale: float,
                    k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """Causal GQA attention of each sequence's new query tokens against its whole paged
    context.  Query ``i`` of a chunk of ``L`` tokens sits at absolute position
    ``ctx - L + i`` and attends to keys ``[0, ctx - L + i]``.  q: [T, nq, D] → [T, nq, D]."""
    T, nq, D = q.shape
    nkv = k_cache.shape[1]
    g = nq // nkv
    out = torch.zeros_like(q)
    cu = cu_seqlens_q.tolist()
    ctxs = context_lens.tolist()
    for s in range(len(ctxs)):
        a, b = cu[s], cu[s + 1]
        L, ctx = b - a, int(ctxs[s])
        if L == 0 or ctx == 0:
            continue
        k, v = gather_kv(k_cache, v_cache, block_tables[s], ctx)
        if k_cache.dtype == FP8:  # attention over scale * byte
            k, v = dequantize_fp8(k, k_scale), dequantize_fp8(v, v_scale)
        k = k.float().repeat_interleave(g, dim=1)  # [ctx, nq, D]
        v = v.float().repeat_interleave(g, dim=1)
        qs = q[a:b].float()  # [L, nq, D]
        scores = torch.einsum("lhd,thd->hlt", qs, k) * scale
        pos = torch.arange(ctx - L, ctx)[:, None]
        keys = torch.arange(ctx)[None, :]
        scores = scores.masked_fill((keys > pos)[None], float("-inf"))
        p = torch.softmax(scores, dim=-1)
        out[a:b] = torch.einsum("hlt,thd->lhd", p, v).to(q.dtype)
    return out


VERIFY_MUTANTS = ("limit+1", "limit-1", "ignore_rows", "head_major", "ctx_excludes_new")


def verify_limits(context_lens, n_rows, qr: int, nq: int, G: int, mutant: Optional[str] = None) -> torch.Tensor:
    """[n_seqs * qr, nq] int64: the last key row ``s * qr + j`` of head ``hq`` attends in a verify
    step, -1 for a row that attends nothing (a padding row ``j >= R``, a sequence with ``C <= 0``).
    The contract: ``C - R + j`` for ``j < R``.

    ``mutant`` (tests) is a deliberate defect: ``"limit+1"`` / ``"limit-1"`` (off by one),
    ``"ignore_rows"`` (R taken as qr: padding rows attend, real rows shift), ``"head_major"`` (the row
    of tile column c = j * G + head taken as c % qr, as if the columns were ordered head-major),
    ``"ctx_excludes_new"`` (C taken as the keys *before* this step's: limit C + j)."""
    assert mutant is None or mutant in VERIFY_MUTANTS, mutant
    lim = torch.full((len(context_lens) * qr, nq), -1, dtype=torch.int64)
    for s, (C, R) in enumerate(zip((int(c) for c in context_lens), (int(r) for r in n_rows))):
        if C <= 0:
            continue
        Rm = qr if mutant == "ignore_rows" else min(R, qr)
        for j in range(Rm):
            for hq in range(nq):
                jl = (j * G + hq % G) % qr if mutant == "head_major" else j
                if jl >= Rm:
                    continue
                l = C - Rm + jl
                l += {"limit+1": 1, "limit-1": -1, "ctx_excludes_new": Rm}.get(mutant, 0)
                lim[s * qr + j, hq] = max(l, -1)
    return lim


def paged_verify(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                 context_lens, n_rows, qr: int, scale: float, dtype=torch.float32, mutant: Optional[str] = None):
    """Attention of a verify step (speculative decoding), sums in ``dtype`` (float64: the tests'
    reference).  q: [n_seqs * qr, nq, D]; sequence s owns rows ``s * qr + j``, the first
    ``R = n_rows[s]`` of them real; ``C = context_lens[s]`` counts the cached keys including the R
    written this step.  Every (row, head) attends keys ``0 .. verify_limits(...)``; a limit of -1
    gives zeros.  -> (out, A) both [n_seqs * qr, nq, D] in ``dtype``, ``A = sum_j p_j |v_j|`` (what a
    rounding bound is measured against).  A mutant's limit may reach past C (never past the block
    table's capacity): it then reads whatever the cache holds there."""
    T, nq, D = q.shape
    nkv = k_cache.shape[1]
    G = nq // nkv
    lim = verify_limits(context_lens, n_rows, qr, nq, G, mutant)
    out = torch.zeros((T, nq, D), dtype=dtype)
    A = torch.zeros((T, nq, D), dtype=dtype)
    cap = block_tables.shape[1] * k_cache.shape[2]
    for s in range(len(context_lens)):
        n = min(int(lim[s * qr:(s + 1) * qr].max()) + 1, cap)
        if n <= 0:
            continue
        k, v = gather_kv(k_cache, v_cache, block_tables[s], n)
        k, v = k.to(dtype), v.to(dtype)
        for j in range(qr):
            for hq in range(nq):
                m = min(int(lim[s * qr + j, hq]) + 1, n)
                if m <= 0:
                    continue
                p = torch.softmax((k[:m, hq // G] @ q[s * qr + j, hq].to(dtype)) * scale, dim=0)
                out[s * qr + j, hq] = p @ v[:m, hq // G]
                A[s * qr + j, hq] = p @ v[:m, hq // G].abs()
    return out, A


# --------------------------------------------------------------------------- sampling
_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h: np.ndarray) -> np.ndarray:
    h = h & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def philox_uniform(seed: int, offset: int, n: int) -> np.ndarray:
    """The kernel's counter-based uniform(0,1) stream, bit-exact (uint32 arithmetic)."""
    s = np.uint64(seed & 0xFFFFFFFF)
    h = (s * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & _M32
    h = (h ^ ((np.uint64(offset & 0xFFFFFFFF) + np.uint64(0x85EBCA6B) + ((h << np.uint64(6)) & _M32)
               + (h >> np.uint64(2))) & _M32)) & _M32
    h = _fmix32(np.array(h, dtype=np.uint64))
    idx = np.arange(n, dtype=np.uint64)
    x = _fmix32(h ^ ((idx * np.uint64(0xC2B2AE35)) & _M32))
    return ((x >> np.uint64(8)).astype(np.float64) + 0.5) * (1.0 / (1 << 24))


def sampling_mask(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, min_p: float) -> torch.Tensor:
    """Boolean mask of tokens allowed by top-k → top-p → min-p (sort-based, HF order)."""
    x = logits.float() / max(temperature, 1e-6)
    V = x.shape[-1]
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        kth = torch.topk(x, top_k).values[..., -1:]
        keep &= x >= kth
    if 0.0 < top_p < 1.0:
        xm = x.masked_fill(~keep, float("-inf"))
        p = torch.softmax(xm, -1)
        sp, idx = torch.sort(p, descending=True)
        before = torch.cumsum(sp, -1) - sp
        k_sorted = before < top_p
        k_sorted[..., 0] = True
        m = torch.zeros_like(keep)
        m.scatter_(-1, idx, k_sorted)
        # ties with the smallest kept value stay in (threshold semantics of the kernel)
        thr = torch.where(m, x, torch.full_like(x, float("inf"))).min(-1, keepdim=True).values
        keep &= x >= thr
    if min_p > 0.0:
        p = torch.softmax(x, -1)
        keep &= p >= min_p * p.max(-1, keepdim=True).values
    return keep


def sample(logits: torch.Tensor, temperature, top_k, top_p, min_p, seeds, offsets) -> torch.Tensor:
    """Row-wise sampling with the kernel's RNG: greedy when temperature == 0, otherwise
    Gumbel-max over the allowed set.  Returns int64 [B]."""
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.long)
    for b in range(B):
        t = float(temperature[b])
        row = logits[b].float().cpu()
        if t <= 0.0:
            out[b] = int(torch.argmax(row))
            continue
        keep = sampling_mask(row[None], t, int(top_k[b]), float(top_p[b]), float(min_p[b]))[0]
        u = torch.from_numpy(philox_uniform(int(seeds[b]), int(offsets[b]), V))
        gumbel = -torch.log(-torch.log(u))
        score = (row.double() / t + gumbel).masked_fill(~keep, float("-inf"))
        out[b] = int(torch.argmax(score))
    return out


def logprobs(logits: torch.Tensor, tokens, n_top, out: torch.Tensor = None) -> torch.Tensor:
    """Log-probabilities of the sampled token and the top-n list, from the raw logits, in float64.

    Per row: ``lse = max + log(sum(exp(x - max)))``; the sampled token gets ``x[t] - lse``; the
    top list holds the ``n`` largest entries in the order (value descending, id ascending) --
    a stable descending sort.  A row whose maximum is -inf reports -inf everywhere.  Output: the
    kernel's packed int32 ``[B, 41]`` rows ``[logprob | 20 ids | 20 logprobs]`` (fp32 bits); rows
    with ``n_top < 0`` are left as they are, slots ``n..19`` hold -1 / -inf."""
    B, V = logits.shape
    nmax = 20
    if out is None:
        out = torch.zeros((B, 1 + 2 * nmax), dtype=torch.int32)
    if all(int(n) < 0 for n in n_top[:B]):
        return out
    x = logits.detach().cpu().double()
    fl = out.view(torch.float32)
    ninf = float("-inf")
    for b in range(B):
        n = int(n_top[b])
        if n < 0:
            continue
        n = min(n, nmax, V)
        row = x[b]
        m = float(row.max())
        dead = m == ninf
        lse = ninf if dead else m + float(torch.log(torch.exp(row - m).sum()))
        t = int(tokens[b])
        fl[b, 0] = ninf if dead or not 0 <= t < V else float(row[t]) - lse
        out[b, 1:1 + nmax] = -1
        fl[b, 1 + nmax:] = ninf
        if n:
            vals, idx = torch.sort(row, descending=True, stable=True)
            out[b, 1:1 + n] = idx[:n].to(torch.int32)
            if not dead:
                fl[b, 1 + nmax:1 + nmax + n] = (vals[:n] - lse).float()
    return out


def prompt_logprobs(logits: torch.Tensor, targets, n_top, out: torch.Tensor = None) -> torch.Tensor:
    """Log-probability, rank and top-n list of a *given* target per row, from the raw logits, in
    float64 (the CPU engine's prompt logprobs).

    As :func:`logprobs`, plus the target's 1-based rank in the total order (value descending, id
    ascending, -0.0 == +0.0): ``1 + #{j : x_j > x_t, or x_j == x_t and j < t}``, counted on the
    exact values.  Output: packed int32 ``[R, 42]`` rows ``[logprob | rank | 20 ids | 20 logprobs]``;
    rows with ``targets < 0`` or ``n_top < 0`` are left as they are; ``targets >= V`` reports
    logprob -inf and rank 0; a row whose maximum is -inf reports -inf and the rank by the formula."""
    R, V = logits.shape
    nmax = 20
    if out is None:
        out = torch.zeros((R, 2 + 2 * nmax), dtype=torch.int32)
    if all(int(n_top[r]) < 0 or int(targets[r]) < 0 for r in range(R)):
        return out
    x = logits.detach().cpu().double()
    fl = out.view(torch.float32)
    ninf = float("-inf")
    for r in range(R):
        n, t = int(n_top[r]), int(targets[r])
        if n < 0 or t < 0:
            continue
        n = min(n, nmax, V)
        row = x[r]
        m = float(row.max())
        dead = m == ninf
        lse = ninf if dead else m + float(torch.log(torch.exp(row - m).sum()))
        if t < V:
            xt = row[t]
            fl[r, 0] = ninf if dead else float(xt) - lse
            out[r, 1] = 1 + int((row > xt).sum()) + int((row[:t] == xt).sum())
        else:
            fl[r, 0] = ninf
            out[r, 1] = 0
        out[r, 2:2 + nmax] = -1
        fl[r, 2 + nmax:] = ninf
        if n:
            vals, idx = torch.sort(row, descending=True, stable=True)
            out[r, 2:2 + n] = idx[:n].to(torch.int32)
            if not dead:
                fl[r, 2 + nmax:2 + nmax + n] = (vals[:n] - lse).float()
    return out


# --------------------------------------------------------------------------- sampling penalties
# The device state of ops/penalties.py, on the same packed table: counts int16 [n_slots, Vs],
# bit 15 = token in the prompt, bits 0..14 = occurrences among the generated tokens (saturating).
PENALTY_MAX_BIAS = 300
PENALTY_ENTRY_WORDS = 6  # slot, start, n_prompt, n_out, n_bias, clear


def _u16(t: torch.Tensor) -> np.ndarray:
    return t.numpy().view(np.uint16)


def penalty_seed(counts, bias_ids, bias_vals, bias_n, entries, ids, V: int) -> None:
    """Entries ``[n, 6]`` of (slot, start, n_prompt, n_out, n_bias, clear) over the int32 stream
    ``ids``: prompt flags from ``ids[start:start+n_prompt]``, counts from the next ``n_out``, then
    ``n_bias`` bias ids and ``n_bias`` fp32 bit patterns.  ``clear`` wipes the slot first; without
    it the entry appends.  Out-of-range slots, ids and entries that overrun the stream are ignored."""
    c = _u16(counts)
    n_slots = c.shape[0]
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    for e in np.asarray(entries, dtype=np.int64).reshape(-1, PENALTY_ENTRY_WORDS):
        slot, start, n_p, n_o, n_b, clear = (int(v) for v in e)
        if not 0 <= slot < n_slots or min(start, n_p, n_o, n_b) < 0 or start + n_p + n_o + 2 * n_b > ids.size:
            continue
        if clear:
            c[slot] = 0
            bias_n[slot] = 0
        base = min(max(int(bias_n[slot]), 0), PENALTY_MAX_BIAS)
        p = ids[start:start + n_p]
        c[slot, p[(p >= 0) & (p < V)]] |= 0x8000
        for t in ids[start + n_p:start + n_p + n_o]:
            if 0 <= t < V and (c[slot, t] & 0x7FFF) != 0x7FFF:
                c[slot, t] += 1
        b0 = start + n_p + n_o
        k = max(0, min(n_b, PENALTY_MAX_BIAS - base))
        bias_ids[slot, base:base + k] = torch.from_numpy(ids[b0:b0 + k].copy())
        bias_vals[slot, base:base + k] = torch.from_numpy(ids[b0 + n_b:b0 + n_b + k].copy().view(np.float32))
        bias_n[slot] = min(base + n_b, PENALTY_MAX_BIAS)


def penalty_apply(logits, counts, slots, rep, freq, pres, bias_ids, bias_vals, bias_n, out=None,
                  dtype=np.float32):
    """Rows with ``slots[r]`` in range: ``out[slot, :V]`` = the row after repetition (seen tokens:
    ``x / r`` if ``x > 0`` else ``x * r``), frequency and presence (``x - f * c``, then ``- p``
    where ``c > 0``) and bias (``+ b``), in that order.  ``dtype=np.float32`` rounds once per
    operation (what the kernel computes); ``np.float64`` is the unrounded value a derived bound
    is measured from (then a new float64 ``[n_slots, V]`` array is returned, NaN where untouched).
    The logits are never written."""
    B, V = logits.shape
    c = _u16(counts)
    n_slots = c.shape[0]
    x = logits.detach().float().cpu().numpy()
    if dtype == np.float64:
        res = np.full((n_slots, V), np.nan, dtype=np.float64)
    else:
        res = out.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(B):
            slot = int(slots[r])
            if not 0 <= slot < n_slots:
                continue
            a = x[r].astype(dtype)
            w = c[slot, :V]
            rp, f, p = (dtype(float(v[r])) for v in (rep, freq, pres))
            seen = w != 0
            a = np.where(seen, np.where(a > 0, a / rp, a * rp), a)
            cnt = (w & 0x7FFF).astype(dtype)
            a = np.where(cnt > 0, (a - f * cnt) - p, a)
            for j in range(min(max(int(bias_n[slot]), 0), PENALTY_MAX_BIAS)):
                t = int(bias_ids[slot, j])
                if 0 <= t < V:
                    a[t] = a[t] + dtype(float(bias_vals[slot, j]))
            res[slot, :V] = a
    return res if dtype == np.float64 else out


def penalty_update(counts, slots, tokens, V: int) -> None:
    """``counts[slots[r], tokens[r]]`` += 1 (saturating at 0x7fff, bit 15 kept) for rows with a slot."""
    c = _u16(counts)
    for r in range(len(slots)):
        slot, t = int(slots[r]), int(tokens[r])
        if 0 <= slot < c.shape[0] and 0 <= t < V and (c[slot, t] & 0x7FFF) != 0x7FFF:
            c[slot, t] += 1


# --------------------------------------------------------------------------- guided decoding
# The device state of ops/grammar.py.  A pool entry is GRAMMAR_TABLE_WORDS int32 words holding one
# byte DFA (engine/grammar.py): [0] states S, [1] byte classes C, [2:4] zero, [4:68] the class of
# every byte (256 x uint8), [68:132] one accept bit per state (bit s & 31 of word s >> 5), then
# trans[S][C] as int16, two per word, little end first; -1 = DEAD.  An entry whose S or C is out
# of range (a never-loaded one holds zeros) is no table.  A slot record is GRAMMAR_SLOT_WORDS
# words: table entry (-1 = none), current state (-1 = DEAD), number of end ids, 17 end ids.
GRAMMAR_MAX_STATES = 2048
GRAMMAR_N_TABLES = 16
GRAMMAR_MAX_END = 17
GRAMMAR_HEAD_WORDS = 132
GRAMMAR_TABLE_WORDS = GRAMMAR_HEAD_WORDS + GRAMMAR_MAX_STATES * 256 // 2
GRAMMAR_SLOT_WORDS = 3 + GRAMMAR_MAX_END
GRAMMAR_SEED_WORDS = 4 + GRAMMAR_MAX_END  # slot, table entry, state, number of end ids, 17 end ids


def grammar_pack(cmap, trans, accept) -> np.ndarray:
    """A DFA (``cmap`` uint8[256], ``trans`` int16[S, C], ``accept`` bool[S]) as the int32 words of
    a pool entry, cut after the last transition."""
    S, C = trans.shape
    assert 1 <= S <= GRAMMAR_MAX_STATES and 1 <= C <= 256 and int(np.max(cmap)) < C
    t = np.ascontiguousarray(trans, dtype="<i2").reshape(-1)
    if t.size % 2:
        t = np.concatenate([t, np.zeros(1, dtype="<i2")])
    bits = np.zeros(GRAMMAR_MAX_STATES, dtype=np.uint8)
    bits[:S] = np.asarray(accept, dtype=np.uint8)
    acc = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
    head = np.array([S, C, 0, 0], dtype=np.int32)
    return np.concatenate([head, np.asarray(cmap, dtype=np.uint8).view("<i4"), acc, t.view("<i4")]).astype(np.int32)


def _grammar_table(words: np.ndarray):
    """Pool entry words → (cmap, trans int16[S, C], accept bool[S]) or None for no table."""
    S, C = int(words[0]), int(words[1])
    if not (1 <= S <= GRAMMAR_MAX_STATES and 1 <= C <= 256):
        return None
    cmap = words[4:68].view(np.uint8)
    acc = np.unpackbits(words[68:132].view(np.uint8), bitorder="little")[:S].astype(bool)
    trans = words[GRAMMAR_HEAD_WORDS:GRAMMAR_HEAD_WORDS + (S * C + 1) // 2].view(np.int16)[:S * C].reshape(S, C)
    return cmap, trans, acc


def grammar_load(pool, entry: int, word_off: int, words) -> None:
    """``pool[entry, word_off:word_off + len(words)] = words``; a chunk that does not fit is ignored."""
    w = np.asarray(words, dtype=np.int32).reshape(-1)
    if not 0 <= entry < pool.shape[0] or word_off < 0 or word_off + w.size > pool.shape[1]:
        return
    pool[entry, word_off:word_off + w.size] = torch.from_numpy(w.copy())


def grammar_seed(rec, entries) -> None:
    """Entries ``[n, 21]`` of (slot, table entry, state, number of end ids, 17 end ids) → slot records."""
    for e in np.asarray(entries, dtype=np.int32).reshape(-1, GRAMMAR_SEED_WORDS):
        if 0 <= int(e[0]) < rec.shape[0]:
            rec[int(e[0])] = torch.from_numpy(e[1:].copy())


def _grammar_row(pool, rec, slot: int):
    """→ (table, state, end ids) of a slot, or None when it is out of range or holds no table."""
    if not 0 <= slot < rec.shape[0]:
        return None
    r = rec[slot].numpy()
    tab = int(r[0])
    if not 0 <= tab < pool.shape[0]:
        return None
    table = _grammar_table(pool[tab].numpy())
    if table is None:
        return None
    S = table[1].shape[0]
    state = int(r[1]) if 0 <= int(r[1]) < S else -1
    ends = r[3:3 + min(max(int(r[2]), 0), GRAMMAR_MAX_END)]
    return table, state, ends


def _grammar_walk_all(table, state: int, off: np.ndarray, data: np.ndarray, V: int, mutant=None) -> np.ndarray:
    """The state every id ``< V`` leads to from ``state`` (-1 = DEAD), all ids at once."""
    cmap, trans, _ = table
    S, C = trans.shape
    lens = np.diff(off[:V + 1]).astype(np.int64)
    if mutant == "drop_last_byte":
        lens = np.maximum(lens - 1, 0)
    st = np.full(V, state, dtype=np.int64)
    start = off[:V].astype(np.int64)
    for j in range(int(lens.max()) if V else 0):
        act = np.nonzero((lens > j) & (st >= 0))[0]
        if act.size == 0:
            break
        cls = cmap[data[start[act] + j]].astype(np.int64)
        nxt = trans[st[act], np.minimum(cls, C - 1)].astype(np.int64)
        nxt[(cls >= C) | (nxt >= S)] = -1
        st[act] = nxt
    return st


def grammar_mask(out, V: int, pool, rec, slots, B: int, off, data, mutant=None) -> None:
    """In place on the fp32 rows ``out[slots[r]]`` of every ``r < B`` whose slot holds a table, for
    every id ``t < V``: an end id is kept iff the state accepts (at DEAD end ids are kept); an id
    with no bytes is dropped; any other id is kept iff walking its bytes from the current state
    never hits DEAD.  Dropped = -inf, kept = untouched.  ``mutant`` names a deliberate defect
    (tests/grammar_cases.py)."""
    off = np.asarray(off)
    data = np.asarray(data)
    o = out.numpy()
    for r in range(B):
        slot = int(slots[r])
        row = _grammar_row(pool, rec, slot)
        if mutant == "next_table" and 0 <= slot < rec.shape[0] and int(rec[slot, 0]) >= 0:
            t2 = _grammar_table(pool[(int(rec[slot, 0]) + 1) % pool.shape[0]].numpy())
            row = None if t2 is None or row is None else (t2, row[1] if row[1] < t2[1].shape[0] else -1, row[2])
        if row is None:
            continue
        table, state, ends = row
        walk_from = 0 if mutant == "from_state_0" else state
        fin = _grammar_walk_all(table, walk_from, off, data, V, mutant)
        keep = fin >= 0
        if mutant != "keep_empty":
            keep &= np.diff(off[:V + 1]) > 0
        end_ok = state < 0 or bool(table[2][state]) or mutant == "keep_end"
        for t in ends:
            if 0 <= int(t) < V:
                keep[int(t)] = end_ok
        o[slot, :V][~keep] = -np.inf


def grammar_advance(pool, rec, slots, tokens, n: int, off, data, V: int, mutant=None) -> None:
    """After sampling, per row with a table: an end id leaves the state alone, any other id ``< V``
    moves it along the id's bytes (DEAD stays DEAD)."""
    off = np.asarray(off)
    data = np.asarray(data)
    for r in range(n):
        slot, t = int(slots[r]), int(tokens[r])
        row = _grammar_row(pool, rec, slot)
        if row is None or not 0 <= t < V:
            continue
        (cmap, trans, _), state, ends = row
        if mutant != "advance_on_end" and t in [int(x) for x in ends]:
            continue
        S, C = trans.shape
        for b in data[off[t]:off[t + 1]]:
            if state < 0:
                break
            c = int(cmap[b])
            state = int(trans[state, c]) if c < C else -1
            if state >= S:
                state = -1
        rec[slot, 1] = state


# ------------------------------------------------------------------------------ LoRA
def lora_col_segments(N: int, b0: int, b1: int, il: int, device=None) -> torch.Tensor:
    """Rank block of every output column of a fused projection (csrc/kernels/lora.hip seg(n)):
    ``il > 0``: gate / up columns interleaved by ``il``; else the q | k | v boundaries b0 <= b1."""
    n = torch.arange(N, device=device)
    if il > 0:
        return (n // il) & 1
    return (n >= b0).long() + (n >= b1).long()


def lora_shrink(x: torch.Tensor, A: torch.Tensor, idx: torch.Tensor, parts: Optional[torch.Tensor] = None,
                eps: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t [M, R] = round(rinv[m] * x[m] @ A[idx[m]]^T) with fp32 products and sums and ONE rounding,
    to the activation dtype (``out``'s: bf16 wherever the GPU kernels run, float32 in a float32 model);
    ``A`` [slots, R, K] (zero-padded ranks), ``parts`` [nparts, M] sums of squares of the rows
    (rinv = 1 / sqrt(sum / K + eps)) or None.  Rows with an index outside [0, slots) are neither
    read nor written (``out`` keeps them; a fresh ``out`` holds zeros there)."""
    M, K = x.shape
    S, R, _ = A.shape
    if out is None:
        out = torch.zeros((M, R), dtype=torch.bfloat16, device=x.device)
    idx = idx[:M].long()
    for s in range(S):
        rows = (idx == s).nonzero().flatten()
        if rows.numel() == 0:
            continue
        t = x[rows].float() @ A[s].float().t()
        if parts is not None:
            ss = parts[:, :M].float().sum(0)[rows]
            t = t * (1.0 / torch.sqrt(ss / K + eps))[:, None]
        out[rows] = t.to(out.dtype)
    return out


def lora_expand(out: torch.Tensor, t: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, idx: torch.Tensor,
                b0: int, b1: int, il: int) -> torch.Tensor:
    """out[m, n] += scale[idx[m]] * sum_j B[idx[m]][n, j] * t[m, seg(n) * seg_r + j], in place;
    ``B`` [slots, N, seg_r], fp32 products and sums, the scale applied last.  fp32 ``out`` (a
    split-K slab) is added to in fp32; bf16 ``out`` becomes bf16(float(out) + delta)."""
    M, N = out.shape
    S, _, seg_r = B.shape
    seg = lora_col_segments(N, b0, b1, il, out.device)
    cols = seg[:, None] * seg_r + torch.arange(seg_r, device=out.device)[None, :]  # [N, seg_r] into t's row
    idx = idx[:M].long()
    for s in range(S):
        rows = (idx == s).nonzero().flatten()
        if rows.numel() == 0:
            continue
        tt = t[rows].float()[:, cols]  # [rows, N, seg_r]
        delta = (tt * B[s].float()[None]).sum(-1) * scale[s].float()
        out[rows] = (out[rows].float() + delta).to(out.dtype)
    return out
