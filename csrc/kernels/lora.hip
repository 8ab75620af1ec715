// Multi-LoRA shrink / expand for gfx950: per-row adapters on top of a shared base projection.
//
//   shrink   t[m, j]   = bf16( rinv[m] * sum_k x[m, k] * A[slot(m)][j, k] )        j < R
//   expand   out[m, n] += s[slot(m)] * sum_j B[slot(m)][n, j] * t[m, seg(n) * seg_r + j]   j < seg_r
//
// fp32 products and sums; t is rounded to bf16 once, after the optional row scale; s multiplies the
// finished fp32 sum.  slot(m) = idx[m]; a row whose index is outside [0, n_slots) is neither read
// nor written.  Adapters are stored zero-padded to seg_r ranks per sub-projection; ranks[slot]
// (optional) is the real rank, and rank columns at or above it are written as zero (shrink) and
// not read (expand), which is the same value.
//
// A fused projection (qkv, interleaved gate_up) stacks its sub-projections' A along the rank axis
// (R = nseg * seg_r) and stores B rows in the fused order of the weight; seg(n) picks the rank
// block of column n:  il > 0: (n / il) & 1 (gate / up rows interleaved by il), else
// (n >= b0) + (n >= b1) (q | k | v boundaries).
//
// Both grids depend on the shapes only, never on idx, so a captured launch stays valid when the
// index buffer is rewritten between replays.  Work mapping (VALU dot products):
//   shrink: a workgroup owns kRows consecutive rows x 4 rank columns; its four waves split K and
//           combine through LDS.  When the tile's rows share one adapter (a prefill sequence, a
//           one-adapter batch) every A vector is loaded once for the kRows rows; in a mixed tile
//           every row reads its own slot's A.  A workgroup whose columns lie at or above the rank
//           of every row's adapter writes zeros and reads nothing.
//   expand: a workgroup owns kRows rows x 256 columns, a thread one column; its B row stays in
//           registers while consecutive rows keep the same adapter.
#include "common.h"

using namespace pk;

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 8;       // rows per workgroup
constexpr int kJW = 4;         // rank columns per workgroup (shrink)
constexpr int kMaxSegVec = 8;  // expand keeps seg_r <= 64 ranks of B in registers

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int slot_of(const int* idx, int m, int M, int n_slots) {
  if (m >= M) return -1;
  const int s = idx[m];
  return (s >= 0 && s < n_slots) ? s : -1;
}

// rinv of row m from the sum-of-squares parts [nparts, M] (every lane returns it)
__device__ __forceinline__ float row_rinv(const float* parts, int nparts, int M, int m, int K, float eps, int lane) {
  float ss = 0.f;
  for (int p = lane; p < nparts; p += 64) ss += parts[static_cast<int64_t>(p) * M + m];
  ss = wave_sum(ss);
  return 1.0f / sqrtf(ss / static_cast<float>(K) + eps);
}

__global__ void __launch_bounds__(kThreads) shrink_kernel(bf16_t* __restrict__ t, const bf16_t* __restrict__ x,
                                                          int64_t ldx, const bf16_t* __restrict__ A,
                                                          const int* __restrict__ idx, const int* __restrict__ ranks,
                                                          int M, int K, int R, int seg_r, int n_slots,
                                                          const float* __restrict__ parts, int nparts, float eps) {
  __shared__ float red[kThreads / 64][kRows * kJW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.y * kRows;
  const int j0 = blockIdx.x * kJW;
  const int KV = K / 8;
  // the tile's slots and ranks (block-uniform: every thread reads the same kRows indices)
  int slots[kRows], rk[kRows];
  bool uniform = true, any = false;
  // rank columns of this workgroup, clamped for the loads; a column past R is never stored
  int jc[kJW];
#pragma unroll
  for (int q = 0; q < kJW; ++q) jc[q] = min(j0 + q, R - 1);
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    slots[r] = slot_of(idx, m0 + r, M, n_slots);
    rk[r] = slots[r] < 0 ? 0 : (ranks ? ranks[slots[r]] : seg_r);
    uniform = uniform && slots[r] >= 0 && slots[r] == slots[0];
    // (rank columns of one workgroup never straddle two rank blocks: seg_r % kJW == 0 is checked by the launcher)
    any = any || (jc[0] % seg_r) < rk[r];
  }
  if (!any) {  // every column is at or above every row's rank (or no row has a slot): zeros, nothing read
    const int r = threadIdx.x / kJW, q = threadIdx.x % kJW;
    if (r < kRows && slots[r] >= 0 && j0 + q < R) t[static_cast<int64_t>(m0 + r) * R + j0 + q] = bf16_t(0);
    return;
  }
  float acc[kRows][kJW];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int q = 0; q < kJW; ++q) acc[r][q] = 0.f;
  // the workgroup's four waves split K; each lane keeps kRows x kJW partial sums
  if (uniform) {  // one adapter: every A vector is loaded once for the kRows rows
    const u32x4* Ap[kJW];
#pragma unroll
    for (int q = 0; q < kJW; ++q)
      Ap[q] = reinterpret_cast<const u32x4*>(A + (static_cast<int64_t>(slots[0]) * R + jc[q]) * K);
    for (int v = threadIdx.x; v < KV; v += kThreads) {
      float a[kJW][8];
#pragma unroll
      for (int q = 0; q < kJW; ++q) unpack8(Ap[q][v], a[q]);
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        float xv[8];
        unpack8(reinterpret_cast<const u32x4*>(x + (m0 + r) * ldx)[v], xv);
#pragma unroll
        for (int q = 0; q < kJW; ++q)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][q] = fmaf(xv[e], a[q][e], acc[r][q]);
      }
    }
  } else {  // mixed adapters (or rows without one): every row reads its own slot's A
    for (int v = threadIdx.x; v < KV; v += kThreads) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (slots[r] < 0 || (jc[0] % seg_r) >= rk[r]) continue;  // block-uniform
        float xv[8];
        unpack8(reinterpret_cast<const u32x4*>(x + (m0 + r) * ldx)[v], xv);
        const bf16_t* Ar = A + static_cast<int64_t>(slots[r]) * R * K;
#pragma unroll
        for (int q = 0; q < kJW; ++q) {
          float a[8];
          unpack8(reinterpret_cast<const u32x4*>(Ar + static_cast<int64_t>(jc[q]) * K)[v], a);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][q] = fmaf(xv[e], a[e], acc[r][q]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int q = 0; q < kJW; ++q) {
      const float s = wave_sum(acc[r][q]);
      if (lane == 0) red[wave][r * kJW + q] = s;
    }
  __syncthreads();
  // wave 0: one lane per (row, column) adds the four waves' sums; the row scale is computed by
  // the whole wave (row_rinv reduces over lanes), row by row
  if (wave != 0) return;
  float rinv_of[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
    rinv_of[r] = (parts && slots[r] >= 0) ? row_rinv(parts, nparts, M, m0 + r, K, eps, lane) : 1.f;
  if (lane < kRows * kJW) {
    const int r = lane / kJW, q = lane % kJW;
    float rinv = 1.f;
    int slot = -1, rank = 0;
#pragma unroll
    for (int rr = 0; rr < kRows; ++rr)
      if (rr == r) {
        rinv = rinv_of[rr];
        slot = slots[rr];
        rank = rk[rr];
      }
    if (slot >= 0 && j0 + q < R) {
      const float s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
      t[static_cast<int64_t>(m0 + r) * R + j0 + q] = ((j0 + q) % seg_r) < rank ? f2bf(s * rinv) : bf16_t(0);
    }
  }
}

template <bool F32>
__global__ void __launch_bounds__(kThreads) expand_kernel(void* __restrict__ out, int64_t ldo,
                                                          const bf16_t* __restrict__ t, const bf16_t* __restrict__ B,
                                                          const float* __restrict__ scale, const int* __restrict__ idx,
                                                          const int* __restrict__ ranks, int M, int N, int R, int seg_r,
                                                          int b0, int b1, int il, int n_slots) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int m0 = blockIdx.y * kRows;
  const int seg = il > 0 ? (n / il) & 1 : (n >= b0) + (n >= b1);
  const int SV = seg_r / 8;
  float b[kMaxSegVec][8];
  int cur = -1, nv = 0;
  float s = 0.f;
  for (int r = 0; r < kRows; ++r) {
    const int m = m0 + r;
    const int slot = slot_of(idx, m, M, n_slots);
    if (slot < 0) continue;
    if (slot != cur) {
      cur = slot;
      const int rk = ranks ? min(ranks[slot], seg_r) : seg_r;
      nv = (rk + 7) / 8;  // padding past the rank is zero: a whole vector may be read
      s = scale[slot];
      const u32x4* bp = reinterpret_cast<const u32x4*>(B + (static_cast<int64_t>(slot) * N + n) * seg_r);
#pragma unroll
      for (int v = 0; v < kMaxSegVec; ++v)
        if (v < nv && v < SV) unpack8(bp[v], b[v]);
    }
    const u32x4* tp = reinterpret_cast<const u32x4*>(t + static_cast<int64_t>(m) * R + seg * seg_r);
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < kMaxSegVec; ++v) {
      if (v < nv && v < SV) {
        float tv[8];
        unpack8(tp[v], tv);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(b[v][e], tv[e], acc);
      }
    }
    const float delta = s * acc;
    if (F32) {
      float* o = static_cast<float*>(out) + m * ldo + n;
      *o = *o + delta;
    } else {
      bf16_t* o = static_cast<bf16_t*>(out) + m * ldo + n;
      *o = f2bf(bf2f(*o) + delta);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// t bf16 [M, R] <- bf16(rinv * x[M, K] (row stride ldx) * A[idx[m]]^T), A bf16 [n_slots, R, K].
// parts: fp32 [nparts, M] sums of squares (rinv = 1 / sqrt(sum / K + eps)) or null for no row scale.
// ranks: int32 [n_slots] real ranks (columns j with j % seg_r >= rank are written as zero) or null.
PK_EXPORT int pk_lora_shrink(void* t, const void* x, int64_t ldx, const void* A, const void* idx, const void* ranks,
                             int M, int K, int R, int seg_r, int n_slots, const void* parts, int nparts, float eps,
                             hipStream_t stream) {
  if (M <= 0) return 0;
  if (K <= 0 || K % 8 || ldx % 8 || ldx < K || R <= 0 || seg_r <= 0 || seg_r % kJW || R % seg_r || n_slots <= 0)
    return -1;
  if (!aligned16(x) || !aligned16(A) || (parts && nparts <= 0)) return -1;
  dim3 grid((R + kJW - 1) / kJW, (M + kRows - 1) / kRows);
  shrink_kernel<<<grid, kThreads, 0, stream>>>(static_cast<bf16_t*>(t), static_cast<const bf16_t*>(x), ldx,
                                               static_cast<const bf16_t*>(A), static_cast<const int*>(idx),
                                               static_cast<const int*>(ranks), M, K, R, seg_r, n_slots,
                                               static_cast<const float*>(parts), nparts, eps);
  return PK_CHECK_LAUNCH();
}

// out[m, n] += scale[idx[m]] * B[idx[m]][n, :] . t[m, seg(n) * seg_r : +seg_r];  B bf16 [n_slots, N, seg_r],
// t bf16 [M, R], scale fp32 [n_slots].  out_f32 = 1: fp32 [M, N] (row stride ldo, a split-K slab);
// 0: bf16, out = bf16(float(out) + delta).  seg(n): il > 0 ? (n / il) & 1 : (n >= b0) + (n >= b1).
PK_EXPORT int pk_lora_expand(void* out, int64_t ldo, int out_f32, const void* t, const void* B, const void* scale,
                             const void* idx, const void* ranks, int M, int N, int R, int seg_r, int b0, int b1,
                             int il, int n_slots, hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || ldo < N || seg_r <= 0 || seg_r % 8 || seg_r > 8 * kMaxSegVec || R % seg_r || n_slots <= 0) return -1;
  const int nseg = R / seg_r;
  const int top = il > 0 ? 1 : (b0 < N) + (b1 < N);  // the largest segment a column can name
  if (il < 0 || top >= nseg || b0 > b1) return -1;
  if (!aligned16(t) || !aligned16(B)) return -1;
  dim3 grid((N + kThreads - 1) / kThreads, (M + kRows - 1) / kRows);
  if (out_f32)
    expand_kernel<true><<<grid, kThreads, 0, stream>>>(out, ldo, static_cast<const bf16_t*>(t),
                                                       static_cast<const bf16_t*>(B), static_cast<const float*>(scale),
                                                       static_cast<const int*>(idx), static_cast<const int*>(ranks), M,
                                                       N, R, seg_r, b0, b1, il, n_slots);
  else
    expand_kernel<false><<<grid, kThreads, 0, stream>>>(out, ldo, static_cast<const bf16_t*>(t),
                                                        static_cast<const bf16_t*>(B), static_cast<const float*>(scale),
                                                        static_cast<const int*>(idx), static_cast<const int*>(ranks), M,
                                                        N, R, seg_r, b0, b1, il, n_slots);
  return PK_CHECK_LAUNCH();
}
