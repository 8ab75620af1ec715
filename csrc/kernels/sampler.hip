// Token sampler for gfx950: greedy / temperature + top-k + top-p + min-p + seeded Gumbel-max.
//
// One 1024-thread workgroup per row (vocab up to ~256k), reading the row with 16-byte
// vectors; every pass after the first is served from L2 (a 128k-vocab bf16 row is 256 KB).
//  * greedy (temperature <= 0): one argmax pass (ties -> lowest index).
//  * top-k: exact k-th largest logit by 4-pass radix select on order-preserving uint32 keys
//    (8-bit digits, 256-bin LDS histogram; the digit is found by a 64-lane suffix scan).
//  * top-p: the same radix walk with *probability mass* per bin instead of counts, over the
//    top-k survivors: finds the smallest logit v* whose upper set holds >= p of the mass.
//  * min-p: x >= max + log(min_p) (in temperature-scaled logit space).
//  * sample: argmax over survivors of x/T + Gumbel(u), u = counter-based hash of
//    (seed, offset, token) -> bit-exact reproducible (see ops/reference.py philox_uniform);
//    u never reaches 1 and the draws next to 1 (the likely winners) are accurate (gumbel()).
// Ties at a threshold are kept (threshold semantics), which matches the reference mask.
#include "sampler_common.h"

using namespace pk;

namespace {

constexpr int kThreads = kRowThreads;

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t row_hash(uint32_t seed, uint32_t offset) {
  uint32_t h = seed * 0x9E3779B1u + 0x7F4A7C15u;
  h ^= offset + 0x85EBCA6Bu + (h << 6) + (h >> 2);
  return fmix32(h);
}

// Gumbel(0,1) draw -log(-log u) of token idx, u = (h + 0.5) * 2^-24 with h the hash's top 24 bits
// (ops/reference.py philox_uniform).  h + 0.5 is exact in fp32 only for h < 2^23; above that it
// rounds to even (by e = +-0.5), u' = fl(h + 0.5) * 2^-24 reaches 1.0f at h = 2^24 - 1 and the
// draw becomes +inf; next to 1, where the likely winners are, 1 - u' is off by 2^-25, as much as 1 - u itself.
// The rounding is known exactly, so it is put back to first order:
//   -log(u) = -log(u' + e * 2^-24) = -log(u') - e * 2^-24 / u' + O((2^-25 / u')^2),  1 / u' ~ 2 - u'
// (u' >= 1/2 wherever e != 0; the error of 2 - u' is (1 - u')^2, times a term that matters only
// where 1 - u' is tiny).  At u' = 1 this gives 2^-25 = 1 - u exactly.  __logf is accurate to
// 2e-7 *relative* on gfx950, also right below 1, so -log(u') loses nothing there.
__device__ __forceinline__ float gumbel(uint32_t rh, uint32_t idx) {
  const float hf = static_cast<float>(fmix32(rh ^ (idx * 0xC2B2AE35u)) >> 8);
  const float a = hf + 0.5f;
  const float e = 0.5f - (a - hf);  // exact: 0 below 2^23
  const float u = a * (1.0f / 16777216.0f);
  const float t = -__logf(u) - (e * (1.0f / 16777216.0f)) * (2.0f - u);
  return -__logf(t);
}

struct Smem {
  float fhist[256];
  uint32_t uhist[256];
  float red[16];
  uint32_t ured[16];
  int ired[16];
  uint32_t sel_digit;
  float sel_f;
};

// One row, T = the row's element type.  The caller's workgroup runs it for exactly one T (the
// choice is uniform per workgroup), so the bf16 / fp32 rows and the fp32 rows of an alternative
// buffer (pk_sample_alt) are the same code.
template <typename T>
__device__ __forceinline__ void sample_row(Smem& sm, float& above_f, uint32_t& above_u, int* __restrict__ out,
                                           const T* __restrict__ x, int row, int V,
                                           const float* __restrict__ temperature, const int* __restrict__ top_k,
                                           const float* __restrict__ top_p, const float* __restrict__ min_p,
                                           const int* __restrict__ seeds, const int* __restrict__ offsets) {
  const int nv = V / 8;
  const float temp = temperature ? temperature[row] : 0.f;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  // ---- pass 1: max (and argmax for greedy)
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int v = threadIdx.x; v < nv; v += kThreads) {
    float f[8];
    Row<T>::load8(x, v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (f[j] > best) {
        best = f[j];
        besti = 8 * v + j;
      }
  }
  block_argmax(best, besti, sm.red, sm.ired);  // (value desc, index asc)
  const float xmax = best;
  if (!(temp > 0.f)) {
    if (threadIdx.x == 0) out[row] = besti;
    return;
  }
  const float inv_t = 1.f / temp;
  const float m = xmax * inv_t;
  float thr = -INFINITY;  // survivors: x*inv_t >= thr

  // ---- top-k: radix select of the k-th largest scaled logit
  const int k = top_k ? top_k[row] : 0;
  if (k > 0 && k < V) {
    uint32_t prefix = 0, pmask = 0, need = static_cast<uint32_t>(k);
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 256; i += kThreads) sm.uhist[i] = 0;
      __syncthreads();
      for (int v = threadIdx.x; v < nv; v += kThreads) {
        float f[8];
        Row<T>::load8(x, v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t key = okey(f[j] * inv_t);
          if ((key & pmask) == prefix) atomicAdd(&sm.uhist[(key >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      select_digit<uint32_t>(sm.uhist, need, &sm.sel_digit, &above_u);
      prefix |= sm.sel_digit << shift;
      pmask |= 255u << shift;
      need -= above_u;
      __syncthreads();
    }
    thr = from_okey(prefix);
  }

  // ---- top-p over the top-k survivors: mass-weighted radix select
  const float p = top_p ? top_p[row] : 1.f;
  if (p > 0.f && p < 1.f) {
    float z = 0.f;
    for (int v = threadIdx.x; v < nv; v += kThreads) {
      float f[8];
      Row<T>::load8(x, v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = f[j] * inv_t;
        if (s >= thr) z += __expf(s - m);
      }
    }
    z = block_sum(z, sm.red);
    float need = p * z;
    uint32_t prefix = 0, pmask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 256; i += kThreads) sm.fhist[i] = 0.f;
      __syncthreads();
      for (int v = threadIdx.x; v < nv; v += kThreads) {
        float f[8];
        Row<T>::load8(x, v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float s = f[j] * inv_t;
          const uint32_t key = okey(s);
          if (s >= thr && (key & pmask) == prefix) atomicAdd(&sm.fhist[(key >> shift) & 255u], __expf(s - m));
        }
      }
      __syncthreads();
      select_digit<float>(sm.fhist, need, &sm.sel_digit, &above_f);
      prefix |= sm.sel_digit << shift;
      pmask |= 255u << shift;
      need -= above_f;
      __syncthreads();
    }
    thr = fmaxf(thr, from_okey(prefix));
  }

  // ---- min-p
  const float mp = min_p ? min_p[row] : 0.f;
  if (mp > 0.f) thr = fmaxf(thr, m + __logf(mp));
  thr = fminf(thr, m);  // the max token always survives

  // ---- Gumbel-max over survivors
  const uint32_t rh = row_hash(static_cast<uint32_t>(seeds ? seeds[row] : 0), static_cast<uint32_t>(offsets ? offsets[row] : 0));
  float bs = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = threadIdx.x; v < nv; v += kThreads) {
    float f[8];
    Row<T>::load8(x, v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = f[j] * inv_t;
      if (s >= thr) {
        const int idx = 8 * v + j;
        const float sc = s + gumbel(rh, static_cast<uint32_t>(idx));
        if (sc > bs || (sc == bs && idx < bi)) {
          bs = sc;
          bi = idx;
        }
      }
    }
  }
  block_argmax(bs, bi, sm.red, sm.ired);
  if (threadIdx.x == 0) out[row] = bi;
}

// alt_slots[row] in [0, n_alt): the row is read as fp32 from alt + alt_slots[row] * alt_stride
// (ops/penalties.py: the penalised copy of the row); every other row, and every row when
// alt_slots is null, is read from `logits` as before.
template <typename T>
__global__ void __launch_bounds__(kThreads) sample_kernel(int* __restrict__ out, const T* __restrict__ logits,
                                                          int64_t stride, int V, const float* __restrict__ temperature,
                                                          const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                          const float* __restrict__ min_p, const int* __restrict__ seeds,
                                                          const int* __restrict__ offsets, const float* __restrict__ alt,
                                                          int64_t alt_stride, const int* __restrict__ alt_slots,
                                                          int n_alt) {
  __shared__ Smem sm;
  __shared__ float above_f;
  __shared__ uint32_t above_u;
  const int row = blockIdx.x;
  const int as = alt_slots ? alt_slots[row] : -1;
  if (as >= 0 && as < n_alt)
    sample_row<float>(sm, above_f, above_u, out, alt + as * alt_stride, row, V, temperature, top_k, top_p, min_p, seeds,
                      offsets);
  else
    sample_row<T>(sm, above_f, above_u, out, logits + row * stride, row, V, temperature, top_k, top_p, min_p, seeds,
                  offsets);
}

int launch_sample(void* out, const void* logits, const void* temperature, const void* top_k, const void* top_p,
                  const void* min_p, const void* seeds, const void* offsets, int B, int V, int stride, int dtype,
                  const void* alt, int64_t alt_stride, const void* alt_slots, int n_alt, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V % 8 || stride % 8) return -1;
  if (alt_slots && (!alt || alt_stride % 8 || alt_stride < V || n_alt < 0)) return -1;
  if (dtype == 0) {
    sample_kernel<bf16_t><<<B, kThreads, 0, stream>>>(
        static_cast<int*>(out), static_cast<const bf16_t*>(logits), stride, V, static_cast<const float*>(temperature),
        static_cast<const int*>(top_k), static_cast<const float*>(top_p), static_cast<const float*>(min_p),
        static_cast<const int*>(seeds), static_cast<const int*>(offsets), static_cast<const float*>(alt), alt_stride,
        static_cast<const int*>(alt_slots), n_alt);
  } else {
    sample_kernel<float><<<B, kThreads, 0, stream>>>(
        static_cast<int*>(out), static_cast<const float*>(logits), stride, V, static_cast<const float*>(temperature),
        static_cast<const int*>(top_k), static_cast<const float*>(top_p), static_cast<const float*>(min_p),
        static_cast<const int*>(seeds), static_cast<const int*>(offsets), static_cast<const float*>(alt), alt_stride,
        static_cast<const int*>(alt_slots), n_alt);
  }
  return PK_CHECK_LAUNCH();
}

}  // namespace

// dtype: 0 = bf16 logits, 1 = fp32 logits.  Any of the parameter arrays may be null (defaults:
// temperature 0 -> greedy, top_k 0, top_p 1, min_p 0, seed 0, offset 0).
PK_EXPORT int pk_sample(void* out, const void* logits, const void* temperature, const void* top_k, const void* top_p,
                        const void* min_p, const void* seeds, const void* offsets, void* unused, int B, int V,
                        int stride, int dtype, hipStream_t stream) {
  return launch_sample(out, logits, temperature, top_k, top_p, min_p, seeds, offsets, B, V, stride, dtype, nullptr, 0,
                       nullptr, 0, stream);
}

// pk_sample with an alternative fp32 source per row: alt fp32 [n_alt, alt_stride], alt_slots int[B]
// (-1 or out of range: the row is read from `logits` exactly as pk_sample does).
PK_EXPORT int pk_sample_alt(void* out, const void* logits, const void* temperature, const void* top_k,
                            const void* top_p, const void* min_p, const void* seeds, const void* offsets, int B, int V,
                            int stride, int dtype, const void* alt, int64_t alt_stride, const void* alt_slots,
                            int n_alt, hipStream_t stream) {
  return launch_sample(out, logits, temperature, top_k, top_p, min_p, seeds, offsets, B, V, stride, dtype, alt,
                       alt_stride, alt_slots, n_alt, stream);
}
