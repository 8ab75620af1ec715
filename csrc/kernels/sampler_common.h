// Helpers shared by the row kernels that walk one logits row per 1024-thread workgroup
// (sampler.hip: token sampling, logprobs.hip: log-probabilities of the sampled token and top-n).
#pragma once
#include "common.h"

namespace pk {

constexpr int kRowThreads = 1024;

// Order-preserving float -> uint32 key (larger float <=> larger key) and its inverse.
__device__ __forceinline__ uint32_t okey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_okey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Row<T>::load8: the v-th 8-element vector of a row as fp32 (16-byte loads).
template <typename T>
struct Row;

template <>
struct Row<bf16_t> {
  static __device__ __forceinline__ void load8(const bf16_t* p, int v, float* out) {
    unpack8(reinterpret_cast<const u32x4*>(p)[v], out);
  }
  static __device__ __forceinline__ float load1(const bf16_t* p, int i) { return bf2f(p[i]); }
};

template <>
struct Row<float> {
  static __device__ __forceinline__ void load8(const float* p, int v, float* out) {
    const float4* q = reinterpret_cast<const float4*>(p) + 2 * v;
    float4 a = q[0], b = q[1];
    out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
    out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
  }
  static __device__ __forceinline__ float load1(const float* p, int i) { return p[i]; }
};

// Wave 0 finds the digit d (scanning 255 -> 0) where the running total first reaches `need`;
// returns (d, total of bins above d).  Other waves wait at the barrier.
template <typename V>
__device__ __forceinline__ void select_digit(const V* hist, V need, uint32_t* out_digit, V* out_above) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    // lane handles bins 255-4*lane .. 252-4*lane (descending)
    V b[4];
    V s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = hist[255 - 4 * lane - j];
      s += b[j];
    }
    // inclusive prefix over lanes (descending bins)
    V incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      V t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const V excl = incl - s;
    const bool hit = excl < need && incl >= need;
    const unsigned long long mask = __ballot(hit);
    const int src = mask ? __ffsll(static_cast<long long>(mask)) - 1 : 63;
    if (lane == src) {
      V acc = excl;
      int d = 252 - 4 * lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (acc + b[j] >= need) {
          d = 255 - 4 * lane - j;
          break;
        }
        acc += b[j];
      }
      *out_digit = static_cast<uint32_t>(d);
      *out_above = acc;
    }
  }
  __syncthreads();
}

// Block arg-max in the order (value descending, index ascending) for a kRowThreads workgroup:
// every thread passes its own candidate and gets the winner back.  `red` / `ired` need 16
// words of LDS each; they may be reused as soon as the call returns.
__device__ __forceinline__ void block_argmax(float& best, int& besti, float* red, int* ired) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ov > best || (ov == best && oi < besti)) {
      best = ov;
      besti = oi;
    }
  }
  __syncthreads();  // earlier readers of red / ired are done
  if (lane == 0) {
    red[wid] = best;
    ired[wid] = besti;
  }
  __syncthreads();
  float b = lane < kRowThreads / 64 ? red[lane] : -INFINITY;
  int bi = lane < kRowThreads / 64 ? ired[lane] : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(b, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > b || (ov == b && oi < bi)) {
      b = ov;
      bi = oi;
    }
  }
  best = b;
  besti = bi;
  __syncthreads();
}

}  // namespace pk
