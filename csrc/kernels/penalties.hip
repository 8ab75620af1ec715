// Sampling penalties and logit bias for gfx950: repetition / frequency / presence penalties and
// logit_bias applied to a *copy* of the logits row, from token history kept on the device.
//
// The raw logits are never written (pk_logprobs reads them after the sampler); a penalised row
// is written as fp32 to out[slot] and the sampler reads it from there (sampler.hip pk_sample_alt).
// State, one row per slot (a slot belongs to one penalised sequence, engine/model_runner.py):
//  * counts [n_slots, cstride] 16-bit words: bit 15 = the token is in the prompt, bits 0..14 =
//    occurrences among the generated tokens, saturating at 0x7fff;
//  * bias_ids / bias_vals [n_slots, kMaxBias] and bias_n [n_slots]: the logit_bias list;
//  * out [n_slots, ostride] fp32: the penalised row.
// Per element, in fp32 and in this order, one rounding per operation (no contraction):
//   seen (word != 0):  x = x > 0 ? x / r : x * r
//   c = count > 0:     x = x - f * c;  x = x - p
//   bias:              x = x + b
// -inf stays -inf.  Every kernel returns early for slot < 0 and ignores a slot >= n_slots or a
// token id outside [0, V).  Rows of one launch have distinct slots, so they never share a word;
// within one seed entry duplicates meet on the same word and are settled by global atomics on
// the containing 32-bit word (compare-and-swap: the neighbouring token's half is carried along).
#include "sampler_common.h"

using namespace pk;

namespace {

constexpr int kThreads = kRowThreads;
constexpr int kMaxBias = 300;
constexpr int kEntryWords = 6;  // slot, start, n_prompt, n_out, n_bias, clear

// ---- seed: one workgroup per entry
__global__ void __launch_bounds__(kThreads) seed_kernel(uint16_t* __restrict__ counts, int64_t cstride,
                                                        int* __restrict__ bias_ids, float* __restrict__ bias_vals,
                                                        int* __restrict__ bias_n, const int* __restrict__ entries,
                                                        const int* __restrict__ ids, int n_ids, int n_slots, int V) {
  const int* e = entries + blockIdx.x * kEntryWords;
  const int slot = e[0], start = e[1], clear = e[5];
  const int n_prompt = e[2], n_out = e[3], n_b = e[4];
  if (slot < 0 || slot >= n_slots || start < 0 || n_prompt < 0 || n_out < 0 || n_b < 0) return;
  // an entry that would read past the id stream is ignored as a whole
  if (static_cast<int64_t>(start) + n_prompt + n_out + 2 * static_cast<int64_t>(n_b) > n_ids) return;
  uint32_t* row32 = reinterpret_cast<uint32_t*>(counts + slot * cstride);  // cstride % 8 == 0: aligned
  if (clear) {
    u32x4* row = reinterpret_cast<u32x4*>(row32);
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int v = threadIdx.x; v < cstride / 8; v += kThreads) row[v] = z;
  }
  const int base = clear ? 0 : min(max(bias_n[slot], 0), kMaxBias);
  __syncthreads();  // the cleared row is visible to the workgroup; everybody has read bias_n
  const int* p = ids + start;
  for (int i = threadIdx.x; i < n_prompt; i += kThreads) {
    const int t = p[i];
    if (t >= 0 && t < V) atomicOr(&row32[t >> 1], 0x8000u << (16 * (t & 1)));
  }
  p += n_prompt;
  for (int i = threadIdx.x; i < n_out; i += kThreads) {
    const int t = p[i];
    if (t < 0 || t >= V) continue;
    const int sh = 16 * (t & 1);
    uint32_t old = row32[t >> 1];
    while (true) {
      const uint32_t h = (old >> sh) & 0xffffu;
      if ((h & 0x7fffu) == 0x7fffu) break;  // saturated
      const uint32_t want = (old & ~(0xffffu << sh)) | ((h + 1u) << sh);
      const uint32_t got = atomicCAS(&row32[t >> 1], old, want);
      if (got == old) break;
      old = got;
    }
  }
  p += n_out;
  for (int j = threadIdx.x; j < n_b; j += kThreads) {
    if (base + j < kMaxBias) {
      bias_ids[slot * kMaxBias + base + j] = p[j];
      bias_vals[slot * kMaxBias + base + j] = __int_as_float(p[n_b + j]);
    }
  }
  if (threadIdx.x == 0) bias_n[slot] = min(base + n_b, kMaxBias);
}

// ---- apply: one workgroup per batch row
// steps 1 and 2 on 8 logits and their 8 count words, one rounding per operation
__device__ __forceinline__ void penalise8(float* y, const u32x4& w, float r, float f, float pp) {
  if (!(w[0] | w[1] | w[2] | w[3])) return;  // most vectors of a 128k row hold no seen token
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t h = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    if (h) {
      float a = y[j];
      a = a > 0.f ? __fdiv_rn(a, r) : __fmul_rn(a, r);
      const uint32_t c = h & 0x7fffu;
      if (c) {
        a = __fsub_rn(a, __fmul_rn(f, static_cast<float>(c)));
        a = __fsub_rn(a, pp);
      }
      y[j] = a;
    }
  }
}

__device__ __forceinline__ void store8(float* o, int v, const float* y) {
  float4* q = reinterpret_cast<float4*>(o) + 2 * v;
  q[0] = make_float4(y[0], y[1], y[2], y[3]);
  q[1] = make_float4(y[4], y[5], y[6], y[7]);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) apply_kernel(float* __restrict__ out, int64_t ostride,
                                                         const T* __restrict__ logits, int64_t stride, int V,
                                                         const uint16_t* __restrict__ counts, int64_t cstride,
                                                         const int* __restrict__ slots, const float* __restrict__ rep,
                                                         const float* __restrict__ freq, const float* __restrict__ pres,
                                                         const int* __restrict__ bias_ids,
                                                         const float* __restrict__ bias_vals,
                                                         const int* __restrict__ bias_n, int n_slots) {
  const int row = blockIdx.x;
  const int slot = slots[row];
  if (slot < 0 || slot >= n_slots) return;  // not penalised: nothing read, nothing written
  const T* x = logits + row * stride;
  const u32x4* cw = reinterpret_cast<const u32x4*>(counts + slot * cstride);
  float* o = out + slot * ostride;
  const float r = rep[row], f = freq[row], pp = pres[row];
  const int nv = V / 8;
  // (two vectors in flight per thread measured no faster: 23.3 vs 22.4 us at B = 64, V = 128,256)
  for (int v = threadIdx.x; v < nv; v += kThreads) {
    float y[8];
    Row<T>::load8(x, v, y);
    penalise8(y, cw[v], r, f, pp);
    store8(o, v, y);
  }
  __syncthreads();  // the row is written (and visible to this workgroup) before biases are added
  const int nb = min(max(bias_n[slot], 0), kMaxBias);
  for (int j = threadIdx.x; j < nb; j += kThreads) {  // ids of one list are unique (validated by the host)
    const int t = bias_ids[slot * kMaxBias + j];
    if (t >= 0 && t < V) o[t] = __fadd_rn(o[t], bias_vals[slot * kMaxBias + j]);
  }
}

// ---- update: one thread per batch row
__global__ void __launch_bounds__(256) update_kernel(uint16_t* __restrict__ counts, int64_t cstride,
                                                     const int* __restrict__ slots, const int* __restrict__ tokens,
                                                     int B, int n_slots, int V) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= B) return;
  const int slot = slots[row];
  if (slot < 0 || slot >= n_slots) return;
  const int t = tokens[row];
  if (t < 0 || t >= V) return;
  uint16_t* w = counts + slot * cstride + t;
  const uint16_t h = *w;
  if ((h & 0x7fffu) != 0x7fffu) *w = static_cast<uint16_t>(h + 1u);  // bit 15 is untouched
}

}  // namespace

// entries: int[n_entries, 6] = (slot, start, n_prompt, n_out, n_bias, clear); ids: the int stream
// of n_ids words an entry indexes: n_prompt prompt ids from `start`, then n_out generated ids,
// then n_bias bias ids, then n_bias fp32 bit patterns.  clear = 1 zeroes the slot's count row and
// bias list first; clear = 0 appends to both.  Entries of one launch must name distinct slots.
PK_EXPORT int pk_penalty_seed(void* counts, int64_t cstride, void* bias_ids, void* bias_vals, void* bias_n,
                              const void* entries, int n_entries, const void* ids, int n_ids, int n_slots, int V,
                              hipStream_t stream) {
  if (n_entries <= 0) return 0;
  if (V <= 0 || cstride % 8 || cstride < V || n_slots <= 0 || n_ids < 0) return -1;
  seed_kernel<<<n_entries, kThreads, 0, stream>>>(static_cast<uint16_t*>(counts), cstride, static_cast<int*>(bias_ids),
                                                  static_cast<float*>(bias_vals), static_cast<int*>(bias_n),
                                                  static_cast<const int*>(entries), static_cast<const int*>(ids), n_ids,
                                                  n_slots, V);
  return PK_CHECK_LAUNCH();
}

// out fp32 [n_slots, ostride] <- penalised logits row of every batch row with slots[row] in
// [0, n_slots); rep / freq / pres fp32 [B] per batch row.  dtype: 0 = bf16 logits, 1 = fp32.
PK_EXPORT int pk_penalty_apply(void* out, int64_t ostride, const void* logits, int64_t stride, int dtype, int B, int V,
                               const void* counts, int64_t cstride, const void* slots, const void* rep,
                               const void* freq, const void* pres, const void* bias_ids, const void* bias_vals,
                               const void* bias_n, int n_slots, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || V % 8 || stride % 8 || stride < V || cstride % 8 || cstride < V || ostride % 8 || ostride < V ||
      n_slots <= 0)
    return -1;
  if (dtype == 0) {
    apply_kernel<bf16_t><<<B, kThreads, 0, stream>>>(
        static_cast<float*>(out), ostride, static_cast<const bf16_t*>(logits), stride, V,
        static_cast<const uint16_t*>(counts), cstride, static_cast<const int*>(slots), static_cast<const float*>(rep),
        static_cast<const float*>(freq), static_cast<const float*>(pres), static_cast<const int*>(bias_ids),
        static_cast<const float*>(bias_vals), static_cast<const int*>(bias_n), n_slots);
  } else if (dtype == 1) {
    apply_kernel<float><<<B, kThreads, 0, stream>>>(
        static_cast<float*>(out), ostride, static_cast<const float*>(logits), stride, V,
        static_cast<const uint16_t*>(counts), cstride, static_cast<const int*>(slots), static_cast<const float*>(rep),
        static_cast<const float*>(freq), static_cast<const float*>(pres), static_cast<const int*>(bias_ids),
        static_cast<const float*>(bias_vals), static_cast<const int*>(bias_n), n_slots);
  } else {
    return -1;
  }
  return PK_CHECK_LAUNCH();
}

// counts[slots[row]][tokens[row]] += 1 (saturating, prompt flag kept) for every batch row with a slot.
PK_EXPORT int pk_penalty_update(void* counts, int64_t cstride, const void* slots, const void* tokens, int B,
                                int n_slots, int V, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || cstride % 8 || cstride < V || n_slots <= 0) return -1;
  update_kernel<<<(B + 255) / 256, 256, 0, stream>>>(static_cast<uint16_t*>(counts), cstride,
                                                     static_cast<const int*>(slots), static_cast<const int*>(tokens), B,
                                                     n_slots, V);
  return PK_CHECK_LAUNCH();
}
