// Per-token log-probabilities for gfx950: logprob of the sampled token and the top-n list.
//
// Taken from the *raw* logits row (before temperature / top-k / top-p / min-p).  One
// 1024-thread workgroup per row, 16-byte loads like the sampler (sampler.hip); passes after the
// first are served from L2.
//  * n_top[row] < 0: the workgroup returns before touching the logits and writes nothing.
//  * lse = max + log(sum exp(x - max)) in fp32 (two passes); the sampled token gets x[t] - lse.
//  * top-n (n <= kNMax) in the total order (value descending, index ascending): 4-pass radix
//    select of the n-th largest value on order-preserving keys (8-bit digits, as the sampler's
//    top-k), over the elements that reach the n-th largest per-thread maximum only.  The
//    elements >= that value are gathered into LDS and rank-sorted there, which settles ties.
//    Only when more than 128 would be gathered (a row full of ties) the same radix walk over
//    the inverted index first picks the lowest ids among the ties: the n-th element of the
//    total order is unique, so exactly n elements compare >= it.
//  * a row whose maximum is -inf reports -inf for every logprob (never NaN).
// Output: 41 32-bit words per row, [logprob | 20 ids | 20 logprobs]; slots n..19 hold -1 / -inf.
//
// The same body, instantiated with kPrompt, scores a row against a *given* target (prompt
// logprobs: the target is the next prompt token) and also reports the target's 1-based rank in
// the total order, 1 + #{j : x_j > x_t, or x_j == x_t and j < t}.  The rank is counted in pass 2,
// from the loads the sum of exponentials already makes (a compare on the keys and the index, one
// extra integer block sum), so a row that asks for no list is still read exactly twice.
//  * targets[row] < 0 or n_top[row] < 0: nothing read, nothing written.
//  * targets[row] >= V: logprob -inf, rank 0, the list as usual.
//  * a row whose maximum is -inf: logprob -inf, the rank by the same formula.
// Output: 42 words per row, [logprob | rank i32 | 20 ids | 20 logprobs].
#include "sampler_common.h"

using namespace pk;

namespace {

constexpr int kThreads = kRowThreads;
constexpr int kNMax = 20;
template <bool kPrompt>
constexpr int kHead = kPrompt ? 2 : 1;  // words before the list: logprob (| rank)
constexpr int kCand = 128;  // candidates the final rank-sort takes (LDS)

struct Smem {
  uint32_t uhist[256];
  float red[16];
  int ired[16];
  uint32_t sel_digit;
  uint32_t above;
  uint32_t ncand;
  uint32_t cand_key[kCand];
  uint32_t cand_idx[kCand];
};

// -0.0 and +0.0 compare equal, so they share a key (ties go by index)
__device__ __forceinline__ uint32_t vkey(float f) { return okey(f == 0.f ? 0.f : f); }

__device__ __forceinline__ int block_sum_int(int v, int* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) red[wid] = v;
  __syncthreads();
  int t = lane < kThreads / 64 ? red[lane] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  return t;
}

// kPrompt = false: `tokens` are the sampled ids (pk_logprobs); true: the targets (pk_prompt_logprobs).
template <typename T, bool kPrompt>
__global__ void __launch_bounds__(kThreads) logprobs_kernel(uint32_t* __restrict__ out, const T* __restrict__ logits,
                                                            int64_t stride, int V, const int* __restrict__ tokens,
                                                            const int* __restrict__ n_top) {
  const int row = blockIdx.x;
  int n = n_top[row];
  if (n < 0) return;  // not requested: nothing read, nothing written
  int target = 0;
  if constexpr (kPrompt) {
    target = tokens[row];
    if (target < 0) return;  // a row without a target (decode row, last prompt row, entry on record)
  }
  constexpr int kH = kHead<kPrompt>;
  __shared__ Smem sm;
  n = min(min(n, kNMax), V);
  const T* x = logits + row * stride;
  const int nv = V / 8;
  uint32_t* o = out + static_cast<int64_t>(row) * (kH + 2 * kNMax);

  // ---- pass 1: max
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
  const uint32_t mykey = vkey(best);  // this thread's own maximum (-inf: it holds no element)
  block_argmax(best, besti, sm.red, sm.ired);
  const float xmax = best;
  const bool dead = !(xmax > -INFINITY);  // every entry is -inf

  // ---- pass 2: sum exp(x - max); with kPrompt also the elements ahead of the target in the
  // total order (a dead row still walks: its rank follows the same formula, its z is unused)
  float z = 0.f;
  int ahead = 0;
  if constexpr (kPrompt) {
    const bool in = target < V;
    const uint32_t tkey = in ? vkey(Row<T>::load1(x, target)) : 0u;
    for (int v = threadIdx.x; v < nv; v += kThreads) {
      float f[8];
      Row<T>::load8(x, v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        z += __expf(f[j] - xmax);
        const uint32_t key = vkey(f[j]);
        ahead += (in && (key > tkey || (key == tkey && 8 * v + j < target))) ? 1 : 0;
      }
    }
    ahead = block_sum_int(ahead, sm.ired);
  } else if (!dead) {
    for (int v = threadIdx.x; v < nv; v += kThreads) {
      float f[8];
      Row<T>::load8(x, v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) z += __expf(f[j] - xmax);
    }
  }
  z = block_sum(z, sm.red);
  const float lse = dead ? -INFINITY : xmax + __logf(z);

  if (threadIdx.x == 0) {
    const int t = kPrompt ? target : tokens[row];
    float lp = -INFINITY;
    if (!dead && t >= 0 && t < V) lp = Row<T>::load1(x, t) - lse;
    o[0] = __float_as_uint(lp);
    if constexpr (kPrompt) o[1] = static_cast<uint32_t>(target < V ? ahead + 1 : 0);
  }
  if (n == 0) {
    if (threadIdx.x < kNMax) {
      o[kH + threadIdx.x] = 0xffffffffu;
      o[kH + kNMax + threadIdx.x] = __float_as_uint(-INFINITY);
    }
    return;
  }

  // ---- a lower bound of the n-th largest value: the n-th largest of the 1024 per-thread maxima
  // (n distinct elements are >= it).  The passes below histogram only elements >= the bound --
  // a few dozen of a 128k row unless the row is full of ties -- so they are plain reads of the
  // row, without an LDS atomic per element.
  uint32_t lo = 0;
  {
    uint32_t pf = 0, pm = 0, nd = static_cast<uint32_t>(n);
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 256; i += kThreads) sm.uhist[i] = 0;
      __syncthreads();
      if ((mykey & pm) == pf) atomicAdd(&sm.uhist[(mykey >> shift) & 255u], 1u);
      __syncthreads();
      select_digit<uint32_t>(sm.uhist, nd, &sm.sel_digit, &sm.above);
      pf |= sm.sel_digit << shift;
      pm |= 255u << shift;
      nd -= sm.above;
      __syncthreads();
    }
    lo = pf;
  }

  // ---- the n-th largest value: radix select over the value keys
  uint32_t prefix = 0, pmask = 0, need = static_cast<uint32_t>(n), ties = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += kThreads) sm.uhist[i] = 0;
    __syncthreads();
    for (int v = threadIdx.x; v < nv; v += kThreads) {
      float f[8];
      Row<T>::load8(x, v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t key = vkey(f[j]);
        if (key >= lo && (key & pmask) == prefix) atomicAdd(&sm.uhist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    select_digit<uint32_t>(sm.uhist, need, &sm.sel_digit, &sm.above);
    prefix |= sm.sel_digit << shift;
    pmask |= 255u << shift;
    need -= sm.above;
    ties = sm.uhist[sm.sel_digit];
    __syncthreads();
  }
  // `prefix` is the key of the n-th value v*; `need` of the `ties` elements equal to v* belong
  // to the top n: those with the lowest ids, i.e. the largest inverted ids.  n - need elements are
  // above v*: when they and all the ties fit the candidate pool (bf16 logits tie at the n-th
  // value more often than not, a handful at a time) the rank-sort below settles the ties and
  // iprefix stays 0; a row with more ties walks the ids first so that exactly n are gathered.
  uint32_t iprefix = 0;
  if (static_cast<uint32_t>(n) - need + ties > static_cast<uint32_t>(kCand)) {
    uint32_t imask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if ((static_cast<uint32_t>(V - 1) >> shift) == 0 && shift > 0) {
        // every id has digit 0 here, every inverted id 255: nothing to select
        iprefix |= 255u << shift;
        imask |= 255u << shift;
        continue;
      }
      for (int i = threadIdx.x; i < 256; i += kThreads) sm.uhist[i] = 0;
      __syncthreads();
      for (int v = threadIdx.x; v < nv; v += kThreads) {
        float f[8];
        Row<T>::load8(x, v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t ik = ~static_cast<uint32_t>(8 * v + j);
          if (vkey(f[j]) == prefix && (ik & imask) == iprefix) atomicAdd(&sm.uhist[(ik >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      select_digit<uint32_t>(sm.uhist, need, &sm.sel_digit, &sm.above);
      iprefix |= sm.sel_digit << shift;
      imask |= 255u << shift;
      need -= sm.above;
      __syncthreads();
    }
  }

  // ---- gather the elements >= (v*, id*) (n of them, or every tie too) and rank-sort them
  if (threadIdx.x == 0) sm.ncand = 0;
  __syncthreads();
  for (int v = threadIdx.x; v < nv; v += kThreads) {
    float f[8];
    Row<T>::load8(x, v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t key = vkey(f[j]);
      const uint32_t ik = ~static_cast<uint32_t>(8 * v + j);
      if (key > prefix || (key == prefix && ik >= iprefix)) {
        const uint32_t slot = atomicAdd(&sm.ncand, 1u);
        if (slot < static_cast<uint32_t>(kCand)) {
          sm.cand_key[slot] = key;
          sm.cand_idx[slot] = static_cast<uint32_t>(8 * v + j);
        }
      }
    }
  }
  __syncthreads();
  const int nc = static_cast<int>(min(sm.ncand, static_cast<uint32_t>(kCand)));
  if (static_cast<int>(threadIdx.x) < nc) {
    const uint32_t key = sm.cand_key[threadIdx.x], idx = sm.cand_idx[threadIdx.x];
    int rank = 0;
    for (int c = 0; c < nc; ++c) {
      const uint32_t ck = sm.cand_key[c], ci = sm.cand_idx[c];
      rank += (ck > key || (ck == key && ci < idx)) ? 1 : 0;
    }
    if (rank < n) {
      o[kH + rank] = idx;
      o[kH + kNMax + rank] = __float_as_uint(dead ? -INFINITY : from_okey(key) - lse);
    }
  }
  if (static_cast<int>(threadIdx.x) >= min(n, nc) && threadIdx.x < kNMax) {
    o[kH + threadIdx.x] = 0xffffffffu;
    o[kH + kNMax + threadIdx.x] = __float_as_uint(-INFINITY);
  }
}

}  // namespace

// out: [B, 41] 32-bit words, row = [logprob f32 | 20 ids i32 | 20 logprobs f32].  tokens: the
// sampled ids int[B]; n_top int[B]: -1 = row not requested (untouched), 0..20 = length of the
// top list.  dtype: 0 = bf16 logits, 1 = fp32 logits.
PK_EXPORT int pk_logprobs(void* out, const void* logits, const void* tokens, const void* n_top, int B, int V,
                          int stride, int dtype, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || V % 8 || stride % 8 || stride < V) return -1;
  if (dtype == 0) {
    logprobs_kernel<bf16_t, false><<<B, kThreads, 0, stream>>>(static_cast<uint32_t*>(out),
                                                               static_cast<const bf16_t*>(logits),
                                                        stride, V,
                                                               static_cast<const int*>(tokens),
                                                               static_cast<const int*>(n_top));
  } else if (dtype == 1) {
    logprobs_kernel<float, false><<<B, kThreads, 0, stream>>>(static_cast<uint32_t*>(out),
                                                              static_cast<const float*>(logits),
                                                       stride, V,
                                                              static_cast<const int*>(tokens),
                                                              static_cast<const int*>(n_top));
  } else {
    return -1;
  }
  return PK_CHECK_LAUNCH();
}

// out: [R, 42] 32-bit words, row = [logprob f32 | rank i32 | 20 ids i32 | 20 logprobs f32] of
// targets[r] under logits row r.  targets int[R]: the id to score, < 0 = row not asked
// (untouched); n_top int[R]: -1 = not asked, 0..20 = length of the top list.  Never captured.
PK_EXPORT int pk_prompt_logprobs(void* out, const void* logits, const void* targets, const void* n_top, int R, int V,
                                 int stride, int dtype, hipStream_t stream) {
  if (V <= 0 || V % 8 || stride % 8 || stride < V || (dtype != 0 && dtype != 1)) return -1;
  if (R <= 0) return 0;
  if (dtype == 0) {
    logprobs_kernel<bf16_t, true><<<R, kThreads, 0, stream>>>(static_cast<uint32_t*>(out),
                                                              static_cast<const bf16_t*>(logits), stride, V,
                                                              static_cast<const int*>(targets),
                                                              static_cast<const int*>(n_top));
  } else {
    logprobs_kernel<float, true><<<R, kThreads, 0, stream>>>(static_cast<uint32_t*>(out),
                                                             static_cast<const float*>(logits), stride, V,
                                                             static_cast<const int*>(targets),
                                                             static_cast<const int*>(n_top));
  }
  return PK_CHECK_LAUNCH();
}
