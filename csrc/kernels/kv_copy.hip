// KV block copy for the token-granular fork of a prompt (parallel sampling, n > 1): the one partial
// block of the forked prompt is copied from the source sequence's block to the fresh private block of
// every forked choice, in K and V of every layer, by ONE launch (2 x layers tensor copies otherwise:
// 64 for an 8B model).  The caches are `2 x layers` separate allocations, so the kernel reads their
// base pointers from a device table built once when the caches are allocated; a block is a
// contiguous run of `block_bytes` at `id * block_bytes` in both the K and the V layout, so the copy
// works on bytes and serves bf16 and FP8 caches alike.  The (src, dst) pairs travel by value in the
// launch arguments: no staging copy, nothing to keep alive after the call returns.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kMaxPairs = 32;
constexpr int kThreads = 256;
constexpr int kMaxSlices = 16;  // workgroups per (pair, tensor)

struct KvCopyPairs {
  int src[kMaxPairs];
  int dst[kMaxPairs];
};

// grid (slices, tensors, pairs): workgroup x copies 16-byte words x*256 + tid, += slices*256 of one
// block of one tensor
__global__ void __launch_bounds__(kThreads) kv_copy_blocks_kernel(char* const* __restrict__ tensors, int64_t block_bytes,
                                                                  KvCopyPairs pairs) {
  char* base = tensors[blockIdx.y];
  const pk::u32x4* src = reinterpret_cast<const pk::u32x4*>(base + pairs.src[blockIdx.z] * block_bytes);
  pk::u32x4* dst = reinterpret_cast<pk::u32x4*>(base + pairs.dst[blockIdx.z] * block_bytes);
  const int64_t n16 = block_bytes / 16;
  for (int64_t i = blockIdx.x * kThreads + threadIdx.x; i < n16; i += static_cast<int64_t>(gridDim.x) * kThreads)
    dst[i] = src[i];
}

}  // namespace

// tensors: device table of n_tensors cache base pointers, each cache num_blocks x block_bytes;
// pairs: HOST array of n_pairs (src, dst) block ids.  -1 (nothing launched) for what could read or
// write outside a cache or make the result depend on the order of the copies.
PK_EXPORT int pk_kv_copy_blocks(const void* tensors, int n_tensors, long long block_bytes, int num_blocks,
                                const int* pairs, int n_pairs, hipStream_t stream) {
  if (n_pairs < 0 || n_pairs > kMaxPairs || n_tensors < 0 || n_tensors > 65535) return -1;
  if (block_bytes <= 0 || block_bytes % 16 || num_blocks <= 0) return -1;
  KvCopyPairs p = {};
  for (int i = 0; i < n_pairs; ++i) {
    const int s = pairs[2 * i], d = pairs[2 * i + 1];
    if (s < 0 || s >= num_blocks || d < 0 || d >= num_blocks || s == d) return -1;
    p.src[i] = s;
    p.dst[i] = d;
  }
  for (int i = 0; i < n_pairs; ++i)
    for (int j = 0; j < n_pairs; ++j)
      if ((i != j && p.dst[i] == p.dst[j]) || p.dst[i] == p.src[j]) return -1;
  if (n_pairs == 0 || n_tensors == 0) return 0;
  const int64_t n16 = block_bytes / 16;
  const int slices = static_cast<int>(std::min<int64_t>((n16 + kThreads - 1) / kThreads, kMaxSlices));
  kv_copy_blocks_kernel<<<dim3(slices, n_tensors, n_pairs), kThreads, 0, stream>>>(
      static_cast<char* const*>(const_cast<void*>(tensors)), block_bytes, p);
  return PK_CHECK_LAUNCH();
}
