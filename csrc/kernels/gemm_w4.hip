// Weight-only MXFP4 (OCP Microscaling: e2m1 elements, one e8m0 scale byte per 32 elements along K)
// projections.
//
//   pk_w4_gemm     the decode GEMM on block-packed nibbles and scale words: the W4 instantiations of
//                  the one decode tile (skinny_tile.h skinny_tile, WFormat<kWMxfp4>) -- a quarter of
//                  the weight bytes of the bf16 kernels (plus 1/16 of that in scales), the same bf16
//                  MFMA pipeline, the same three epilogues, no channel scale
//   pk_w4_widen    packed nibbles + scales -> row-major bf16 [N, K] scratch with the block scale
//                  applied (exact): the prefill path, followed by the library GEMM (ops/gemm_w4.py)
#include "skinny_tile.h"

using namespace pk;

namespace {

// Instantiated for what the unfused TP=1 decode chain and the general path launch: kBF16 / kPartial /
// kSiluMul on packed weights, no norm prologue, no in-launch hand-off, not grouped.
template <int MT, int MODE, bool NT, bool RS, int KR>
__global__ void __launch_bounds__(256, 2) w4_gemm_kernel(const GemmW4Args args) {
  __shared__ SkinnyLds<MT> lds;
  skinny_tile<MT, MODE, true, false, NT, RS, KR, 0, kWMxfp4>(args, blockIdx.x, 0, gridDim.x, lds, Flow{});
}

template <int MODE, bool NT, bool RS, int KR = 2>
int launch_w4(const GemmW4Args& a, hipStream_t stream) {
  const dim3 grid((a.N / (64 * KR)) * a.S * a.row_tiles);
  if (a.tile_rows == 128) {
    w4_gemm_kernel<8, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a);
    return PK_CHECK_LAUNCH();
  }
  switch ((min(a.M, 64) + 15) / 16) {
    case 1: w4_gemm_kernel<1, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    case 2: w4_gemm_kernel<2, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    case 3:
    case 4: w4_gemm_kernel<4, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    default: return -1;
  }
  return PK_CHECK_LAUNCH();
}

// the instantiation switch of the W4 kernels (tiling rules: skinny_tile.h skinny_tiling)
int dispatch_w4(const GemmW4Args& args, int mode, hipStream_t stream) {
  if (args.M <= 0) return 0;
  GemmW4Args a = args;
  const bool rs = a.row_scale != 0;
  if ((mode & ~(7 | 64 | 128)) || (mode & 7) > kSiluMul) return -1;
  if (a.W == nullptr || a.A == nullptr || a.w_xscale == nullptr) return -1;
  if (a.M > 512) return -1;  // (ops/gemm.py DECODE_MAX_M)
  SkinnyTiling tiling;
  if (!skinny_tiling(a, a.M, mode, tiling)) return -1;
  const bool nt = tiling.nt, half = tiling.half;
  const int m = mode & 7;
  if (m == kPartial ? a.partial == nullptr : (a.out == nullptr || a.S != 1)) return -1;
  if (half) {  // the split-K slab projections only
    if (m != kPartial || nt) return -1;
    return rs ? launch_w4<kPartial, false, true, 1>(a, stream) : launch_w4<kPartial, false, false, 1>(a, stream);
  }
  switch (m) {
    case kBF16:
      if (rs) return -1;
      return nt ? launch_w4<kBF16, true, false>(a, stream) : launch_w4<kBF16, false, false>(a, stream);
    case kPartial:
      return rs ? launch_w4<kPartial, false, true>(a, stream) : launch_w4<kPartial, false, false>(a, stream);
    default:  // kSiluMul
      if (a.N % 32) return -1;
      if (rs) return nt ? launch_w4<kSiluMul, true, true>(a, stream) : launch_w4<kSiluMul, false, true>(a, stream);
      return nt ? launch_w4<kSiluMul, true, false>(a, stream) : launch_w4<kSiluMul, false, false>(a, stream);
  }
}

// one thread per 16 packed bytes (a lane's load in the GEMM): four 8-element runs of one row, one
// MX block each
__global__ void __launch_bounds__(256) w4_widen_kernel(bf16_t* __restrict__ out, const uint8_t* __restrict__ wp,
                                                       const uint32_t* __restrict__ xs, int N, int K) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(N) * K / 32) return;
  const int lane = static_cast<int>(i & 63), r = lane & 15, g = lane >> 4;
  int64_t q = i >> 6;  // (n-block, k-step, tile)
  const uint32_t x = xs[q * 16 + r];
  const int tile = static_cast<int>(q & 7);
  q >>= 3;
  const int ksteps = K / 128;
  const int ks = static_cast<int>(q % ksteps), nb = static_cast<int>(q / ksteps);
  const u32x4 raw = *reinterpret_cast<const u32x4*>(wp + i * 16);
  bf16_t* o = out + static_cast<int64_t>(nb * 128 + tile * 16 + r) * K + ks * 128 + 8 * g;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    *reinterpret_cast<bf16x8_t*>(o + 32 * s) = mxfp4_widen8(raw[s], (x >> (8 * s)) & 0xffu);
}

}  // namespace

// mode 0: out bf16 [M, ldo] (S must be 1); 1: fp32 slabs [S, M, N] in partial; 2: SiLU-mul of
// interleaved gate/up rows -> out bf16 [M, N / 2] (S must be 1); bit 6: non-temporal weight loads;
// bit 7: 64-row n-blocks (mode 1 only).  W: pack_w4 nibbles of [N, K] (N K / 2 bytes); xscale: pack_w4
// scale words (N K / 32 bytes, every byte in [2, 252]).  nrm_parts non-null: the folded-norm row
// scale from [nrm_nparts, M] sums of squares (modes 1 and 2).
// Requires M <= 512, N % 128 == 0, K % (256 S) == 0, lda % 8 == 0.
PK_EXPORT int pk_w4_gemm(void* out, void* partial, const void* A, const void* W, const void* xscale, int M, int N,
                         int K, int lda, int ldo, int S, int mode, const void* nrm_parts, int nrm_nparts, float eps,
                         hipStream_t stream) {
  GemmW4Args a{};
  a.out = static_cast<bf16_t*>(out);
  a.partial = static_cast<float*>(partial);
  a.A = static_cast<const bf16_t*>(A);
  a.W = static_cast<const bf16_t*>(W);  // packed nibbles: the tile reads them as bytes
  a.w_xscale = static_cast<const uint32_t*>(xscale);
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldo = ldo; a.S = S;
  a.nrm_parts = static_cast<const float*>(nrm_parts);
  a.row_scale = nrm_parts != nullptr;
  a.nrm_nparts = nrm_nparts;
  a.eps = eps;
  return dispatch_w4(a, mode, stream);
}

// packed nibbles + scale words of [N, K] (pack_w4) -> row-major bf16 [N, K], block scales applied;
// N % 128 == 0, K % 128 == 0
PK_EXPORT int pk_w4_widen(void* out, const void* packed, const void* xscale, int N, int K, hipStream_t stream) {
  if (N <= 0 || K <= 0 || N % 128 || K % 128) return -1;
  const int64_t n = static_cast<int64_t>(N) * K / 32;
  w4_widen_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(
      static_cast<bf16_t*>(out), static_cast<const uint8_t*>(packed), static_cast<const uint32_t*>(xscale), N, K);
  return PK_CHECK_LAUNCH();
}
