// Weight-only FP8 (OCP e4m3, one fp32 scale per output channel) projections.
//
//   pk_w8_gemm     the decode GEMM on block-packed e4m3 weights: the W8 instantiations of the one
//                  decode tile (skinny_tile.h skinny_tile, WFormat<kWFp8>) -- half the weight bytes
//                  of the bf16 kernels, the same bf16 MFMA pipeline, the same three epilogues
//   pk_w8_widen    packed bytes -> row-major bf16 [N, K] scratch (exact, no scale)   } the prefill
//   pk_col_scale   out[m, n] = bf16(float(out[m, n]) * scale[n]), in place           } path
//
// Prefill-sized M widens a projection into one shared scratch, runs the library GEMM on it and
// scales the columns (ops/gemm_w8.py).
#include "skinny_tile.h"

using namespace pk;

namespace {

// Instantiated for what the unfused TP=1 decode chain and the general path launch: kBF16 / kPartial /
// kSiluMul on packed weights, no norm prologue, no in-launch hand-off, not grouped.
template <int MT, int MODE, bool NT, bool RS, int KR>
__global__ void __launch_bounds__(256, 2) w8_gemm_kernel(const GemmW8Args args) {
  __shared__ SkinnyLds<MT> lds;
  skinny_tile<MT, MODE, true, false, NT, RS, KR, 0, kWFp8>(args, blockIdx.x, 0, gridDim.x, lds, Flow{});
}

template <int MODE, bool NT, bool RS, int KR = 2>
int launch_w8(const GemmW8Args& a, hipStream_t stream) {
  const dim3 grid((a.N / (64 * KR)) * a.S * a.row_tiles);
  if (a.tile_rows == 128) {
    w8_gemm_kernel<8, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a);
    return PK_CHECK_LAUNCH();
  }
  switch ((min(a.M, 64) + 15) / 16) {
    case 1: w8_gemm_kernel<1, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    case 2: w8_gemm_kernel<2, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    case 3:
    case 4: w8_gemm_kernel<4, MODE, NT, RS, KR><<<grid, 256, 0, stream>>>(a); break;
    default: return -1;
  }
  return PK_CHECK_LAUNCH();
}

// the instantiation switch of the W8 kernels (tiling rules: skinny_tile.h skinny_tiling)
int dispatch_w8(const GemmW8Args& args, int mode, hipStream_t stream) {
  if (args.M <= 0) return 0;
  GemmW8Args a = args;
  const bool rs = a.row_scale != 0;
  if ((mode & ~(7 | 64 | 128)) || (mode & 7) > kSiluMul) return -1;
  if (a.W == nullptr || a.A == nullptr || a.w_scale == nullptr) return -1;
  SkinnyTiling tiling;
  if (!skinny_tiling(a, a.M, mode, tiling)) return -1;
  const bool nt = tiling.nt, half = tiling.half;
  const int m = mode & 7;
  if (m == kPartial ? a.partial == nullptr : (a.out == nullptr || a.S != 1)) return -1;
  if (half) {  // the split-K slab projections only
    if (m != kPartial || nt) return -1;
    return rs ? launch_w8<kPartial, false, true, 1>(a, stream) : launch_w8<kPartial, false, false, 1>(a, stream);
  }
  switch (m) {
    case kBF16:
      if (rs) return -1;
      return nt ? launch_w8<kBF16, true, false>(a, stream) : launch_w8<kBF16, false, false>(a, stream);
    case kPartial:
      return rs ? launch_w8<kPartial, false, true>(a, stream) : launch_w8<kPartial, false, false>(a, stream);
    default:  // kSiluMul
      if (a.N % 32) return -1;
      if (rs) return nt ? launch_w8<kSiluMul, true, true>(a, stream) : launch_w8<kSiluMul, false, true>(a, stream);
      return nt ? launch_w8<kSiluMul, true, false>(a, stream) : launch_w8<kSiluMul, false, false>(a, stream);
  }
}

// one thread per 16 packed bytes (a lane's load in the GEMM): two 8-element runs of one row
__global__ void __launch_bounds__(256) w8_widen_kernel(bf16_t* __restrict__ out, const fp8_t* __restrict__ wp, int N,
                                                       int K) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(N) * K / 16) return;
  const int lane = static_cast<int>(i & 63), r = lane & 15, g = lane >> 4;
  int64_t q = i >> 6;
  const int jj = static_cast<int>(q & 1);
  q >>= 1;
  const int tile = static_cast<int>(q & 7);
  q >>= 3;
  const int ksteps = K / 128;
  const int ks = static_cast<int>(q % ksteps), nb = static_cast<int>(q / ksteps);
  const u32x4 raw = *reinterpret_cast<const u32x4*>(wp + i * 16);
  bf16_t* o = out + static_cast<int64_t>(nb * 128 + tile * 16 + r) * K + ks * 128 + 64 * jj + 8 * g;
  *reinterpret_cast<u32x4*>(o) = fp8_widen8(uint2{raw[0], raw[1]});
  *reinterpret_cast<u32x4*>(o + 32) = fp8_widen8(uint2{raw[2], raw[3]});
}

// one thread per 8 columns; rows in a grid-stride loop over blockIdx.y
__global__ void __launch_bounds__(256) col_scale_kernel(bf16_t* __restrict__ out, const float* __restrict__ scale,
                                                        int M, int N, int ldo) {
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c >= N) return;
  const float4 s0 = ld4f(scale + c), s1 = ld4f(scale + c + 4);
  const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    bf16_t* p = out + static_cast<int64_t>(m) * ldo + c;
    float v[8];
    unpack8(*reinterpret_cast<const u32x4*>(p), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= sv[j];
    *reinterpret_cast<u32x4*>(p) = pack8(v);
  }
}

}  // namespace

// mode 0: out bf16 [M, ldo] (S must be 1); 1: fp32 slabs [S, M, N] in partial; 2: SiLU-mul of
// interleaved gate/up rows -> out bf16 [M, N / 2] (S must be 1); bit 6: non-temporal weight loads;
// bit 7: 64-row n-blocks (mode 1 only).  W: pack_w8 bytes of [N, K]; scale: fp32 [N].  nrm_parts
// non-null: the folded-norm row scale from [nrm_nparts, M] sums of squares (modes 1 and 2).
// Requires M <= 1024, N % 128 == 0, K % (256 S) == 0, lda % 8 == 0.
PK_EXPORT int pk_w8_gemm(void* out, void* partial, const void* A, const void* W, const void* scale, int M, int N,
                         int K, int lda, int ldo, int S, int mode, const void* nrm_parts, int nrm_nparts, float eps,
                         hipStream_t stream) {
  GemmW8Args a{};
  a.out = static_cast<bf16_t*>(out);
  a.partial = static_cast<float*>(partial);
  a.A = static_cast<const bf16_t*>(A);
  a.W = static_cast<const bf16_t*>(W);  // packed e4m3 bytes: the tile reads them as fp8_t
  a.w_scale = static_cast<const float*>(scale);
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldo = ldo; a.S = S;
  a.nrm_parts = static_cast<const float*>(nrm_parts);
  a.row_scale = nrm_parts != nullptr;
  a.nrm_nparts = nrm_nparts;
  a.eps = eps;
  return dispatch_w8(a, mode, stream);
}

// packed e4m3 bytes of [N, K] (pack_w8) -> row-major bf16 [N, K]; N % 128 == 0, K % 128 == 0
PK_EXPORT int pk_w8_widen(void* out, const void* packed, int N, int K, hipStream_t stream) {
  if (N <= 0 || K <= 0 || N % 128 || K % 128) return -1;
  const int64_t n = static_cast<int64_t>(N) * K / 16;
  w8_widen_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(static_cast<bf16_t*>(out),
                                                                             static_cast<const fp8_t*>(packed), N, K);
  return PK_CHECK_LAUNCH();
}

// out [M, ldo] bf16, in place: column n times scale[n]; N % 8 == 0, ldo % 8 == 0
PK_EXPORT int pk_col_scale(void* out, const void* scale, int M, int N, int ldo, hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 8 || ldo % 8 || ldo < N) return -1;
  const dim3 grid((N / 8 + 255) / 256, M < 8192 ? M : 8192);
  col_scale_kernel<<<grid, 256, 0, stream>>>(static_cast<bf16_t*>(out), static_cast<const float*>(scale), M, N, ldo);
  return PK_CHECK_LAUNCH();
}
