// The decode GEMM workgroup body for FP8 (OCP e4m3) weights with one fp32 scale per output channel:
// a sibling of skinny_tile (skinny_tile.h) that streams half the weight bytes.
//
//   y[m, n] = (sum_k x[m, k] * widen(byte[n, k])) * scale[n]      (fp32 products and sums)
//
// Activations stay bf16 and the MFMA is the bf16 one: a weight fragment is widened e4m3 -> bf16
// (exact, kv_fp8.h fp8_widen8) right before the MFMA that consumes it.  Only the weight pointer /
// load, that fragment, and a per-column scale of acc ahead of the RS row scale differ from
// skinny_tile; the A staging, the k-chunk rotation, the row tiles and the three epilogues are the
// same, so the fp32 slabs feed the same reducers.  Instantiated for what the unfused TP=1 decode
// chain and the general path launch: kBF16 / kPartial / kSiluMul on packed weights, no norm
// prologue, no in-launch hand-off, not grouped.
//
// Block-packed W8 (ops/gemm_w8.py pack_w8): per (128-row n-block, 128-deep k-step) the 16 KiB a
// workgroup consumes are contiguous, as 8 row tiles x 2 loads of 1 KiB in lane order; lane
// l = 16 g + r of load jj holds row r, bytes 0-7 = k 32 (2 jj) + 8 g .. + 7 and bytes 8-15 =
// k 32 (2 jj + 1) + 8 g .. + 7: the MFMA A fragments of k-blocks s = 2 jj and 2 jj + 1.
#pragma once
#include "kv_fp8.h"
#include "skinny_tile.h"

struct GemmW8Args {
  bf16_t* out;             // kBF16: [M, ldo]; kSiluMul: [M, ldo] of N / 2 columns
  float* partial;          // kPartial: fp32 slabs [S, M, N]
  const bf16_t* A;         // [M, lda]
  const fp8_t* W;          // block-packed e4m3 bytes of [N, K]
  const float* scale;      // [N]
  int M, N, K, lda, ldo, S;
  const float* nrm_parts;  // RS: per-row sums of squares [nrm_nparts, M]
  int nrm_nparts;
  float eps;
  int row_tiles;           // set by dispatch
  int tile_rows;           // set by dispatch: 64, or 128 for the MT = 8 variant
};

namespace {

constexpr int kW8Step = 8 * 2 * 1024;  // packed bytes of one (n-block, 128-deep k-step)

template <bool NT>
__device__ __forceinline__ u32x4 ldw8(const fp8_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return *reinterpret_cast<const u32x4*>(p);
}

template <int MT, int MODE, bool NT, bool RS = false, int KR = 2>
__device__ __forceinline__ void skinny_tile_w8(const GemmW8Args& args, const int bx_in, const int gdx,
                                               SkinnyLds<MT>& L) {
  static_assert(MODE == kBF16 || MODE == kPartial || MODE == kSiluMul, "W8: bf16 out, fp32 slabs or SiLU-mul");
  constexpr int kR = KR;
  constexpr int kKA = SkinnyLds<MT>::kKA;  // k per staged A tile
  constexpr int kPPR = kKA / 8;             // 16-byte pieces per A row
  auto& a_lds = L.a;
  auto& rinv_s = L.rinv;
  const int N = args.N, K = args.K, S = args.S;
  // row tiles: see skinny_tile (the workgroups of one W tile share one XCD's L2)
  int bx = bx_in, rt = 0;
  if (args.row_tiles > 1) {
    const int RT = args.row_tiles, T = gdx / RT;
    if ((T & 7) == 0) {
      const int q = bx >> 3;
      rt = q % RT;
      bx = (q / RT) * 8 + (bx & 7);
    } else {
      rt = bx % RT;
      bx /= RT;
    }
  }
  const int row0 = rt * 16 * MT;
  const int M = min(args.M - row0, 16 * MT);
  if (M <= 0) return;
  const bf16_t* __restrict__ A = args.A + static_cast<int64_t>(row0) * args.lda;
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int nb = bx / S, split = bx % S;
  const int kper = K / S;
  const int k0 = split * kper;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = nb * 64 * kR + w * 16 * kR;

  // RS: the row's sum-of-squares parts, requested before the weight stream (see skinny_tile)
  constexpr int kRsRows = MT > 4 ? 2 : 1;
  constexpr int kRsLoads = 16 / (kRsRows * kRsRows);
  float rs_p[RS ? kRsRows * kRsLoads : 1];
  if constexpr (RS) {
    const int np = min(args.nrm_nparts, 4 * kRsLoads), sub = tid & 3;
#pragma unroll
    for (int h = 0; h < kRsRows; ++h) {
      const int rr = min(64 * h + (tid >> 2), M - 1);
#pragma unroll
      for (int q = 0; q < kRsLoads; ++q)
        rs_p[h * kRsLoads + q] = args.nrm_parts[min(sub + 4 * q, np - 1) * args.M + row0 + rr];
    }
  }
  // the scales of this lane's 4 output columns per 16-column tile, consumed after the main loop
  float4 sc_n[kR];
#pragma unroll
  for (int t = 0; t < kR; ++t) sc_n[t] = ld4f(args.scale + n0 + 16 * t + 4 * g);

  const fp8_t* wp[kR];
#pragma unroll
  for (int t = 0; t < kR; ++t)
    wp[t] = args.W + static_cast<int64_t>(n0 >> 7) * 128 * K + (((n0 & 127) >> 4) + t) * 2 * 1024 + 16 * lane;

  // A staging: MT*16 rows x kKA cols of 16-byte pieces over 256 threads
  constexpr int kPieces = (16 * MT * kPPR + 255) / 256;
  u32x4 stage[kPieces];
  int aoff[kPieces];  // element offset of each staged piece in its k-chunk (rows <= 1024: 32 bits)
#pragma unroll
  for (int p = 0; p < kPieces; ++p)
    aoff[p] = min((tid + 256 * p) / kPPR, M - 1) * args.lda + ((tid + 256 * p) % kPPR) * 8;
  auto load_a = [&](int kc) {
#pragma unroll
    for (int p = 0; p < kPieces; ++p)
      stage[p] = *reinterpret_cast<const u32x4*>(A + kc + aoff[p]);
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int p = 0; p < kPieces; ++p) {
      const int idx = tid + 256 * p;
      *reinterpret_cast<u32x4*>(&a_lds[buf][idx / kPPR][(idx % kPPR) * 8]) = stage[p];
    }
  };

  f32x4 acc[kR][MT];
#pragma unroll
  for (int t = 0; t < kR; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one 128-deep k-step of weights: 2 loads of 16 bytes per 16-row tile (raw e4m3, widened at use)
  u32x4 wa[kR][2], wb[kR][2];
  auto load_w = [&](u32x4 (&dst)[kR][2], int k) {
#pragma unroll
    for (int t = 0; t < kR; ++t)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) dst[t][jj] = ldw8<NT>(wp[t] + static_cast<int64_t>(k >> 7) * kW8Step + jj * 1024);
  };
  auto mma_step = [&](const u32x4 (&wf)[kR][2], int buf, int kk) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8_t af[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        af[mt] = *reinterpret_cast<const bf16x8_t*>(&a_lds[buf][16 * mt + r][kk + 32 * s + 8 * g]);
#pragma unroll
      for (int t = 0; t < kR; ++t) {
        const u32x4 raw = wf[t][s >> 1];
        const uint2 half = (s & 1) ? uint2{raw[2], raw[3]} : uint2{raw[0], raw[1]};
        const bf16x8_t wv = __builtin_bit_cast(bf16x8_t, fp8_widen8(half));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, af[mt], acc[t][mt], 0, 0, 0);
      }
    }
  };

  // chunk order rotated per n-block; every load in the loop is unconditional (see skinny_tile)
  const int nchunks = kper / kKC;
  const int rot = (nb * 5) % nchunks;
  auto ck = [&](int c) { return k0 + ((min(c, nchunks - 1) + rot) % nchunks) * kKC; };
  if constexpr (MT > 4) {
    const int nsteps = 2 * nchunks;  // even
    const int rot2 = 2 * rot;
    auto ks = [&](int j) { return k0 + ((min(j, nsteps - 1) + rot2) % nsteps) * 128; };
    load_a(ks(0));
    load_w(wa, ks(0));
    load_w(wb, ks(1));
    store_a(0);
    int buf = 0;
    for (int j = 0; j < nsteps; j += 2) {
      load_a(ks(j + 1));
      __syncthreads();
      mma_step(wa, buf, 0);
      load_w(wa, ks(j + 2));
      store_a(buf ^ 1);
      buf ^= 1;
      load_a(ks(j + 2));
      __syncthreads();
      mma_step(wb, buf, 0);
      load_w(wb, ks(j + 3));
      store_a(buf ^ 1);
      buf ^= 1;
    }
  } else {
    load_a(ck(0));
    load_w(wa, ck(0));
    load_w(wb, ck(0) + 128);
    store_a(0);
    int buf = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int kn = ck(c + 1);
      load_a(kn);
      __syncthreads();  // chunk c visible in a_lds[buf]; every wave is done with a_lds[buf^1]
      mma_step(wa, buf, 0);
      load_w(wa, kn);
      mma_step(wb, buf, 128);
      load_w(wb, kn + 128);
      store_a(buf ^ 1);
      buf ^= 1;
    }
  }

  if constexpr (RS) {
    const int np = min(args.nrm_nparts, 4 * kRsLoads), sub = tid & 3;
#pragma unroll
    for (int h = 0; h < kRsRows; ++h) {
      float ss = 0.f;
#pragma unroll
      for (int q = 0; q < kRsLoads; ++q) ss += sub + 4 * q < np ? rs_p[h * kRsLoads + q] : 0.f;
      ss += __shfl_xor(ss, 1, 4);
      ss += __shfl_xor(ss, 2, 4);
      const int row = 64 * h + (tid >> 2);
      if (sub == 0 && row < M) rinv_s[row] = rsqrtf(ss / K + args.eps);
    }
    __syncthreads();
  }

  // acc[t][mt][i] = C[m = 16*mt + r][n = n0 + 16*t + 4*g + i]
  static_assert(MODE != kSiluMul || kR == 2, "SiLU: gate and up of the same columns in one wave");
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = 16 * mt + r;
    if (m >= M) continue;
#pragma unroll
    for (int t = 0; t < kR; ++t) {  // the channel scale, before the row scale
      acc[t][mt][0] *= sc_n[t].x;
      acc[t][mt][1] *= sc_n[t].y;
      acc[t][mt][2] *= sc_n[t].z;
      acc[t][mt][3] *= sc_n[t].w;
    }
    if constexpr (RS) {
      const float sc = rinv_s[m];
#pragma unroll
      for (int t = 0; t < kR; ++t) acc[t][mt] *= sc;
    }
    if constexpr (MODE == kPartial) {
      float* p = args.partial + (static_cast<int64_t>(split) * args.M + row0 + m) * N + n0 + 4 * g;
#pragma unroll
      for (int t = 0; t < kR; ++t) *reinterpret_cast<f32x4*>(p + 16 * t) = acc[t][mt];
    } else if constexpr (MODE == kBF16) {
      bf16_t* o = args.out + static_cast<int64_t>(row0 + m) * args.ldo + n0 + 4 * g;
#pragma unroll
      for (int t = 0; t < kR; ++t) {
        uint2 v;
        v.x = pack2(acc[t][mt][0], acc[t][mt][1]);
        v.y = pack2(acc[t][mt][2], acc[t][mt][3]);
        *reinterpret_cast<uint2*>(o + 16 * t) = v;
      }
    } else {  // kSiluMul: tile 0 = gate, tile 1 = up of the same 16 columns
      bf16_t* o = args.out + static_cast<int64_t>(row0 + m) * args.ldo + (n0 >> 1) + 4 * g;
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = rbf(silu(rbf(acc[0][mt][i]))) * rbf(acc[1][mt][i]);
      uint2 v;
      v.x = pack2(y[0], y[1]);
      v.y = pack2(y[2], y[3]);
      *reinterpret_cast<uint2*>(o) = v;
    }
  }
}

}  // namespace
