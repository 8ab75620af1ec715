// FP8 (OCP e4m3fn) KV-cache elements for the gfx950 attention kernels and cache writers.
//
// A cache byte is e4m3_rne(clamp(x / scale, -448, 448)); attention uses scale * byte.  The cache
// keeps the ELEMENT offsets of the bf16 layout (common.h kcache_off / vcache_off), so a 32-token
// tile of one kv head is 4 KiB and an MFMA operand fragment 8 bytes per lane.  Readers widen
// e4m3 to bf16 (exact: 3 mantissa bits, exponents inside bf16's range) with v_cvt_pk_f32_fp8 +
// v_cvt_pk_bf16_f32 and feed the bf16 MFMA pipeline; the two per-layer scales are folded into
// the softmax scale (K) and the final 1 / l normalisation (V), both outside the key loop.
#pragma once
#include "common.h"

namespace pk {

typedef uint8_t fp8_t;  // raw e4m3fn bits

struct KvScale {
  float k = 1.f, v = 1.f;
};

template <typename CT>
constexpr bool kIsFp8 = sizeof(CT) == 1;

constexpr float kFp8Max = 448.f;

// a scale an entry point accepts: positive and finite
inline bool kv_scales_ok(float k_scale, float v_scale) {
  return k_scale > 0.f && v_scale > 0.f && k_scale < INFINITY && v_scale < INFINITY;
}

// The cache type argument of an entry point: kv_dtype 0 is bf16 (the scales are ignored), 1 is e4m3
// with scales that pass kv_scales_ok.  Calls f(element, scales...): a bf16_t and no scales, or an
// fp8_t and one KvScale -- the trailing pack the kernels take.  Anything else: -1, f is not called.
template <typename F>
int with_kv_type(int kv_dtype, float k_scale, float v_scale, F&& f) {
  if (kv_dtype == 0) return f(bf16_t{});
  if (kv_dtype == 1 && kv_scales_ok(k_scale, v_scale)) return f(fp8_t{}, KvScale{k_scale, v_scale});
  return -1;
}

// x / scale clamped to the finite range (+-inf and anything beyond +-448 store +-448; the clamp is
// explicit, the conversion's own overflow mode is never reached)
__device__ __forceinline__ float fp8_prep(float x, float scale) {
  return fminf(fmaxf(__fdiv_rn(x, scale), -kFp8Max), kFp8Max);
}

// two / four / eight clamped floats -> packed e4m3 bytes (round to nearest even, subnormals kept)
__device__ __forceinline__ uint32_t fp8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return static_cast<uint32_t>(w);
}

__device__ __forceinline__ uint2 fp8_pack8(const float* f) {
  uint2 r;
  r.x = fp8_pack4(f[0], f[1], f[2], f[3]);
  r.y = fp8_pack4(f[4], f[5], f[6], f[7]);
  return r;
}

__device__ __forceinline__ fp8_t fp8_from(float x) {
  return static_cast<fp8_t>(__builtin_amdgcn_cvt_pk_fp8_f32(x, 0.f, 0, false) & 0xff);
}

__device__ __forceinline__ float fp8_to_f(fp8_t b) {
  return __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(b), false)[0];
}

// the value a cache byte holds for x (quantise, then widen again), before the scale
__device__ __forceinline__ float fp8_round(float x, float scale) { return fp8_to_f(fp8_from(fp8_prep(x, scale))); }

// 8 e4m3 bytes -> 8 bf16 (exact)
__device__ __forceinline__ u32x4 fp8_widen8(uint2 raw) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw.x), false);
  const auto b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw.x), true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw.y), false);
  const auto d = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw.y), true);
  return u32x4{pack2(a[0], a[1]), pack2(b[0], b[1]), pack2(c[0], c[1]), pack2(d[0], d[1])};
}

}  // namespace pk
