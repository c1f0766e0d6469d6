// rua_seg.h — what the kernels of the per-sequence operators (rua_softmax.hip, rua_scan.hip, rua_argreduce.hip,
// rua_linear_scan.hip, rua_pool.hip, rua_norm.hip) share: the element types, the clamped sequence length, the padding
// test, narrow-row accesses and the exp / log / inf / nan / shuffle one-liners.  Their host side — checks, cut plan,
// lanes geometry — is rua_seg_plan.h.
#pragma once
#include "rua_dev.h"
#include "rua_seg_plan.h"

namespace rua {

static_assert(SEG_WAVES_PER_BLOCK == RUA_WAVES_PER_BLOCK, "the lanes geometry of rua_seg_plan.h counts waves per workgroup");

// ---------------------------------------------------------------- element types
struct sm_f32 {
  using raw = float; using acc = float;
  static __device__ __forceinline__ acc up(raw v) { return v; }
  static __device__ __forceinline__ raw down(acc v) { return v; }
  static const char* name() { return "f32"; }
};
struct sm_f64 {
  using raw = double; using acc = double;
  static __device__ __forceinline__ acc up(raw v) { return v; }
  static __device__ __forceinline__ raw down(acc v) { return v; }
  static const char* name() { return "f64"; }
};
struct sm_bf16 {
  using raw = uint16_t; using acc = float;
  static __device__ __forceinline__ acc up(raw v) { return __uint_as_float((uint32_t)v << 16); }
  static __device__ __forceinline__ raw down(acc f) {           // round to nearest even
    uint32_t u = __float_as_uint(f);
    if (f != f) return (raw)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (raw)(u >> 16);
  }
  static const char* name() { return "bf16"; }
};
struct sm_f16 {
  using raw = _Float16; using acc = float;
  static __device__ __forceinline__ acc up(raw v) { return (float)v; }
  static __device__ __forceinline__ raw down(acc v) { return (_Float16)v; }
  static const char* name() { return "f16"; }
};

// the length of sequence b, clamped to what the storage can hold (corrupt lengths must not walk out of it; every row
// is range-checked again where it is formed)
__device__ __forceinline__ int64_t safe_len(const rua_layout& L, int64_t b) {
  int64_t len = seq_len(L, b);
  if (len < 0) len = 0;
  switch (L.kind) {
    case RUA_CAT: {
      const int64_t off = cat_off(L, b);
      if (off < 0 || off > L.n_rows) return 0;
      return len < L.n_rows - off ? len : L.n_rows - off;
    }
    case RUA_LEFT:  return len < L.T_phys ? len : L.T_phys;
    case RUA_RIGHT: { const int64_t t = L.T_log < L.T_phys ? L.T_log : L.T_phys; return len < t ? len : (t > 0 ? t : 0); }
    case RUA_PACK:  return len < L.T ? len : L.T;
  }
  return 0;
}

// padding rows of sequence b in a LEFT / RIGHT storage: position j of [0, T_phys) holds no token
__device__ __forceinline__ bool is_pad(const rua_layout& L, int64_t j, int64_t len) {
  if (L.kind == RUA_LEFT) return j >= len;
  const int64_t lo = L.T_log - len;
  return j < lo || j >= L.T_log;
}

// `nb` bytes (a row) in pieces of W bytes, W a power of two that divides nb and every base address
__device__ __forceinline__ void ld_row_w(const char* p, int nb, int W, void* dst) {
  if (W == 16) { *(uint4*)dst = *(const uint4*)p; return; }
  if (W == 8) {
#pragma unroll
    for (int i = 0; i < 2; ++i) if (i * 8 < nb) ((uint2*)dst)[i] = ((const uint2*)p)[i];
    return;
  }
  if (W == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i * 4 < nb) ((uint32_t*)dst)[i] = ((const uint32_t*)p)[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) if (i * 2 < nb) ((uint16_t*)dst)[i] = ((const uint16_t*)p)[i];
}
__device__ __forceinline__ void st_row_w(char* p, int nb, int W, const void* src) {
  if (W == 16) { *(uint4*)p = *(const uint4*)src; return; }
  if (W == 8) {
#pragma unroll
    for (int i = 0; i < 2; ++i) if (i * 8 < nb) ((uint2*)p)[i] = ((const uint2*)src)[i];
    return;
  }
  if (W == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i * 4 < nb) ((uint32_t*)p)[i] = ((const uint32_t*)src)[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) if (i * 2 < nb) ((uint16_t*)p)[i] = ((const uint16_t*)src)[i];
}

// ---------------------------------------------------------------- one-liners over the accumulator type
__device__ __forceinline__ float seg_exp(float v) { return expf(v); }
__device__ __forceinline__ double seg_exp(double v) { return exp(v); }
__device__ __forceinline__ float seg_log(float v) { return logf(v); }
__device__ __forceinline__ double seg_log(double v) { return log(v); }
template <typename A> __device__ __forceinline__ A seg_inf();
template <> __device__ __forceinline__ float seg_inf<float>() { return __builtin_inff(); }
template <> __device__ __forceinline__ double seg_inf<double>() { return __builtin_inf(); }
template <typename A> __device__ __forceinline__ A seg_nan();
template <> __device__ __forceinline__ float seg_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double seg_nan<double>() { return __builtin_nan(""); }
template <typename A> __device__ __forceinline__ A seg_shfl_xor(A v, int mask) { return __shfl_xor(v, mask, RUA_WAVE); }

}  // namespace rua
