// rua_seg.h — what the per-sequence operators (rua_softmax.hip, rua_scan.hip) share: the element types, the clamped
// sequence length, the padding test, narrow-row accesses and the host-side layout checks.
#pragma once
#include "rua_dev.h"

namespace rua {

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

// ---------------------------------------------------------------- host side
static int sm_check_layout(const rua_layout* L) {
  if (!L || L->B < 0 || L->n_rows < 0) return RUA_EINVAL;
  switch (L->kind) {
    case RUA_CAT:   return (L->lens && !L->off) ? RUA_EINVAL : 0;
    case RUA_LEFT:
    case RUA_RIGHT: return (L->T_phys >= 0 && L->n_rows <= L->B * L->T_phys) ? 0 : RUA_EINVAL;
    case RUA_PACK:  return (L->T < 0 || (L->T > 0 && !L->boff)) ? RUA_EINVAL : 0;
  }
  return RUA_EINVAL;
}

// an upper bound of the longest sequence that needs no look at the device
static int64_t sm_len_bound(const rua_layout& L) {
  switch (L.kind) {
    case RUA_CAT:   return L.T_log > 0 && L.T_log < L.n_rows ? L.T_log : L.n_rows;
    case RUA_LEFT:
    case RUA_RIGHT: return L.T_phys;
    case RUA_PACK:  return L.T;
  }
  return 0;
}

}  // namespace rua
