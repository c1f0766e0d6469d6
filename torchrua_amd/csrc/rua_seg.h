// rua_seg.h — what the kernels of the per-sequence operators (rua_softmax.hip, rua_scan.hip, rua_argreduce.hip,
// rua_linear_scan.hip, rua_pool.hip, rua_norm.hip, rua_conv.hip, rua_compress.hip, rua_join.hip, rua_repeat.hip) share:
// the element types, the clamped sequence length, the padding test and fill, the block range of the cut form, rows
// moved as bits, narrow-row accesses and the exp / log / inf / nan / shuffle one-liners.  Their host side — checks, cut
// plan, lanes geometry, access width — is rua_seg_plan.h, what the fold operators' launchers do after it (trace, dtype
// switch, the sequencing of a rows launch) rua_seg_launch.h; the offsets scan of compress and repeat is rua_seg_scan.h.
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

// the tokens [tb, te) of a sequence of `len` that block `blk` of `maxblk` takes (maxblk == 0: all of them).  The last
// block takes what a length bound that understates left over: every token is walked
__device__ __forceinline__ void seg_block_range(int maxblk, int blk, int64_t len, int64_t& tb, int64_t& te) {
  tb = 0;
  te = len;
  if (maxblk > 0) {
    tb = (int64_t)blk * SEG_BLOCK_TOK;
    if (blk < maxblk - 1 && te > tb + SEG_BLOCK_TOK) te = tb + SEG_BLOCK_TOK;
    if (tb > te) tb = te;
  }
}

// the padding rows of sequence b of a LEFT / RIGHT storage: st(row) for the positions j0, j0 + step, ... of [0, T_phys)
// that hold no token (zeros in the compress moves, -1 in the tables of rua_seg_scan.h; rua_join.hip and rua_repeat.hip
// keep this loop spelled out in their kernels, which compile to another instruction schedule through it)
template <typename St>
__device__ __forceinline__ void seg_fill_padding(const rua_layout& D, int64_t b, int64_t dlen, int j0, int step, St st) {
  if (D.kind != RUA_LEFT && D.kind != RUA_RIGHT) return;
  for (int64_t j = j0; j < D.T_phys; j += step) {
    if (!is_pad(D, j, dlen)) continue;
    const int64_t row = b * D.T_phys + j;
    if (row < D.n_rows) st(row);
  }
}

// ---------------------------------------------------------------- rows as bits (compress, join, repeat_interleave)
// 16 bytes of a row (fewer at its end: `nb`) in accesses of W bytes, W = seg_access_width: a power of two that divides
// the row and every base address.  W is a template argument: the launchers pick the kernel with RUA_DISPATCH_W
template <int W> struct row_word;
template <> struct row_word<16> { using t = uint4; };
template <> struct row_word<8> { using t = uint2; };
template <> struct row_word<4> { using t = uint32_t; };
template <> struct row_word<2> { using t = uint16_t; };
template <> struct row_word<1> { using t = uint8_t; };
struct alignas(16) row_vec { uint32_t d[4]; };

template <int W> __device__ __forceinline__ void row_ld(const char* p, int nb, row_vec& v) {
  using T = typename row_word<W>::t;
#pragma unroll
  for (int i = 0; i < 16 / W; ++i) if (i * W < nb) ((T*)&v)[i] = ((const T*)p)[i];
}
template <int W> __device__ __forceinline__ void row_st(char* p, int nb, const row_vec& v) {
  using T = typename row_word<W>::t;
#pragma unroll
  for (int i = 0; i < 16 / W; ++i) if (i * W < nb) ((T*)p)[i] = ((const T*)&v)[i];
}
__device__ __forceinline__ void row_zero(row_vec& v) { v.d[0] = v.d[1] = v.d[2] = v.d[3] = 0u; }

// LAUNCH(16 | 8 | 4 | 2 | 1) for the access width W of a launch
#define RUA_DISPATCH_W(W, LAUNCH)                                                                                      \
  switch (W) {                                                                                                         \
    case 16: LAUNCH(16); break;                                                                                        \
    case 8:  LAUNCH(8); break;                                                                                         \
    case 4:  LAUNCH(4); break;                                                                                         \
    case 2:  LAUNCH(2); break;                                                                                         \
    default: LAUNCH(1); break;                                                                                         \
  }

// `nb` bytes (a row) in pieces of W bytes, W a power of two that divides nb and every base address.  (W at run time,
// for the fold operators, whose kernels are instantiated by element type; the movers above take row_ld<W> / row_st<W>)
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
