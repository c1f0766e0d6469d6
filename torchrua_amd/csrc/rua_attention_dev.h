// rua_attention_dev.h — what the attention kernels (rua_attention.hip: the flash-style forward and the backward;
// rua_attention_decode.hip: the split-KV decode forward; rua_attention_paged.hip: the forward over a paged cache) share: the payload types and their matrix instruction, the
// range-checked row, the LDS tile helpers, the rounding and packing of a tile into the B operand, the store of an O^T
// accumulator, the padding zeros, the band, and the entry checks of their launchers.  The text was moved here from
// rua_attention.hip unchanged; the geometry it serves is described there.
#pragma once
#include <stdint.h>
#include "rua_seg_launch.h"

namespace rua {

constexpr int64_t ATTN_MAX_GRID = 2048;
constexpr int ATTN_BLOCK_TOK = 128;                // positions of a work item: 4 waves x 32
constexpr int ATTN_KB = 64;                        // keys staged per step of the forward and the dQ kernel
constexpr int ATTN_QB = 32;                        // queries staged per step of the dK / dV kernel
static_assert(RUA_BLOCK == 4 * RUA_WAVE && ATTN_BLOCK_TOK == 32 * RUA_WAVES_PER_BLOCK, "a wave owns 32 positions");

typedef float attn_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 attn_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 attn_f16x8 __attribute__((ext_vector_type(8)));

// the payload types: 16-bit patterns in memory, one rounding, one matrix instruction
struct at_bf16 {
  // bf16 keeps 8 significant bits: a weight rounded to it is off by up to 2^-8, as much as the rounding of the result
  // itself.  The weights therefore meet v / dO as hi + lo (P rounded once, and the rounded remainder): two MFMAs
  static constexpr bool SPLIT = true;
  static __device__ __forceinline__ uint16_t down(float f) { return sm_bf16::down(f); }
  static __device__ __forceinline__ float up(uint16_t v) { return sm_bf16::up(v); }
  static __device__ __forceinline__ attn_f32x16 mfma(uint4 a, uint4 b, attn_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(attn_bf16x8, a), __builtin_bit_cast(attn_bf16x8, b), c,
                                                   0, 0, 0);
  }
};
struct at_f16 {
  static constexpr bool SPLIT = false;
  static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
  static __device__ __forceinline__ float up(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
  static __device__ __forceinline__ attn_f32x16 mfma(uint4 a, uint4 b, attn_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(attn_f16x8, a), __builtin_bit_cast(attn_f16x8, b), c,
                                                  0, 0, 0);
  }
};

// the row of token t of sequence b, range-checked where it is formed; -1: there is none
__device__ __forceinline__ int64_t attn_row(const rua_layout& L, int64_t b, int64_t t, int64_t len) {
  if (t < 0 || t >= len) return -1;
  const int64_t r = token_to_row(L, b, t, len);
  return (r >= 0 && r < L.n_rows) ? r : (int64_t)-1;
}

__device__ __forceinline__ uint16_t attn_elem(const uint4& x, int i) {
  const uint32_t w = i < 2 ? x.x : i < 4 ? x.y : i < 6 ? x.z : x.w;
  return (uint16_t)(w >> (16 * (i & 1)));
}

// ROWS positions [t0, t0 + ROWS) of head h of sequence b into LDS: plain [ROWS][D + 8] and / or transposed
// [D][ROWS + 8]; positions past the end become zeros.  All 256 threads call
template <int D, int ROWS, bool PLAIN, bool TRANS>
__device__ __forceinline__ void attn_stage(const rua_layout& L, int64_t b, int64_t len, int64_t t0, int h, int heads,
                                           const uint16_t* __restrict__ src, uint16_t* sP, uint16_t* sT, int tid) {
  constexpr int CH = D / 8, PS = D + 8, TS = ROWS + 8;
  for (int c = tid; c < ROWS * CH; c += RUA_BLOCK) {
    const int r = c / CH, dc = c % CH;
    const int64_t row = attn_row(L, b, t0 + r, len);
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) x = *(const uint4*)(src + (row * heads + h) * (int64_t)D + dc * 8);
    if (PLAIN) *(uint4*)(sP + r * PS + dc * 8) = x;
    if (TRANS) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sT[(dc * 8 + i) * TS + r] = attn_elem(x, i);
    }
  }
}

// the A operand of the second contraction: 8 tokens of row `d` of a transposed tile, in the order the accumulator layout
// keeps them in the registers 8 c .. 8 c + 7 of a lane of half g
template <int TS> __device__ __forceinline__ uint4 attn_ld_t(const uint16_t* sT, int d, int tok0, int c, int g) {
  const uint16_t* p = sT + d * TS + tok0 + 16 * c + 4 * g;
  const uint2 lo = *(const uint2*)p, hi = *(const uint2*)(p + 8);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// the registers 8 c .. 8 c + 7 of a tile, each rounded ONCE to the payload type: the B operand of the second contraction
template <typename X> __device__ __forceinline__ uint4 attn_pack8(const float* v) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)X::down(v[2 * i]) | ((uint32_t)X::down(v[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// what the rounding of attn_pack8 left behind (exact in fp32), rounded to the payload type: the lo half of a split P
template <typename X> __device__ __forceinline__ uint4 attn_pack8_lo(const float* v) {
  float r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = v[i] - X::up(X::down(v[i]));
  return attn_pack8<X>(r);
}

// the accumulator (rows d, column = the lane's token) times `mul`, rounded once, to row `dst` (D elements)
template <typename X, int D>
__device__ __forceinline__ void attn_store_row(const attn_f32x16* acc, float mul, uint16_t* dst, int g) {
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      uint32_t w[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        w[i] = (uint32_t)X::down(acc[dt][4 * r4 + 2 * i] * mul) | ((uint32_t)X::down(acc[dt][4 * r4 + 2 * i + 1] * mul) << 16);
      *(uint2*)(dst + 32 * dt + 8 * r4 + 4 * g) = make_uint2(w[0], w[1]);
    }
  }
}

// zeros into the padding rows of head h of sequence b of an L / R result (and 0 into `aux`, one float per (row, head))
template <int D>
__device__ __forceinline__ void attn_zero_padding(const rua_layout& L, int64_t b, int64_t len, int h, int heads,
                                                  uint16_t* out, uint16_t* out2, float* aux, int tid) {
  seg_fill_padding(L, b, len, tid, RUA_BLOCK, [&](int64_t row) {
    const int64_t at = (row * heads + h) * (int64_t)D;
#pragma unroll
    for (int i = 0; i < D / 8; ++i) {
      ((uint4*)(out + at))[i] = make_uint4(0u, 0u, 0u, 0u);
      if (out2) ((uint4*)(out2 + at))[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (aux) aux[row * heads + h] = 0.f;
  });
}

// the keys a query block may see: all of them, or those at or below its last position
template <bool CAUSAL> __device__ __forceinline__ int64_t attn_key_end(int64_t S, int64_t q0) {
  return (CAUSAL && q0 + ATTN_BLOCK_TOK < S) ? q0 + ATTN_BLOCK_TOK : S;
}

// THE BAND FORM (rua_segment_attention_band_*; BAND = true, CAUSAL = false).  Query t of a sequence with T queries and S
// keys sees key s iff  -left <= s - (t + shift) <= right,  shift = S - T when the masks are aligned at the END of the
// sequence and 0 otherwise; a negative bound is no bound.  Query head h reads kv head h / (heads / heads_kv), a kv row
// holds heads_kv x D elements.  Every comparison is made on the difference d = s - (t + shift), whose terms are lengths;
// `t + shift + right` is never formed (a bound may be any int64).
struct attn_band {
  int64_t left, right;
  int32_t heads_kv, align_end;
};

__device__ __forceinline__ bool attn_band_sees(const attn_band& bd, int64_t d) {
  return (bd.left < 0 || d >= -bd.left) && (bd.right < 0 || d <= bd.right);
}
// max(0, a - w), w < 0: unbounded — the first position that a band edge `w` below position `a` leaves visible
__device__ __forceinline__ int64_t attn_band_lo(int64_t a, int64_t w) { return (w < 0 || a <= w) ? 0 : a - w; }
// min(n, c + w + 1), w < 0: unbounded — one past the last of n positions that a band edge `w` above `c` leaves visible
// (it may be <= 0: an empty band)
__device__ __forceinline__ int64_t attn_band_hi(int64_t c, int64_t w, int64_t n) {
  return (w < 0 || w >= n - 1 - c) ? n : c + w + 1;
}

// ---------------------------------------------------------------- host side
static int attn_check_entry(const rua_layout* lq, const rua_layout* lk, int32_t heads, int32_t heads_kv, int32_t D,
                            int32_t dtype, double scale, int64_t bound) {
  int e;
  if ((e = sm_check_layout(lq)) != 0) return e;
  if ((e = sm_check_layout(lk)) != 0) return e;
  if (lk->B != lq->B) return RUA_EINVAL;
  if (heads <= 0 || (D != 32 && D != 64 && D != 128)) return RUA_EINVAL;
  if (heads_kv <= 0 || heads % heads_kv != 0) return RUA_EINVAL;
  if (dtype != RUA_BF16 && dtype != RUA_F16) return RUA_EINVAL;
  if (!(scale == scale) || scale - scale != 0.0 || bound < 0) return RUA_EINVAL;    // a finite number
  return 0;
}

static bool attn_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// the work items of a launch over blocks of `bound` positions, and its grid; false: too many for 63 bits
static bool attn_items(int64_t B, int32_t heads, int64_t bound, int64_t& nblk, int64_t& items, unsigned& grid) {
  nblk = (bound + ATTN_BLOCK_TOK - 1) / ATTN_BLOCK_TOK;
  if ((double)B * (double)heads * (double)nblk >= 9.0e18) return false;
  items = B * heads * nblk;
  grid = (unsigned)(items < ATTN_MAX_GRID ? items : ATTN_MAX_GRID);
  return true;
}

// LAUNCH(payload type, D) by (dtype, D): the band instantiations <X, D, false, true>
#define RUA_ATTN_DISPATCH_BAND(dtype, D, LAUNCH)                                                                       \
  do {                                                                                                                 \
    if ((dtype) == RUA_BF16) {                                                                                         \
      if ((D) == 32) LAUNCH(at_bf16, 32); else if ((D) == 64) LAUNCH(at_bf16, 64); else LAUNCH(at_bf16, 128);          \
    } else {                                                                                                           \
      if ((D) == 32) LAUNCH(at_f16, 32); else if ((D) == 64) LAUNCH(at_f16, 64); else LAUNCH(at_f16, 128);             \
    }                                                                                                                  \
  } while (0)

}  // namespace rua
