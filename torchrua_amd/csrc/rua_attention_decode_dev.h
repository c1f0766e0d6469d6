// rua_attention_decode_dev.h — what the decode walks (rua_attention_decode.hip: a bf16 / f16 cache;
// rua_attention_decode_fp8.hip: an e4m3 cache; rua_attention_decode_paged.hip: either, in pages named by a block table)
// share beyond rua_attention_dev.h and the plan: the layout of a workspace slot, the merge factor, the widths of the
// transposed V tiles, the exact e4m3 converts, and the two host steps around a walk — the checks that come before the first HIP call and
// the launch of the combine kernel.  Both are defined ONCE, in rua_attention_decode.hip, next to the combine kernel.
#pragma once
#include "rua_attention_dev.h"
#include "rua_attention_decode_plan.h"

namespace rua {

constexpr int DEC_SLOT_HEAD = 2 * DEC_COLS;        // floats before acc in a workspace slot: m[32], l[32]

// m* and the factor of every wave from the four (m_i) of a column: the merge rule, in the fixed order 0, 1, 2, 3
__device__ __forceinline__ float dec_factor(float mi, float mstar) {
  return mstar == -__builtin_inff() ? 0.f : expf(mi - mstar);
}

constexpr int DEC_TS = 32 + 8;                     // tokens of a transposed V row in LDS, padded by 16 bytes
constexpr int DEC8_TS = 32 + 4;                    // tokens of a transposed V row in LDS (see BANKS)

typedef __bf16 dec8_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 dec8_f16x2 __attribute__((ext_vector_type(2)));

// two e4m3 codes (the low or the high half of `w`) as two elements of X's type, exactly; the scale operand is 1.0
template <typename X, bool HI> __device__ __forceinline__ uint32_t dec8_pair(uint32_t w) {
  if constexpr (X::SPLIT)   // at_bf16
    return __builtin_bit_cast(uint32_t, (dec8_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  else
    return __builtin_bit_cast(uint32_t, (dec8_f16x2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
}

// eight codes (8 bytes) as one matrix operand of eight elements
template <typename X> __device__ __forceinline__ uint4 dec8_up(uint32_t lo, uint32_t hi) {
  return make_uint4(dec8_pair<X, false>(lo), dec8_pair<X, true>(lo), dec8_pair<X, false>(hi), dec8_pair<X, true>(hi));
}

static bool dec8_bad_scale(double x) { return !(x > 0.0) || x - x != 0.0; }   // not a finite positive number

// what the checks leave for the launches; run == false: the call is complete without one
struct dec_launch {
  dec_plan p;
  int64_t items, pairs, cgrid;
  unsigned grid;
  attn_band bd;
  bool run;
};

// the checks of rua_segment_attention_decode in their order; `kv_es` is the bytes of a K / V element
int dec_prepare(const rua_layout* q, const rua_layout* kv, const void* q_ptr, const void* k_ptr, const void* v_ptr,
                const void* out, const void* lse, const void* ws, int64_t ws_bytes, int32_t heads, int32_t D,
                int32_t dtype, int32_t heads_kv, int64_t left, int64_t right, int32_t align_end, double scale,
                int64_t T_max, int64_t S_max, int64_t kv_chunk, int kv_es, dec_launch& L);

// seg_attn_decode_combine_kernel over the partials a walk with n_split > 1 left in `ws`
int dec_combine(const rua_layout* q, const rua_layout* kv, const dec_launch& L, const void* ws, void* out, void* lse,
                int32_t heads, int32_t D, int32_t dtype, int32_t heads_kv, int64_t T_max, hipStream_t s);

}  // namespace rua
