// rua_attention_decode_plan.h — what rua_segment_attention_decode decides BEFORE its first HIP call, as plain host C++
// (no HIP header, no device, no allocation): the column blocks of the packed (query position, head in group) columns,
// the keys per split, the number of splits and the bytes of the workspace.  rua_attention_decode_plan (include/rua.h)
// is this function; Python sizes the workspace with it and hands its answers back to the launcher, which checks them
// against the same function: one source for the numbers.  The plan reads nothing but its integer arguments — never a
// layout — so the 4 x 4 pairs of layouts of one batch share one plan and therefore one set of bits.
#pragma once
#include <stdint.h>
#include "rua.h"

namespace rua {

constexpr int DEC_COLS = 32;                     // columns of a column block: the N of the 32 x 32 matrix tile
constexpr int DEC_MAX_T = 32;                    // the most queries of one sequence (longer ones are `attention`'s)
constexpr int DEC_STEP = 128;                    // keys of one step of a workgroup: 4 waves x 32; the unit of kv_chunk
constexpr int64_t DEC_MAX_GRID = 4096;           // workgroups of a launch; more items are strided over.  Decode wants
                                                 // more, smaller workgroups than the forward's 2 048 x 128-query blocks
// A HEURISTIC NOBODY HAS TUNED: the plan splits until the work items reach about twice what the device holds at once,
// counted as 256 compute units with 4 resident workgroups each
constexpr int64_t DEC_CUS = 256;
constexpr int64_t DEC_FILL_ITEMS = 2 * 4 * DEC_CUS;

struct dec_plan {
  int64_t ncb;        // column blocks: ceil(T_max G / 32)
  int64_t kv_chunk;   // keys per split, a multiple of 128
  int64_t n_split;    // ceil(S_max / kv_chunk), at least 1
  int64_t ws_bytes;   // n_split > 1: B heads_kv ncb n_split slots of 32 (D + 2) floats (m[32], l[32], acc[32][D]); else 0
};

static int64_t dec_ceil_div(int64_t a, int64_t b) { return a <= 0 ? 0 : (a - 1) / b + 1; }

// 0, or RUA_EINVAL (an argument outside the operator's domain) / RUA_ERANGE (the items or the workspace do not fit 63 bits)
static int dec_make_plan(int64_t B, int32_t heads, int32_t heads_kv, int32_t D, int64_t T_max, int64_t S_max,
                         int64_t kv_chunk_in, dec_plan& p) {
  p = {0, DEC_STEP, 1, 0};
  if (B < 0 || heads <= 0 || heads_kv <= 0 || heads % heads_kv != 0) return RUA_EINVAL;
  if (D != 32 && D != 64 && D != 128) return RUA_EINVAL;
  if (T_max < 0 || T_max > DEC_MAX_T || S_max < 0) return RUA_EINVAL;
  if (kv_chunk_in < 0 || kv_chunk_in % DEC_STEP != 0) return RUA_EINVAL;
  const int64_t G = heads / heads_kv;
  p.ncb = dec_ceil_div(T_max * G, DEC_COLS);
  if ((double)B * (double)heads_kv * (double)p.ncb >= 4.0e18) return RUA_ERANGE;
  const int64_t base = B * heads_kv * p.ncb;                    // the items of an unsplit launch
  const int64_t whole = S_max > DEC_STEP ? dec_ceil_div(S_max, DEC_STEP) * DEC_STEP : DEC_STEP;
  if (kv_chunk_in > 0) {
    p.kv_chunk = kv_chunk_in;
  } else if (S_max <= DEC_STEP || base == 0 || base >= DEC_FILL_ITEMS) {
    p.kv_chunk = whole;                                         // the items already fill the device, or one step is all
  } else {
    int64_t want = dec_ceil_div(DEC_FILL_ITEMS, base);
    if (want > whole / DEC_STEP) want = whole / DEC_STEP;       // never a chunk below 128
    p.kv_chunk = dec_ceil_div(dec_ceil_div(S_max, want), DEC_STEP) * DEC_STEP;
  }
  p.n_split = S_max > p.kv_chunk ? dec_ceil_div(S_max, p.kv_chunk) : 1;
  if (p.n_split > 1) {
    const double bytes = (double)base * (double)p.n_split * DEC_COLS * (D + 2) * 4.0;
    if (bytes >= 4.0e18) return RUA_ERANGE;
    p.ws_bytes = base * p.n_split * DEC_COLS * (D + 2) * 4;
  }
  return 0;
}

}  // namespace rua
