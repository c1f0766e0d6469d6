// rua_attention_paged_dev.h — what the walks over a PAGED KV cache share (rua_attention_decode_paged.hip: decode steps;
// rua_attention_paged.hip: prefill): the block table as a kernel argument, how a key position becomes a pool row, and
// the host checks of the pool, the table and the cache type that come before any HIP call.  The text was moved here
// from rua_attention_decode_paged.hip unchanged; the rules it implements are described there.
#pragma once
#include "rua_attention_decode_dev.h"

namespace rua {

struct dec_pages {
  const int32_t* table;   // [B][max_pages]
  int64_t max_pages, num_pages;
  int32_t lg;             // log2 page_size, 4 .. 8
};

// the table entry that serves lane j of the sub-tile [ks, ks + 32) of a sequence of S keys whose table row is `tb`; -1
// when nothing may be read: the sub-tile is off, the lane's key is past the end, or the column is past the table
__device__ __forceinline__ int32_t pg_entry(const dec_pages& pt, const int32_t* __restrict__ tb, int64_t S, int64_t ks,
                                            bool on, int j) {
  const int64_t pos = ks + j, col = pos >> pt.lg;
  return (on && pos < S && col < pt.max_pages) ? tb[col] : -1;
}

// the pool row of key ks + j from its table entry, -1 (zeros) past the end or for a page id outside the pool
__device__ __forceinline__ int64_t pg_row(const dec_pages& pt, int32_t page, int64_t S, int64_t ks, int j) {
  const int64_t pos = ks + j;
  if (pos >= S || page < 0 || (int64_t)page >= pt.num_pages) return -1;
  return ((int64_t)page << pt.lg) | (pos & (((int64_t)1 << pt.lg) - 1));
}

// the cache type and its scales: an unknown kv_dtype, a scale with RUA_KV_SAME, a by-value scale that is not finite and
// positive; `f8` is whether the pool holds e4m3 codes
static int pg_check_cache(int32_t kv_dtype, const float* k_scale, const float* v_scale, double k_scale_by_value,
                          double v_scale_by_value, bool& f8) {
  f8 = kv_dtype == RUA_KV_E4M3;
  if (kv_dtype != RUA_KV_SAME && !f8) return RUA_EINVAL;
  if (f8 ? dec8_bad_scale(k_scale_by_value) || dec8_bad_scale(v_scale_by_value)
         : k_scale || v_scale || k_scale_by_value != 1.0 || v_scale_by_value != 1.0)
    return RUA_EINVAL;
  return 0;
}

// the checks that are the paged entries' own, in front of those of their walks; `lg` is log2 page_size
static int pg_check(const rua_layout* q, int32_t heads_kv, int32_t D, int kv_es, const void* k_ptr, const void* v_ptr,
                    const int32_t* page_table, int64_t max_pages, int32_t page_size, int64_t num_pages, int64_t S_max,
                    int32_t& lg) {
  for (lg = 4; lg <= 8 && (1 << lg) != page_size; ++lg) {}
  if (lg > 8 || max_pages < 0 || num_pages < 0 || !q) return RUA_EINVAL;
  if ((q->B > 0 && max_pages > 0 && !page_table) || (num_pages > 0 && (!k_ptr || !v_ptr))) return RUA_EINVAL;
  if ((uintptr_t)page_table & 3) return RUA_EALIGN;
  if (max_pages > 0x7fffffffLL || (double)q->B * (double)max_pages >= 4.0e18) return RUA_ERANGE;
  if ((double)num_pages * page_size * (double)heads_kv * D * kv_es >= 9.0e18) return RUA_ERANGE;
  if ((double)S_max > (double)max_pages * page_size) return RUA_EINVAL;   // the longest sequence fits the table
  return 0;
}

}  // namespace rua
