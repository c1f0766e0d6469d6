// rua_compress.hip — per-sequence compress: keep the tokens of a C / L / P / R container where a mask is set
// (rua_segment_compress_plan, rua_segment_compress_move; include/rua.h).  An extension: the first operator of the family
// whose result has ANOTHER raggedness than its input, decided by the data.
//
// Two steps with the caller's one read-back of the new lengths between them (they size the result):
//   plan  a per-sequence exclusive count over the 1-byte mask in the input's storage layout: rank[row] = the position
//         the token will have in its new sequence, -1 for a dropped token and for a padding row; new_lens[b].  Integer
//         work: every form gives the same bits.
//   move  the rows of the input (`big`) with rank >= 0 go to the row of token (b, rank) of the result (`small`), found
//         from small's rua_layout whatever its kind; `expand` is the adjoint: the rows of big with rank >= 0 read that
//         row of small, every other row of big — padding included — is written as zeros.
// Both walk sequence by sequence (token_to_row), so b is known by construction and a PackedSequence, whose tokens of one
// sequence are strided, or a right-aligned batch, whose tokens are offset, take the same walk as a CattedSequence.
// Rows move as bits: plain vector loads and stores of the widest power of two (up to 16 bytes) that divides the row and
// both base addresses.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_scan.h"
#include "rua_compress_plan.h"

namespace rua {

constexpr int CM_SLOTS = 32;               // move: tokens a step of a workgroup (rows form) or half wave (lanes form) takes
constexpr int CM_LPR = 8;                  // rows form: 16-byte pieces per row chunk (128 bytes)
constexpr int CM_UNR = 4;                  // tokens in flight per thread
static_assert(CM_SLOTS * CM_LPR == RUA_BLOCK, "a thread per (token slot, 16-byte piece of the chunk)");
static_assert(RUA_WAVE == 64, "the counts below are 64-bit ballots");

// ---------------------------------------------------------------- the plan
// the family's offsets scan (rua_seg_scan.h) over the mask: a token's value is whether it is kept, the sum in front of a
// lane a popcount of the lower lanes' bits of one 64-bit ballot, and a kept token stores its position, a dropped one -1
struct cp_scan {
  using in_t = uint8_t;
  using out_t = int32_t;
  using sum_t = int32_t;
  using val_t = bool;
  static constexpr bool COUNTS_INVALID = false;
  static constexpr int32_t PAD = -1;
  static const char* kernel() { return "seg_compress_plan_kernel"; }
  static const char* phase1() { return "count"; }
  static __device__ __forceinline__ bool load(const uint8_t* mask, int64_t row, int&) { return mask[row] != 0; }
  template <int G>
  static __device__ __forceinline__ void wave_prefix(bool keep, int lane, int q, int32_t& before, int32_t& total) {
    const unsigned long long bal = __ballot(keep);
    if (G == 32) {
      const uint32_t m = (uint32_t)(bal >> (lane & 32));
      before = __popc(m & ((1u << q) - 1u));
      total = __popc(m);
    } else {
      before = __popcll(bal & ((1ull << lane) - 1ull));
      total = __popcll(bal);
    }
  }
  static __device__ __forceinline__ int32_t store(bool keep, int32_t pos) { return keep ? pos : -1; }
};
static_assert(sizeof(cp_scan::sum_t) == CP_WS_ELEM_BYTES, "the workspace the host plan sizes holds the kernel's counts");

// ---------------------------------------------------------------- the move
// (the row of `small` a token of `big` goes to: cm_small_row, rua_seg_scan.h)
// Rows wider than one vector: a workgroup per unit of `big` and 128-byte column chunk; a unit is a sequence, or
// (maxblk > 0: few but long sequences) a block of SEG_BLOCK_TOK tokens of one.  Thread (q, l) = (tid / 8, tid % 8) takes
// the tokens q, q + 32, ... of the unit, CM_UNR of them in flight, and owns the l-th 16-byte piece of the chunk.
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_compress_move_rows_kernel(rua_layout S, rua_layout Bg,
                                                                           const int32_t* __restrict__ rank,
                                                                           char* small, char* big, int64_t rb,
                                                                           int n_chunks, int maxblk, int expand) {
  const int tid = threadIdx.x;
  const int l = tid & (CM_LPR - 1), q = tid >> 3;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  const int64_t unit = blockIdx.x / (unsigned)n_chunks;
  int64_t b = unit;
  int blk = 0;
  if (maxblk > 0) { blk = (int)(unit % maxblk); b = unit / maxblk; }
  if (b >= Bg.B) return;
  const int64_t col0 = (int64_t)c * 128 + (int64_t)l * 16;
  const int nb = rb - col0 >= 16 ? 16 : (rb - col0 > 0 ? (int)(rb - col0) : 0);
  if (nb <= 0) return;
  const int64_t len = safe_len(Bg, b), slen = safe_len(S, b);
  int64_t tb, te;
  seg_block_range(maxblk, blk, len, tb, te);

  for (int64_t t0 = tb + q; t0 < te; t0 += CM_SLOTS * CM_UNR) {
    int64_t rows[CM_UNR], srows[CM_UNR];
    row_vec v[CM_UNR];
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      const int64_t t = t0 + (int64_t)i * CM_SLOTS;
      rows[i] = srows[i] = -1;
      row_zero(v[i]);
      if (t < te) {
        const int64_t row = token_to_row(Bg, b, t, len);
        if (row >= 0 && row < Bg.n_rows) {
          rows[i] = row;
          srows[i] = cm_small_row(S, rank, b, row, slen);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      if (srows[i] < 0) continue;
      if (expand) row_ld<W>(small + srows[i] * rb + col0, nb, v[i]);
      else row_ld<W>(big + rows[i] * rb + col0, nb, v[i]);
    }
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      if (expand) {
        if (rows[i] >= 0) row_st<W>(big + rows[i] * rb + col0, nb, v[i]);
      } else if (srows[i] >= 0) {
        row_st<W>(small + srows[i] * rb + col0, nb, v[i]);
      }
    }
  }

  if (blk == 0) {
    row_vec z;
    row_zero(z);
    char* out = expand ? big : small;
    seg_fill_padding(expand ? Bg : S, b, expand ? len : slen, q, CM_SLOTS,
                     [&](int64_t row) { row_st<W>(out + row * rb + col0, nb, z); });
  }
}

// Rows of one vector (<= 16 bytes): the family's lanes geometry — a wave takes two sequences, 32 lanes each; lane r of
// a half takes the tokens r, r + 32, ... of its sequence, CM_UNR of them in flight.  Never cut.
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_compress_move_lanes_kernel(rua_layout S, rua_layout Bg,
                                                                            const int32_t* __restrict__ rank,
                                                                            char* small, char* big, int nb, int expand) {
  const int tid = threadIdx.x;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int q = lane & (CM_SLOTS - 1);
  const int64_t b = ((int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + w) * 2 + (lane >> 5);
  if (b >= Bg.B) return;
  const int64_t len = safe_len(Bg, b), slen = safe_len(S, b);

  for (int64_t t0 = q; t0 < len; t0 += CM_SLOTS * CM_UNR) {
    int64_t rows[CM_UNR], srows[CM_UNR];
    row_vec v[CM_UNR];
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      const int64_t t = t0 + (int64_t)i * CM_SLOTS;
      rows[i] = srows[i] = -1;
      row_zero(v[i]);
      if (t < len) {
        const int64_t row = token_to_row(Bg, b, t, len);
        if (row >= 0 && row < Bg.n_rows) {
          rows[i] = row;
          srows[i] = cm_small_row(S, rank, b, row, slen);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      if (srows[i] < 0) continue;
      if (expand) row_ld<W>(small + srows[i] * nb, nb, v[i]);
      else row_ld<W>(big + rows[i] * nb, nb, v[i]);
    }
#pragma unroll
    for (int i = 0; i < CM_UNR; ++i) {
      if (expand) {
        if (rows[i] >= 0) row_st<W>(big + rows[i] * nb, nb, v[i]);
      } else if (srows[i] >= 0) {
        row_st<W>(small + srows[i] * nb, nb, v[i]);
      }
    }
  }

  row_vec z;
  row_zero(z);
  char* out = expand ? big : small;
  seg_fill_padding(expand ? Bg : S, b, expand ? len : slen, q, CM_SLOTS,
                   [&](int64_t row) { row_st<W>(out + row * nb, nb, z); });
}

// ---------------------------------------------------------------- host side
static int cm_launch_move(const rua_layout& S, const rua_layout& Bg, const int32_t* rank, char* small, char* big,
                          int64_t rb, int expand, hipStream_t s) {
  const uint64_t bases = (uint64_t)(uintptr_t)small | (uint64_t)(uintptr_t)big;
  const int W = seg_access_width(rb, bases);
  const bool tr = g_trace_on.load(std::memory_order_relaxed) != 0;
  char rec[200];
  if (rb <= 16) {
    const seg_lanes ln = seg_lanes_geometry(rb, bases, Bg.B);
    if (!ln.grid) return RUA_ERANGE;
    if (tr) {
      snprintf(rec, sizeof rec, "seg_compress_move_lanes_kernel W=%d row_bytes=%d expand=%d small=%d big=%d cut=0", W,
               (int)rb, expand, S.kind, Bg.kind);
      trace_add(rec);
    }
#define RUA_CM_LANES(WV)                                                                                               \
  hipLaunchKernelGGL((seg_compress_move_lanes_kernel<WV>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, S, Bg, rank, \
                     small, big, (int)rb, expand)
    RUA_DISPATCH_W(W, RUA_CM_LANES)
#undef RUA_CM_LANES
  } else {
    const seg_plan p = seg_make_plan(Bg, rb, 1, 0);
    const bool cut = p.maxblk > 0;
    const int64_t grid = seg_rows_grid(Bg, p, cut);
    if (!grid) return RUA_ERANGE;
    if (tr) {
      snprintf(rec, sizeof rec, "seg_compress_move_rows_kernel W=%d row_bytes=%lld expand=%d small=%d big=%d cut=%d blocks=%d chunks=%d",
               W, (long long)rb, expand, S.kind, Bg.kind, (int)cut, p.maxblk, p.n_chunks);
      trace_add(rec);
    }
#define RUA_CM_ROWS(WV)                                                                                                \
  hipLaunchKernelGGL((seg_compress_move_rows_kernel<WV>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, S, Bg, rank,     \
                     small, big, rb, p.n_chunks, p.maxblk, expand)
    RUA_DISPATCH_W(W, RUA_CM_ROWS)
#undef RUA_CM_ROWS
  }
  return (int)hipGetLastError();
}

// the layout (a mask has one byte per storage row), then the length bound: a rank is an int32
static int cp_check_entry(const rua_layout* lay, int64_t row_bytes) {
  const int e = seg_check_entry(lay, row_bytes, 1);
  if (e != 0) return e;
  return cp_too_long(*lay) ? RUA_ERANGE : 0;
}

}  // namespace rua

extern "C" int64_t rua_compress_ws_bytes(const rua_layout* lay) {
  using namespace rua;
  if (cp_check_entry(lay, 1) != 0) return 0;
  return seg_make_scan_plan(*lay, CP_WS_ELEM_BYTES).ws_bytes;
}

extern "C" int rua_segment_compress_plan(const rua_layout* lay, const void* mask, int32_t* rank, int64_t* new_lens,
                                         void* ws, void* stream) {
  using namespace rua;
  int e;
  if ((e = cp_check_entry(lay, 1)) != 0) return e;
  if (lay->B == 0) return 0;
  if (!new_lens || (lay->n_rows > 0 && (!mask || !rank))) return RUA_EINVAL;
  if ((const void*)rank == mask || (const void*)new_lens == mask || (const void*)new_lens == (const void*)rank)
    return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)rank % 4 || (uint64_t)(uintptr_t)new_lens % 8 || (uint64_t)(uintptr_t)ws % 4) return RUA_EALIGN;
  seg_scan_plan p = seg_make_scan_plan(*lay, CP_WS_ELEM_BYTES);
  if (p.form == SEG_SCAN_CUT && !ws) {                         // ws == NULL: do not cut
    p.form = SEG_SCAN_LONG;
    p.maxblk = 0;
    p.grid = lay->B;
  }
  if (p.grid <= 0 || p.grid > 0x7fffffffLL) return RUA_ERANGE;
  return seg_launch_offsets<cp_scan>(p, *lay, (const uint8_t*)mask, rank, new_lens, ws, (hipStream_t)stream);
}

extern "C" int rua_segment_compress_move(const rua_layout* small, const rua_layout* big, const int32_t* rank,
                                         void* small_data, void* big_data, int64_t row_bytes, int32_t expand,
                                         void* stream) {
  using namespace rua;
  int e;
  if ((e = cp_check_entry(big, row_bytes)) != 0) return e;
  if ((e = cp_check_entry(small, row_bytes)) != 0) return e;
  if (small->B != big->B) return RUA_EINVAL;
  const rua_layout* dst = expand ? big : small;
  if (big->B == 0 || row_bytes == 0 || dst->n_rows == 0) return 0;
  if (!rank || !small_data || !big_data || small_data == big_data) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)rank % 4) return RUA_EALIGN;
  if (seg_too_large(big, row_bytes, 1) || seg_too_large(small, row_bytes, 1)) return RUA_ERANGE;
  return cm_launch_move(*small, *big, rank, (char*)small_data, (char*)big_data, row_bytes, expand ? 1 : 0,
                        (hipStream_t)stream);
}
