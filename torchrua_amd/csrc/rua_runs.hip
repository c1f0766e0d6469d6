// rua_runs.hip — per-sequence unique_consecutive (run-length encode) over a C / L / P / R container
// (rua_segment_runs_heads, rua_segment_runs_inverse, rua_segment_runs_counts; include/rua.h).  An extension: the inverse
// of repeat_interleave.  Every run of equal consecutive tokens INSIDE a sequence collapses to its first token.
//
//   heads    the only kernel that reads the payload: head[row(b, t)] = (t == 0) || row(b, t) != row(b, t - 1), one byte
//            per storage row — the mask rua_segment_compress_plan scans into the rank table and the new lengths, and
//            rua_segment_compress_move moves the values by.  The predecessor's row comes from token_to_row, so the
//            strided tokens of a PackedSequence and the offset tokens of a right-aligned batch take the same walk as a
//            CattedSequence, and a sequence's first token is never compared with anything.
//   inverse  the family's offsets scan (rua_seg_scan.h) over the same mask: the heads up to and including a token,
//            minus one — the index of the token's run inside its sequence, int64; 0 in padding rows.
//   counts   the run lengths in the layout of the RESULT: the heads scatter their positions into a table of starts laid
//            out like `counts`, then every run subtracts its start from its successor's (the last run of a sequence from
//            the sequence's length).  No atomics: a long run costs what a short one does.
// Integer work and comparisons only: every form gives the same bits.
#include <stdio.h>
#include <stdint.h>
#include <atomic>
#include "rua_seg_scan.h"
#include "rua_compress_plan.h"

namespace rua {

constexpr int RN_SLOTS = 32;               // wide compare: tokens a step of a workgroup takes
constexpr int RN_LPR = 8;                  // ... and lanes per token: 16-byte pieces of a 128-byte row chunk
static_assert(RN_SLOTS * RN_LPR == RUA_BLOCK, "a thread per (token slot, 16-byte piece of the chunk)");
static_assert(RUA_WAVE == 64, "the ballots below are 64-bit");

// ---------------------------------------------------------------- the equality rule
// whether 16 bytes of two rows differ (bytes past the row's end are zeros in both).  `eq` is the dtype code of the four
// float types — IEEE equality per element: a NaN differs from everything, -0.0 equals +0.0 — or RUA_RUNS_BITS
__device__ __forceinline__ bool rn_differ(const row_vec& a, const row_vec& p, int eq) {
  bool d = false;
  switch (eq) {
    case RUA_F32:
#pragma unroll
      for (int i = 0; i < 4; ++i) d |= !(__uint_as_float(a.d[i]) == __uint_as_float(p.d[i]));
      return d;
    case RUA_F64:
#pragma unroll
      for (int i = 0; i < 2; ++i)
        d |= !(__hiloint2double((int)a.d[2 * i + 1], (int)a.d[2 * i]) == __hiloint2double((int)p.d[2 * i + 1], (int)p.d[2 * i]));
      return d;
    case RUA_BF16:
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d |= !(__uint_as_float(a.d[i] << 16) == __uint_as_float(p.d[i] << 16));
        d |= !(__uint_as_float(a.d[i] & 0xffff0000u) == __uint_as_float(p.d[i] & 0xffff0000u));
      }
      return d;
    case RUA_F16:
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d |= !(__builtin_bit_cast(_Float16, (uint16_t)a.d[i]) == __builtin_bit_cast(_Float16, (uint16_t)p.d[i]));
        d |= !(__builtin_bit_cast(_Float16, (uint16_t)(a.d[i] >> 16)) == __builtin_bit_cast(_Float16, (uint16_t)(p.d[i] >> 16)));
      }
      return d;
  }
  return ((a.d[0] ^ p.d[0]) | (a.d[1] ^ p.d[1]) | (a.d[2] ^ p.d[2]) | (a.d[3] ^ p.d[3])) != 0u;
}

// ---------------------------------------------------------------- the walk
// G = RUA_BLOCK / per_wg lanes walk one sequence, or (maxblk > 0) one block of SEG_BLOCK_TOK tokens of one: the
// geometry of the offsets scan (seg_make_scan_plan).  Lane q of them takes the tokens tb + q, tb + q + G, ... < te
struct rn_unit { int64_t b, len, tb, te; int q, G, blk; };
__device__ __forceinline__ bool rn_take_unit(const rua_layout& L, int per_wg, int maxblk, rn_unit& u) {
  u.G = RUA_BLOCK / per_wg;
  u.q = threadIdx.x & (u.G - 1);
  u.b = (int64_t)blockIdx.x * per_wg + threadIdx.x / u.G;
  u.blk = 0;
  if (maxblk > 0) {
    u.blk = (int)(blockIdx.x % (unsigned)maxblk);
    u.b = blockIdx.x / (unsigned)maxblk;
  }
  if (u.b >= L.B) return false;
  u.len = safe_len(L, u.b);
  seg_block_range(maxblk, u.blk, u.len, u.tb, u.te);
  return true;
}

// the storage row of token (b, t), or -1 where it is not in the storage
__device__ __forceinline__ int64_t rn_row(const rua_layout& L, int64_t b, int64_t t, int64_t len) {
  const int64_t row = token_to_row(L, b, t, len);
  return row >= 0 && row < L.n_rows ? row : -1;
}

// ---------------------------------------------------------------- heads
// Rows of one vector (<= 16 bytes): a lane per token — one vector load of the row and one of its predecessor
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_runs_heads_lanes_kernel(rua_layout L, const char* __restrict__ data,
                                                                         uint8_t* __restrict__ head, int nb, int eq,
                                                                         int per_wg, int maxblk) {
  rn_unit u;
  if (!rn_take_unit(L, per_wg, maxblk, u)) return;
  for (int64_t t = u.tb + u.q; t < u.te; t += u.G) {
    const int64_t row = rn_row(L, u.b, t, u.len);
    if (row < 0) continue;
    bool h = true;
    const int64_t prev = t > 0 ? rn_row(L, u.b, t - 1, u.len) : -1;
    if (prev >= 0) {
      row_vec a, p;
      row_zero(a);
      row_zero(p);
      row_ld<W>(data + row * nb, nb, a);
      row_ld<W>(data + prev * nb, nb, p);
      h = rn_differ(a, p, eq);
    }
    head[row] = h ? 1 : 0;
  }
}

// Wider rows: a workgroup per sequence or (maxblk > 0) block of one; thread (q, l) = (tid / 8, tid % 8) takes the tokens
// q, q + 32, ... and the l-th 16-byte piece of every 128-byte chunk of the row.  The eight lanes of a token combine
// their pieces by ballot after every chunk and stop at the first chunk that differs.
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_runs_heads_rows_kernel(rua_layout L, const char* __restrict__ data,
                                                                        uint8_t* __restrict__ head, int64_t rb, int eq,
                                                                        int maxblk) {
  rn_unit u;
  if (!rn_take_unit(L, 1, maxblk, u)) return;
  const int tid = threadIdx.x;
  const int l = tid & (RN_LPR - 1), q = tid >> 3;
  const int group = tid & (RUA_WAVE - 1) & ~(RN_LPR - 1);       // the first lane of this token's eight, in its wave
  for (int64_t t = u.tb + q; t < u.te; t += RN_SLOTS) {
    const int64_t row = rn_row(L, u.b, t, u.len);
    if (row < 0) continue;
    const int64_t prev = t > 0 ? rn_row(L, u.b, t - 1, u.len) : -1;
    bool h = true;
    if (prev >= 0) {
      h = false;
      for (int64_t c0 = 0; c0 < rb && !h; c0 += 128) {          // (uniform over the eight lanes of the token)
        const int64_t col = c0 + (int64_t)l * 16;
        const int nb = rb - col >= 16 ? 16 : (rb - col > 0 ? (int)(rb - col) : 0);
        bool mine = false;
        if (nb > 0) {
          row_vec a, p;
          row_zero(a);
          row_zero(p);
          row_ld<W>(data + row * rb + col, nb, a);
          row_ld<W>(data + prev * rb + col, nb, p);
          mine = rn_differ(a, p, eq);
        }
        h = ((__ballot(mine) >> group) & 0xffull) != 0ull;
      }
    }
    if (l == 0) head[row] = h ? 1 : 0;
  }
}

// ---------------------------------------------------------------- inverse
// the offsets scan over the head mask: a token stores the heads in front of it, plus its own, minus one
struct rn_inverse_scan {
  using in_t = uint8_t;
  using out_t = int64_t;
  using sum_t = int32_t;
  using val_t = bool;
  static constexpr bool COUNTS_INVALID = false;
  static constexpr int64_t PAD = 0;
  static const char* kernel() { return "seg_runs_inverse_kernel"; }
  static const char* phase1() { return "count"; }
  static __device__ __forceinline__ bool load(const uint8_t* head, int64_t row, int&) { return head[row] != 0; }
  template <int G>
  static __device__ __forceinline__ void wave_prefix(bool h, int lane, int q, int32_t& before, int32_t& total) {
    const unsigned long long bal = __ballot(h);
    if (G == 32) {
      const uint32_t m = (uint32_t)(bal >> (lane & 32));
      before = __popc(m & ((1u << q) - 1u));
      total = __popc(m);
    } else {
      before = __popcll(bal & ((1ull << lane) - 1ull));
      total = __popcll(bal);
    }
  }
  static __device__ __forceinline__ int64_t store(bool h, int32_t pos) {
    const int64_t r = (int64_t)pos + (h ? 1 : 0) - 1;
    return r > 0 ? r : 0;                                      // (a first token that is no head: a mask that is not ours)
  }
};
static_assert(sizeof(rn_inverse_scan::sum_t) == CP_WS_ELEM_BYTES, "the workspace rule of rua_compress_ws_bytes");

// ---------------------------------------------------------------- counts
// phase starts: every head of `big` (rank >= 0) leaves its position at its run's row of the table
__global__ __launch_bounds__(RUA_BLOCK) void seg_runs_starts_kernel(rua_layout S, rua_layout Bg,
                                                                    const int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ starts, int per_wg, int maxblk) {
  rn_unit u;
  if (!rn_take_unit(Bg, per_wg, maxblk, u)) return;
  const int64_t slen = safe_len(S, u.b);
  for (int64_t t = u.tb + u.q; t < u.te; t += u.G) {
    const int64_t row = rn_row(Bg, u.b, t, u.len);
    if (row < 0) continue;
    const int64_t sr = cm_small_row(S, rank, u.b, row, slen);
    if (sr >= 0) starts[sr] = (int32_t)t;
  }
}

// phase diff: run (b, r) of `small` ends where run (b, r + 1) starts, the last one where the sequence of `big` ends
__global__ __launch_bounds__(RUA_BLOCK) void seg_runs_counts_kernel(rua_layout S, rua_layout Bg,
                                                                    const int32_t* __restrict__ starts,
                                                                    int64_t* __restrict__ counts, int per_wg, int maxblk) {
  rn_unit u;
  if (!rn_take_unit(S, per_wg, maxblk, u)) return;
  const int64_t len = safe_len(Bg, u.b);
  for (int64_t r = u.tb + u.q; r < u.te; r += u.G) {
    const int64_t row = rn_row(S, u.b, r, u.len);
    if (row < 0) continue;
    int64_t next = len;
    if (r + 1 < u.len) {
      const int64_t nrow = rn_row(S, u.b, r + 1, u.len);
      if (nrow >= 0) next = starts[nrow];
    }
    counts[row] = next - (int64_t)starts[row];
  }
  if (u.blk == 0) seg_fill_padding(S, u.b, u.len, u.q, u.G, [&](int64_t row) { counts[row] = 0; });
}

// ---------------------------------------------------------------- host side
// the walk's geometry over `lay`: the plan of the offsets scan, never with a workspace of its own
static seg_scan_plan rn_walk_plan(const rua_layout& lay) { return seg_make_scan_plan(lay, 0); }

static bool rn_grid_fits(const seg_scan_plan& p) { return p.grid > 0 && p.grid <= 0x7fffffffLL; }

static void rn_note(const char* kernel, const seg_scan_plan& p, int kind, const char* phase, int W, int64_t rb) {
  if (g_trace_on.load(std::memory_order_relaxed) == 0) return;
  char rec[200];
  int n = snprintf(rec, sizeof rec, "%s form=%s G=%d kind=%d cut=%d blocks=%d phase=%s", kernel,
                   seg_scan_form_name(p.form), RUA_BLOCK / p.per_wg, kind, (int)(p.form == SEG_SCAN_CUT), p.maxblk, phase);
  if (W > 0 && n > 0 && n < (int)sizeof rec) snprintf(rec + n, sizeof rec - n, " W=%d row_bytes=%lld", W, (long long)rb);
  trace_add(rec);
}

// the layout, then the length bound (a rank, a start and a count of heads are int32)
static int rn_check_entry(const rua_layout* lay, int64_t row_bytes) {
  const int e = seg_check_entry(lay, row_bytes, 1);
  if (e != 0) return e;
  return cp_too_long(*lay) ? RUA_ERANGE : 0;
}

}  // namespace rua

extern "C" int rua_segment_runs_heads(const rua_layout* lay, const void* data, int64_t row_bytes, int32_t eq, void* head,
                                      void* stream) {
  using namespace rua;
  int e;
  if ((e = rn_check_entry(lay, row_bytes)) != 0) return e;
  if (eq != RUA_RUNS_BITS) {
    const int es = seg_esize(eq, false);
    if (!es || row_bytes % es) return RUA_EINVAL;
  }
  if (lay->B == 0 || lay->n_rows == 0) return 0;
  if (!head || (row_bytes > 0 && !data) || data == (const void*)head) return RUA_EINVAL;
  if (seg_too_large(lay, row_bytes, 1)) return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  seg_scan_plan p = rn_walk_plan(*lay);
  if (!rn_grid_fits(p)) return RUA_ERANGE;
  const int W = seg_access_width(row_bytes, (uint64_t)(uintptr_t)data);
  if (row_bytes <= 16) {
    // (rows of no bytes are all equal: the zeroed vectors compare so)
    rn_note("seg_runs_heads_lanes_kernel", p, lay->kind, "whole", W, row_bytes);
#define RUA_RN_LANES(WV)                                                                                               \
  hipLaunchKernelGGL((seg_runs_heads_lanes_kernel<WV>), dim3((unsigned)p.grid), dim3(RUA_BLOCK), 0, s, *lay,            \
                     (const char*)data, (uint8_t*)head, (int)row_bytes, (int)eq, p.per_wg, p.maxblk)
    RUA_DISPATCH_W(W, RUA_RN_LANES)
#undef RUA_RN_LANES
  } else {
    if (p.form != SEG_SCAN_CUT) {                               // a workgroup per sequence, whatever its length
      p.form = SEG_SCAN_LONG;
      p.per_wg = 1;
      p.grid = lay->B;
      if (!rn_grid_fits(p)) return RUA_ERANGE;
    }
    rn_note("seg_runs_heads_rows_kernel", p, lay->kind, "whole", W, row_bytes);
#define RUA_RN_ROWS(WV)                                                                                                \
  hipLaunchKernelGGL((seg_runs_heads_rows_kernel<WV>), dim3((unsigned)p.grid), dim3(RUA_BLOCK), 0, s, *lay,             \
                     (const char*)data, (uint8_t*)head, row_bytes, (int)eq, p.maxblk)
    RUA_DISPATCH_W(W, RUA_RN_ROWS)
#undef RUA_RN_ROWS
  }
  return (int)hipGetLastError();
}

extern "C" int rua_segment_runs_inverse(const rua_layout* lay, const void* head, int64_t* inverse, int64_t* new_lens,
                                        void* ws, void* stream) {
  using namespace rua;
  int e;
  if ((e = rn_check_entry(lay, 1)) != 0) return e;
  if (lay->B == 0) return 0;
  if (!new_lens || (lay->n_rows > 0 && (!head || !inverse))) return RUA_EINVAL;
  if (lay->n_rows > 0 &&                                       // (a storage without rows: the tables may both be null)
      ((const void*)inverse == head || (const void*)new_lens == head || (const void*)new_lens == (const void*)inverse))
    return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)inverse % 8 || (uint64_t)(uintptr_t)new_lens % 8 || (uint64_t)(uintptr_t)ws % 4) return RUA_EALIGN;
  seg_scan_plan p = seg_make_scan_plan(*lay, CP_WS_ELEM_BYTES);
  if (p.form == SEG_SCAN_CUT && !ws) {                         // ws == NULL: do not cut
    p.form = SEG_SCAN_LONG;
    p.maxblk = 0;
    p.grid = lay->B;
  }
  if (!rn_grid_fits(p)) return RUA_ERANGE;
  return seg_launch_offsets<rn_inverse_scan>(p, *lay, (const uint8_t*)head, inverse, new_lens, ws, (hipStream_t)stream);
}

extern "C" int rua_segment_runs_counts(const rua_layout* small, const rua_layout* big, const int32_t* rank,
                                       int32_t* starts, int64_t* counts, void* stream) {
  using namespace rua;
  int e;
  if ((e = rn_check_entry(big, 1)) != 0) return e;
  if ((e = rn_check_entry(small, 1)) != 0) return e;
  if (small->B != big->B) return RUA_EINVAL;
  if (big->B == 0 || small->n_rows == 0) return 0;
  if (!rank || !starts || !counts || (const void*)starts == (const void*)counts || (const void*)starts == (const void*)rank ||
      (const void*)counts == (const void*)rank)
    return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)rank % 4 || (uint64_t)(uintptr_t)starts % 4 || (uint64_t)(uintptr_t)counts % 8) return RUA_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const seg_scan_plan pb = rn_walk_plan(*big), ps = rn_walk_plan(*small);
  if (!rn_grid_fits(pb) || !rn_grid_fits(ps)) return RUA_ERANGE;
  if (big->n_rows > 0) {
    rn_note("seg_runs_counts_kernel", pb, big->kind, "starts", 0, 0);
    hipLaunchKernelGGL(seg_runs_starts_kernel, dim3((unsigned)pb.grid), dim3(RUA_BLOCK), 0, s, *small, *big, rank, starts,
                       pb.per_wg, pb.maxblk);
    if ((e = (int)hipGetLastError()) != 0) return e;
  }
  rn_note("seg_runs_counts_kernel", ps, small->kind, "diff", 0, 0);
  hipLaunchKernelGGL(seg_runs_counts_kernel, dim3((unsigned)ps.grid), dim3(RUA_BLOCK), 0, s, *small, *big, starts, counts,
                     ps.per_wg, ps.maxblk);
  return (int)hipGetLastError();
}
