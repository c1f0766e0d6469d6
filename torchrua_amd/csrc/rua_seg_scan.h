// rua_seg_scan.h — the offsets scan of the operators whose result has another raggedness than their input
// (rua_compress.hip, rua_repeat.hip, rua_runs.hip; included by these alone): ONE value per token of the input's storage layout,
// scanned exclusively per sequence.  out[row] = what the operator makes of the token's value and of the sum in front of
// it in its sequence, Op::PAD for a padding row; new_lens[b] = the sum over the sequence.  Integer work: every form gives
// the same bits.  Its host plan is seg_make_scan_plan (rua_seg_plan.h).
//
// An operator is a struct `Op` that holds what differs and nothing else:
//   in_t, out_t, sum_t, val_t       the element read, the element written, the sums (registers, LDS, workspace) and
//                                   the value of one token
//   load(in, row, bad)              the value of the token in storage row `row`; ++bad for a value it does not take
//   wave_prefix<G>(v, lane, q, before, total)   over the min(G, 64) lanes that scan together: the sum in front of the
//                                   lane and the sum of all
//   store(v, position)              what out[row] gets
//   PAD                             what a padding row of a LEFT / RIGHT storage gets
//   COUNTS_INVALID                  whether `bad` is added to new_lens[B] (a word the entry point zeroed)
//   kernel(), phase1()              the names of the trace records
#pragma once
#include <stdio.h>
#include <atomic>
#include "rua_seg.h"

namespace rua {

extern std::atomic<int> g_trace_on;        // the dispatch trace (rua_reduce.hip)
void trace_add(const char* rec);

// G lanes walk one sequence, G tokens per step: 32 (two sequences per wave), 64 (a wave per sequence) or 256 (a
// workgroup per sequence, or — maxblk > 0, the cut form — per block of SEG_BLOCK_TOK tokens of one).  Inside a wave the
// sum in front of a lane is the operator's wave_prefix; a workgroup adds the sums of the waves below through LDS; the
// sum of the steps before is carried in a register.
// phase 0: `out` and new_lens in one launch.  The cut form takes two: phase 1 leaves every block's sum in
// ws[b * maxblk + blk] (and counts the invalid values); phase 2 adds the sums of the blocks before its own in block
// order and writes `out`, the last block also new_lens.  Padding rows of a LEFT / RIGHT storage get Op::PAD (block 0
// writes them).
// the row of `small` that the token of big's row `row` (sequence b) goes to by the rank table of a compress plan, or
// -1: dropped, or a rank that names no token of the new sequence (a rank table that does not belong to these layouts
// must not index out of range)
__device__ __forceinline__ int64_t cm_small_row(const rua_layout& S, const int32_t* rank, int64_t b, int64_t row,
                                                int64_t slen) {
  const int64_t r = rank[row];
  if (r < 0 || r >= slen) return -1;
  const int64_t sr = token_to_row(S, b, r, slen);
  return sr >= 0 && sr < S.n_rows ? sr : -1;
}

template <int G, typename Op>
__global__ __launch_bounds__(RUA_BLOCK) void seg_offsets_kernel(rua_layout L, const typename Op::in_t* __restrict__ in,
                                                                typename Op::out_t* __restrict__ out,
                                                                int64_t* __restrict__ new_lens, int maxblk,
                                                                typename Op::sum_t* ws, int phase) {
  using sum_t = typename Op::sum_t;
  constexpr int PER_WG = RUA_BLOCK / G;
  __shared__ sum_t wsum[RUA_WAVES_PER_BLOCK];
  const int tid = threadIdx.x;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int q = tid % G;
  int64_t b = (int64_t)blockIdx.x * PER_WG + tid / G;
  int blk = 0;
  if (G == RUA_BLOCK && maxblk > 0) {
    blk = (int)(blockIdx.x % (unsigned)maxblk);
    b = blockIdx.x / (unsigned)maxblk;
  }
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  int64_t tb, te;
  seg_block_range(G == RUA_BLOCK ? maxblk : 0, blk, len, tb, te);
  int64_t span = te - tb;                                      // uniform over the lanes that scan together
  if (G == 32) {
    const int64_t other = __shfl_xor(span, 32, RUA_WAVE);
    span = span > other ? span : other;
  }

  sum_t carried = 0;
  int bad = 0;
  if (phase == 2 && have) {
    for (int i = 0; i < blk; ++i) carried += ws[b * maxblk + i];
  }
  for (int64_t u0 = 0; u0 < span; u0 += G) {
    const int64_t t = tb + u0 + q;
    int64_t row = -1;
    typename Op::val_t v = 0;
    if (t < te) {
      row = token_to_row(L, b, t, len);
      if (row >= 0 && row < L.n_rows) v = Op::load(in, row, bad); else row = -1;
    }
    sum_t before, total;
    Op::template wave_prefix<G>(v, lane, q, before, total);
    if (G == RUA_BLOCK) {
      if (lane == 0) wsum[w] = total;
      __syncthreads();                                         // (workgroup-uniform trip count: b and blk are)
      total = 0;
#pragma unroll
      for (int i = 0; i < RUA_WAVES_PER_BLOCK; ++i) {
        const sum_t s = wsum[i];
        if (i < w) before += s;
        total += s;
      }
      __syncthreads();
    }
    if (phase != 1 && row >= 0) out[row] = Op::store(v, carried + before);
    carried += total;
  }

  if (!have) return;
  // invalid values are rare (the caller raises on any): a vector atomic per lane that met one, into the word the entry
  // point zeroed
  if (Op::COUNTS_INVALID && phase != 2 && bad > 0) atomicAdd((unsigned long long*)(new_lens + L.B), (unsigned long long)bad);
  if (q == 0) {
    if (phase == 1) ws[b * maxblk + blk] = carried;
    else if (phase == 0 || blk == maxblk - 1) new_lens[b] = carried;
  }
  if (phase != 1 && blk == 0) seg_fill_padding(L, b, len, q, G, [&](int64_t row) { out[row] = Op::PAD; });
}

static const char* seg_scan_form_name(int form) {
  switch (form) {
    case SEG_SCAN_LANES: return "lanes";
    case SEG_SCAN_ROWS:  return "rows";
    case SEG_SCAN_LONG:  return "long";
    case SEG_SCAN_CUT:   return "cut";
  }
  return "?";
}

// the launches of plan `p` (seg_make_scan_plan, its grid checked by the caller; the cut form needs `ws`)
template <typename Op>
static int seg_launch_offsets(const seg_scan_plan& p, const rua_layout& L, const typename Op::in_t* in,
                              typename Op::out_t* out, int64_t* new_lens, void* ws, hipStream_t s) {
  const bool tr = g_trace_on.load(std::memory_order_relaxed) != 0;
  char rec[200];
  const dim3 grid((unsigned)p.grid), block(RUA_BLOCK);
  auto note = [&](const char* phase) {
    if (!tr) return;
    snprintf(rec, sizeof rec, "%s form=%s G=%d kind=%d cut=%d blocks=%d phase=%s", Op::kernel(),
             seg_scan_form_name(p.form), RUA_BLOCK / p.per_wg, L.kind, (int)(p.form == SEG_SCAN_CUT), p.maxblk, phase);
    trace_add(rec);
  };
  auto* sums = (typename Op::sum_t*)ws;
  switch (p.form) {
    case SEG_SCAN_LANES:
      note("whole");
      hipLaunchKernelGGL((seg_offsets_kernel<32, Op>), grid, block, 0, s, L, in, out, new_lens, 0, nullptr, 0);
      break;
    case SEG_SCAN_ROWS:
      note("whole");
      hipLaunchKernelGGL((seg_offsets_kernel<64, Op>), grid, block, 0, s, L, in, out, new_lens, 0, nullptr, 0);
      break;
    case SEG_SCAN_LONG:
      note("whole");
      hipLaunchKernelGGL((seg_offsets_kernel<RUA_BLOCK, Op>), grid, block, 0, s, L, in, out, new_lens, 0, nullptr, 0);
      break;
    case SEG_SCAN_CUT: {
      note(Op::phase1());
      hipLaunchKernelGGL((seg_offsets_kernel<RUA_BLOCK, Op>), grid, block, 0, s, L, in, out, new_lens, p.maxblk, sums, 1);
      const int e = (int)hipGetLastError();
      if (e) return e;
      note("finish");
      hipLaunchKernelGGL((seg_offsets_kernel<RUA_BLOCK, Op>), grid, block, 0, s, L, in, out, new_lens, p.maxblk, sums, 2);
      break;
    }
  }
  return (int)hipGetLastError();
}

}  // namespace rua
