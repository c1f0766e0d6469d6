// rua_repeat_plan.h — what the per-sequence repeat_interleave (rua_repeat.hip) decides BEFORE its first HIP call, as
// plain host C++ (no HIP header): which of its four forms scans the counts, the launch geometry of that form and the
// workspace of the cut form; and the grid of the move and of the run sum.  Layout and entry checks, the length bound
// and the cut rule are rua_seg_plan.h.  tests/c/repeat_plan_host.cpp walks this header alone.
#pragma once
#include "rua_seg_plan.h"

namespace rua {

// the plan scans one int64 count per token, so its forms go by the length bound, as the compress plan's do:
//   RP_LANES  bound <= 64: two sequences per wave, 32 lanes each (8 per workgroup)
//   RP_ROWS   bound < SEG_BLOCK_TOK: a wave per sequence, 64 tokens per step (4 per workgroup)
//   RP_LONG   longer (or unknown: CAT lengths the host never saw): a workgroup per sequence, 256 tokens per step, the
//             sum carried from step to step
//   RP_CUT    the family's cut rule over B units (seg_cut_blocks): a workgroup per (sequence, block), two launches, the
//             blocks' sums in the workspace
enum rp_form { RP_LANES = 0, RP_ROWS = 1, RP_LONG = 2, RP_CUT = 3 };

constexpr int64_t RP_LANES_MAX_LEN = 64;
constexpr int64_t RP_MAX_COUNT = 0x7fffffffLL;   // a count above this (or below 0) is invalid: counted, taken as 0

struct rp_plan {
  int form;           // enum rp_form
  int per_wg;         // sequences a workgroup takes (CUT: 1 unit)
  int maxblk;         // CUT: blocks per sequence, else 0
  int64_t grid;       // workgroups; 0 = nothing to launch or it does not fit (RUA_ERANGE when B > 0)
  int64_t ws_bytes;   // CUT: one int64 per (sequence, block), else 0
};

static rp_plan rp_make_plan(const rua_layout& L) {
  rp_plan p = {RP_LANES, 2 * SEG_WAVES_PER_BLOCK, 0, 0, 0};
  if (L.B <= 0) return p;
  const int64_t bound = sm_len_bound(L);
  const int64_t mb = seg_cut_blocks(L, L.B);
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) {
    p.form = RP_CUT;
    p.per_wg = 1;
    p.maxblk = (int)mb;
    p.grid = L.B * mb;                            // < SEG_CUT_MAX_UNITS * SEG_CUT_MAX_BLOCKS <= 2^31 - 1
    p.ws_bytes = L.B * mb * 8;
    return p;
  }
  if (bound <= RP_LANES_MAX_LEN) { p.form = RP_LANES; p.per_wg = 2 * SEG_WAVES_PER_BLOCK; }
  else if (bound < SEG_BLOCK_TOK) { p.form = RP_ROWS; p.per_wg = SEG_WAVES_PER_BLOCK; }
  else { p.form = RP_LONG; p.per_wg = 1; }
  const int64_t grid = (L.B - 1) / p.per_wg + 1;  // (B itself may be 2^63 - 1)
  p.grid = grid > 0x7fffffffLL ? 0 : grid;
  return p;
}

// the move (walked by the DESTINATION's sequences) and the run sum (walked by the SOURCE's): a workgroup per (sequence,
// 128-byte column chunk) that walks the sequence block by block, or — the cut rule over B * chunks units of the layout
// that is walked — per (sequence, block of SEG_BLOCK_TOK tokens, chunk).  Blocks need nothing of each other: no
// workspace.  Rows of one vector (<= 16 bytes) put a token on every thread instead of on eight.
struct rp_walk {
  int n_chunks;       // 128-byte column chunks of a row (0: the row is wider than a grid has chunks)
  int lpr_log2;       // log2 of the threads a row chunk takes: 3 (eight 16-byte pieces), or 0 for rows of one vector
  int maxblk;         // > 0: cut, with this many blocks per sequence
  int64_t grid;       // workgroups; 0 = it does not fit (RUA_ERANGE)
};

static rp_walk rp_make_walk(const rua_layout& L, int64_t row_bytes) {
  rp_walk w = {0, 3, 0, 0};
  if (row_bytes <= 0 || L.B <= 0) return w;
  if ((row_bytes + 127) / 128 > 0x7fffffff) return w;
  w.n_chunks = (int)((row_bytes + 127) / 128);
  w.lpr_log2 = row_bytes <= 16 ? 0 : 3;
  // (the product in 128 bits: B and the chunk count are each below 2^63 only)
  const __int128 units = (__int128)L.B * w.n_chunks;
  const int64_t mb = units < SEG_CUT_MAX_UNITS ? seg_cut_blocks(L, (int64_t)units) : 0;
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) w.maxblk = (int)mb;
  const __int128 grid = units * (w.maxblk > 0 ? w.maxblk : 1);
  w.grid = grid > 0x7fffffffLL ? 0 : (int64_t)grid;
  return w;
}

}  // namespace rua
