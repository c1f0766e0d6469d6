// rua_repeat_plan.h — what the per-sequence repeat_interleave (rua_repeat.hip) decides BEFORE its first HIP call beyond
// rua_seg_plan.h, as plain host C++ (no HIP header): the counts it takes, the element of its workspace and the grid of
// the move and of the run sum.  The forms of the plan, its grid and its workspace are the family's offsets scan
// (seg_make_scan_plan); layout and entry checks, the length bound and the cut rule are rua_seg_plan.h too.
// tests/c/repeat_plan_host.cpp walks this header.
#pragma once
#include "rua_seg_plan.h"

namespace rua {

constexpr int64_t RP_MAX_COUNT = 0x7fffffffLL;   // a count above this (or below 0) is invalid: counted, taken as 0
constexpr int RP_WS_ELEM_BYTES = 8;              // the cut form keeps one int64 sum per (sequence, block)

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
