// rua_compress_plan.h — what rua_segment_compress_plan decides BEFORE its first HIP call, as plain host C++ (no HIP
// header): which of its four forms counts the mask, the launch geometry of that form and the workspace of the cut form.
// Everything else the operator decides on the host — layout and entry checks, the length bound, the cut rule, the
// geometry of the move — is rua_seg_plan.h.  tests/c/compress_plan_host.cpp walks this header alone.
#pragma once
#include "rua_seg_plan.h"

namespace rua {

// the plan walks a 1-byte mask, so its forms go by the length bound, not by the row width:
//   CP_LANES  bound <= 64: two sequences per wave, 32 lanes each (8 per workgroup)
//   CP_ROWS   bound < SEG_BLOCK_TOK: a wave per sequence, 64 tokens per step (4 per workgroup)
//   CP_LONG   longer (or unknown: CAT lengths the host never saw): a workgroup per sequence, 256 tokens per step,
//             SEG_BLOCK_TOK tokens per block, the count carried from block to block
//   CP_CUT    the family's cut rule over B units (seg_cut_blocks): a workgroup per (sequence, block), two launches
enum cp_form { CP_LANES = 0, CP_ROWS = 1, CP_LONG = 2, CP_CUT = 3 };

constexpr int64_t CP_LANES_MAX_LEN = 64;
constexpr int64_t CP_MAX_LEN = 0x7fffffffLL;     // a rank is an int32: sequences of 2^31 tokens or more are refused

struct cp_plan {
  int form;           // enum cp_form
  int per_wg;         // sequences a workgroup takes (CUT: 1 unit)
  int maxblk;         // CUT: blocks per sequence, else 0
  int64_t grid;       // workgroups; 0 = nothing to launch or it does not fit (RUA_ERANGE when B > 0)
  int64_t ws_bytes;   // CUT: one int32 per (sequence, block), else 0
};

static bool cp_too_long(const rua_layout& L) { return sm_len_bound(L) > CP_MAX_LEN; }

static cp_plan cp_make_plan(const rua_layout& L) {
  cp_plan p = {CP_LANES, 2 * SEG_WAVES_PER_BLOCK, 0, 0, 0};
  if (L.B <= 0) return p;
  const int64_t bound = sm_len_bound(L);
  const int64_t mb = seg_cut_blocks(L, L.B);
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) {
    p.form = CP_CUT;
    p.per_wg = 1;
    p.maxblk = (int)mb;
    p.grid = L.B * mb;                            // < SEG_CUT_MAX_UNITS * SEG_CUT_MAX_BLOCKS <= 2^31 - 1
    p.ws_bytes = L.B * mb * 4;
    return p;
  }
  if (bound <= CP_LANES_MAX_LEN) { p.form = CP_LANES; p.per_wg = 2 * SEG_WAVES_PER_BLOCK; }
  else if (bound < SEG_BLOCK_TOK) { p.form = CP_ROWS; p.per_wg = SEG_WAVES_PER_BLOCK; }
  else { p.form = CP_LONG; p.per_wg = 1; }
  // (B - 1) / per_wg + 1: B itself may be 2^63 - 1
  const int64_t grid = (L.B - 1) / p.per_wg + 1;
  p.grid = grid > 0x7fffffffLL ? 0 : grid;
  return p;
}

}  // namespace rua
