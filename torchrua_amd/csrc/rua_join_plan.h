// rua_join_plan.h — what rua_segment_join decides BEFORE its first HIP call, as plain host C++ (no HIP header): the
// access width, how many threads own one row, how many threads walk one unit (a sequence, or a block of one) and the
// grid.  The layout and entry checks, the length bound and the cut rule are rua_seg_plan.h.
// tests/c/join_plan_host.cpp walks this header alone.
#pragma once
#include "rua_seg_plan.h"

namespace rua {

constexpr int JN_MAX_PARTS = 8;                  // == RUA_JOIN_MAX_PARTS (rua_join.hip checks it)
constexpr int JN_BLOCK = 256;                    // threads of a workgroup (rua_join.hip checks it against RUA_BLOCK)
constexpr int64_t JN_RUN_BYTES = 16384;          // the run of destination rows a workgroup should own: the mover's 16 KiB

// ONE kernel; a form is the number of threads that walk one unit together (`tg`) and the threads that own one row (`g`):
//   JN_LANES  rows of one vector (<= 16 bytes), not cut: the family's lanes geometry — two sequences per wave, 32 lanes
//             each, a lane per token (tg = 32, g = 1; 8 sequences per workgroup)
//   JN_WAVE   wider rows whose longest joined sequence is at most a workgroup's run (bound * row_bytes <= 16 KiB): a wave
//             per sequence, 4 sequences per workgroup, so that a workgroup still owns about 16 KiB of destination rows
//   JN_ROWS   anything longer: a workgroup per sequence — or, under the family's cut rule over B units (a thread group
//             owns WHOLE rows: there are no column chunks to count), per block of SEG_BLOCK_TOK tokens; narrow rows are
//             cut too (g = 1: 256 consecutive tokens per step)
enum jn_form { JN_LANES = 0, JN_WAVE = 1, JN_ROWS = 2 };

struct jn_plan {
  int form;          // enum jn_form
  int W;             // bytes per access: seg_access_width of the row and every base address
  int tg_log2;       // log2 of the threads that walk one unit: 5, 6 or 8
  int g_log2;        // log2 of the threads that own one row: 0 .. 6 (16 bytes each per step; rows beyond 1 KiB loop)
  int maxblk;        // > 0: cut, with this many blocks per sequence
  int64_t grid;      // workgroups; 0 = it does not fit a launch (RUA_ERANGE when B > 0)
};

// `J` is the JOINED side's layout (the destination of a join, the source of an unjoin): its sequences are the units
static jn_plan jn_make_plan(const rua_layout& J, int64_t row_bytes, uint64_t bases) {
  jn_plan p = {JN_LANES, 1, 5, 0, 0, 0};
  p.W = seg_access_width(row_bytes, bases);
  if (J.B <= 0 || row_bytes <= 0) return p;
  const int64_t pieces = (row_bytes - 1) / 16 + 1;
  while (p.g_log2 < 6 && ((int64_t)1 << p.g_log2) < pieces) ++p.g_log2;
  const int64_t bound = sm_len_bound(J);
  const int64_t mb = seg_cut_blocks(J, J.B);
  int64_t grid;
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) {
    p.form = JN_ROWS;
    p.tg_log2 = 8;
    p.maxblk = (int)mb;
    grid = J.B * mb;                               // < SEG_CUT_MAX_UNITS * SEG_CUT_MAX_BLOCKS <= 2^31 - 1
  } else if (row_bytes <= 16) {
    p.form = JN_LANES;
    p.tg_log2 = 5;
    grid = seg_lanes_geometry(row_bytes, bases, J.B).grid;
  } else if (bound <= JN_RUN_BYTES / row_bytes) {
    p.form = JN_WAVE;
    p.tg_log2 = 6;
    grid = (J.B - 1) / SEG_WAVES_PER_BLOCK + 1;    // (B - 1) / n + 1: B itself may be 2^63 - 1
  } else {
    p.form = JN_ROWS;
    p.tg_log2 = 8;
    grid = J.B;
  }
  p.grid = grid > 0x7fffffffLL ? 0 : grid;
  return p;
}

}  // namespace rua
