// rua_seg_plan.h — what the per-sequence operators (softmax, cumsum, argreduce, linear_scan, softmax_pool, norm, conv,
// compress, join, repeat_interleave) decide BEFORE their first HIP call, as plain host C++ (no HIP header): the element
// size, the layout and entry checks, the cut plan, the form of a rows launch and the slab rule of the two-walk
// operators, the launch geometry of the lanes form, the access width of the operators that move rows as bits and the
// plan of the offsets scan.  One place for all of them: a new operator of the
// family takes these and adds only its kernels, its pointer checks and the bytes it keeps per (block, padded column).
#pragma once
#include <stdint.h>
#include "rua.h"

namespace rua {

constexpr int SEG_BLOCK_TOK = 2048;             // tokens per block: the unit of every fold order and of the cut form
constexpr int64_t SEG_CUT_MAX_UNITS = 1024;     // fewer (sequence x chunk) units than this leave the chip idle ...
constexpr int64_t SEG_CUT_MIN_LEN = 4 * SEG_BLOCK_TOK;   // ... when the sequences are this long: cut them across workgroups
constexpr int64_t SEG_CUT_MAX_BLOCKS = 0x7fffffff / SEG_CUT_MAX_UNITS;   // units x blocks has to fit a grid
constexpr int SEG_WAVES_PER_BLOCK = 4;          // (rua_seg.h checks it against RUA_WAVES_PER_BLOCK)
// the `mode` of a rows kernel: the whole sequence, or the two launches of the cut form
enum { SEG_FULL = 0, SEG_PARTIAL = 1, SEG_FINISH = 2 };

// bytes of an element; 0 = the family does not take the dtype (`allow_i64`: the operators that only add or compare)
static int seg_esize(int32_t dtype, bool allow_i64) {
  switch (dtype) {
    case RUA_F32: return 4;
    case RUA_BF16: case RUA_F16: return 2;
    case RUA_F64: return 8;
    case RUA_I64: return allow_i64 ? 8 : 0;
  }
  return 0;
}

static int sm_check_layout(const rua_layout* L) {
  if (!L || L->B < 0 || L->n_rows < 0) return RUA_EINVAL;
  switch (L->kind) {
    case RUA_CAT:   return (L->lens && !L->off) ? RUA_EINVAL : 0;
    case RUA_LEFT:
    case RUA_RIGHT: return (L->T_phys >= 0 && L->n_rows <= L->B * L->T_phys) ? 0 : RUA_EINVAL;
    case RUA_PACK:  return (L->T < 0 || (L->T > 0 && !L->boff)) ? RUA_EINVAL : 0;
  }
  return RUA_EINVAL;
}

// an upper bound of the longest sequence that needs no look at the device
static int64_t sm_len_bound(const rua_layout& L) {
  switch (L.kind) {
    case RUA_CAT:   return L.T_log > 0 && L.T_log < L.n_rows ? L.T_log : L.n_rows;
    case RUA_LEFT:
    case RUA_RIGHT: return L.T_phys;
    case RUA_PACK:  return L.T;
  }
  return 0;
}

// what every entry point checks first, in this order: the layout, then H and the dtype (`es` = seg_esize of it)
static int seg_check_entry(const rua_layout* lay, int64_t H, int es) {
  const int e = sm_check_layout(lay);
  if (e != 0) return e;
  return H < 0 || !es ? RUA_EINVAL : 0;
}

// a payload whose byte offsets would not fit 64 bits is refused (RUA_ERANGE), after the operator's own pointer checks
static bool seg_too_large(const rua_layout* lay, int64_t H, int es) {
  return (double)lay->n_rows * (double)H * es >= 9.0e18;
}

// blocks per sequence when `units` (sequence x chunk) workgroups of sequences this long leave the chip idle; 0 = no cut
static int64_t seg_cut_blocks(const rua_layout& L, int64_t units) {
  const int64_t bound = sm_len_bound(L);
  return units < SEG_CUT_MAX_UNITS && bound >= SEG_CUT_MIN_LEN ? (bound + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK : 0;
}

struct seg_plan {
  int n_chunks;       // 128-byte column chunks of a row (0: the row is wider than a grid has chunks)
  int maxblk;         // > 0: the cut form, with this many blocks per sequence
  int64_t ws_bytes;   // what the cut form needs: `ws_bytes_per_column` per block and (padded) column
};

// rows of one vector (<= 16 bytes) take the lanes form and are never cut
static seg_plan seg_make_plan(const rua_layout& L, int64_t H, int es, int ws_bytes_per_column) {
  seg_plan p = {0, 0, 0};
  if (!es || H <= 0 || L.B <= 0) return p;
  const int64_t row_bytes = H * es;
  if ((row_bytes + 127) / 128 > 0x7fffffff) return p;
  p.n_chunks = (int)((row_bytes + 127) / 128);
  if (row_bytes <= 16) return p;
  const int64_t mb = seg_cut_blocks(L, L.B * p.n_chunks);
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) {
    p.maxblk = (int)mb;
    p.ws_bytes = L.B * mb * p.n_chunks * (128 / es) * ws_bytes_per_column;
  }
  return p;
}

// the grid of a rows-form launch: a workgroup per (sequence, chunk) and, when cut, block; 0 = it does not fit (RUA_ERANGE)
static int64_t seg_rows_grid(const rua_layout& L, const seg_plan& p, bool cut) {
  const int64_t grid = L.B * (int64_t)p.n_chunks * (cut ? p.maxblk : 1);
  return p.n_chunks <= 0 || grid > 0x7fffffffLL ? 0 : grid;
}

// what a rows-form launcher decides after its plan: `al`, every access a whole aligned 16-byte vector (`bases`: the
// addresses ORed together); `cut`, the cut form (the plan asks for it and the caller brought the workspace); the grid of
// the launch (seg_rows_grid; a cut grid always fits: fewer than SEG_CUT_MAX_UNITS units x at most SEG_CUT_MAX_BLOCKS)
struct seg_rows { seg_plan p; bool al; bool cut; int64_t grid; };
static seg_rows seg_rows_form(const seg_plan& p, const rua_layout& L, int64_t row_bytes, uint64_t bases, bool ws_given) {
  const bool cut = ws_given && p.maxblk > 0;
  return {p, row_bytes % 16 == 0 && bases % 16 == 0, cut, seg_rows_grid(L, p, cut)};
}

// rows of the LDS slab of the two-walk operators (softmax, norm), 0 = stream.  Resident when the sequences can be
// expected to fit a slab: the host's bound, or twice the average where a CattedSequence came without one; the bound in
// whole rounds of `slots` rows, at most `most`.  A longer sequence streams inside the same launch (the same bits).
// L.B > 0.
static int seg_slab_cap(const rua_layout& L, bool cut, int slots, int64_t most) {
  const int64_t bound = sm_len_bound(L);
  const int64_t expect = (L.kind == RUA_CAT && !(L.T_log > 0)) ? 2 * (L.n_rows / L.B) : bound;
  if (cut || expect > 1024) return 0;
  const int64_t need = (bound + slots - 1) / slots * slots;
  return (int)(need < most ? need : most);
}

// bytes per access of the operators that move rows as bits: the widest power of two, up to 16, that divides the row and
// every base address (`bases`: the addresses ORed together)
static int seg_access_width(int64_t row_bytes, uint64_t bases) {
  const uint64_t mix = (uint64_t)row_bytes | bases | 16u;
  return (int)(mix & (~mix + 1));
}

// the lanes form (rows of one vector): two sequences per wave; W = seg_access_width.  grid == 0: B does not fit
// (RUA_ERANGE)
struct seg_lanes { int W; int64_t grid; };
static seg_lanes seg_lanes_geometry(int64_t row_bytes, uint64_t bases, int64_t B) {
  const int64_t waves = (B + 1) / 2;
  const int64_t grid = (waves + SEG_WAVES_PER_BLOCK - 1) / SEG_WAVES_PER_BLOCK;
  return {seg_access_width(row_bytes, bases), grid > 0x7fffffffLL ? 0 : grid};
}

// ---------------------------------------------------------------- the offsets scan (compress, repeat_interleave)
// The operators whose result has another raggedness than their input scan ONE value per token (a 1-byte mask, an int64
// count) per sequence, so the forms of that scan go by the length bound, not by the row width:
//   SEG_SCAN_LANES  bound <= 64: two sequences per wave, 32 lanes each (8 per workgroup)
//   SEG_SCAN_ROWS   bound < SEG_BLOCK_TOK: a wave per sequence, 64 tokens per step (4 per workgroup)
//   SEG_SCAN_LONG   longer (or unknown: CAT lengths the host never saw): a workgroup per sequence, 256 tokens per step,
//                   the sum carried from step to step
//   SEG_SCAN_CUT    the family's cut rule over B units (seg_cut_blocks): a workgroup per (sequence, block), two launches,
//                   the blocks' sums in the workspace
enum seg_scan_form { SEG_SCAN_LANES = 0, SEG_SCAN_ROWS = 1, SEG_SCAN_LONG = 2, SEG_SCAN_CUT = 3 };

constexpr int64_t SEG_SCAN_LANES_MAX_LEN = 64;

struct seg_scan_plan {
  int form;           // enum seg_scan_form
  int per_wg;         // sequences a workgroup takes (CUT: 1 unit)
  int maxblk;         // CUT: blocks per sequence, else 0
  int64_t grid;       // workgroups; 0 = nothing to launch or it does not fit (RUA_ERANGE when B > 0)
  int64_t ws_bytes;   // CUT: one sum of `ws_elem_bytes` per (sequence, block), else 0
};

static seg_scan_plan seg_make_scan_plan(const rua_layout& L, int ws_elem_bytes) {
  seg_scan_plan p = {SEG_SCAN_LANES, 2 * SEG_WAVES_PER_BLOCK, 0, 0, 0};
  if (L.B <= 0) return p;
  const int64_t bound = sm_len_bound(L);
  const int64_t mb = seg_cut_blocks(L, L.B);
  if (mb > 0 && mb <= SEG_CUT_MAX_BLOCKS) {
    p.form = SEG_SCAN_CUT;
    p.per_wg = 1;
    p.maxblk = (int)mb;
    p.grid = L.B * mb;                            // < SEG_CUT_MAX_UNITS * SEG_CUT_MAX_BLOCKS <= 2^31 - 1
    p.ws_bytes = L.B * mb * ws_elem_bytes;
    return p;
  }
  if (bound <= SEG_SCAN_LANES_MAX_LEN) { p.form = SEG_SCAN_LANES; p.per_wg = 2 * SEG_WAVES_PER_BLOCK; }
  else if (bound < SEG_BLOCK_TOK) { p.form = SEG_SCAN_ROWS; p.per_wg = SEG_WAVES_PER_BLOCK; }
  else { p.form = SEG_SCAN_LONG; p.per_wg = 1; }
  const int64_t grid = (L.B - 1) / p.per_wg + 1;  // (B - 1) / per_wg + 1: B itself may be 2^63 - 1
  p.grid = grid > 0x7fffffffLL ? 0 : grid;
  return p;
}

}  // namespace rua
