// rua_sort_plan.h — what the per-sequence stable sort (rua_sort.hip) decides BEFORE its first HIP call beyond
// rua_seg_plan.h, as plain host C++ (no HIP header): the form by the length bound, the grids, the workspace, and the
// arithmetic of the rank-merge passes — how many passes a sequence needs, which two runs an element's run is paired
// with in a pass, where the element goes, and which ping-pong buffer a pass reads.  The merge arithmetic is marked
// RUA_HD: the kernels call the very functions tests/c/sort_plan_host.cpp walks on the host.
#pragma once
#include "rua_seg_plan.h"

#if defined(__HIPCC__)
#define RUA_HD __host__ __device__ __forceinline__
#else
#define RUA_HD inline
#endif

namespace rua {

constexpr int SORT_BLOCK_LOG2 = 11;                         // a block is SEG_BLOCK_TOK tokens: one LDS slab
static_assert((1 << SORT_BLOCK_LOG2) == SEG_BLOCK_TOK, "the sort's block is the family's block");
constexpr int64_t SORT_LANES_MAX_LEN = 64;                  // up to a wave's worth: the lanes form
constexpr int64_t SORT_MAX_LEN = 0x7fffffffLL;              // positions are 31 bits of an element
constexpr int64_t SORT_WS_HEADER = 256;                     // the workspace starts with the word of passes needed
enum { SORT_LANES = 0, SORT_BLOCK = 1, SORT_MERGE = 2 };

// ---------------------------------------------------------------- the merge (shared with the kernels)
// merge passes a sequence of `len` tokens needs after its blocks of 2^blk_log2 tokens are sorted: ceil(log2(blocks))
static RUA_HD int sort_passes(int64_t len, int blk_log2) {
  const int64_t blocks = len <= 0 ? 0 : ((len - 1) >> blk_log2) + 1;
  int p = 0;
  while (p < 62 && ((int64_t)1 << p) < blocks) ++p;
  return p;
}

// pass k merges runs of 2^(blk_log2 + k) tokens in pairs.  The pair of the run that holds position t of a sequence of
// `len`: left run [base, mid), right run [mid, end) — the right one shorter or EMPTY at the end of the sequence (an
// odd run at this level: its elements keep their places)
static RUA_HD void sort_pairing(int64_t t, int64_t len, int run_log2, int64_t& base, int64_t& mid, int64_t& end) {
  base = (t >> (run_log2 + 1)) << (run_log2 + 1);
  mid = base + ((int64_t)1 << run_log2);
  end = base + ((int64_t)1 << (run_log2 + 1));
  if (mid > len) mid = len;
  if (end > len) end = len;
}

// where the element at position t goes.  `rank`: for an element of the left run the elements of the right run that
// are SMALLER (lower bound), for one of the right run the elements of the left run that are smaller OR EQUAL (upper
// bound) — stable by construction, whatever the keys
static RUA_HD int64_t sort_dest(int64_t base, int64_t mid, int64_t t, int64_t rank) {
  return t < mid ? t + rank : base + (t - mid) + rank;
}

// the parity rule: every block sort leaves its run in buffer 0, pass k reads buffer k & 1 and writes the other one —
// except the LAST pass of a sequence, which writes the caller's outputs (no copy-back)
static RUA_HD int sort_src_buffer(int pass) { return pass & 1; }

// ---------------------------------------------------------------- the plan
// bytes one ping-pong buffer keeps per element: the key image and the position in 8 bytes, 8 + 4 for 8-byte elements
static int sort_elem_bytes(int es) { return es == 8 ? 12 : 8; }

struct sort_plan {
  int form;             // SORT_LANES | SORT_BLOCK | SORT_MERGE; -1 = refused (RUA_ERANGE)
  int G;                // LANES: lanes per sequence (8 .. 64)
  int maxblk;           // BLOCK / MERGE, not CAT: blocks per sequence the grid covers
  int passes;           // MERGE: launches of the merge kernel, from the length bound
  int64_t grid;         // workgroups of the lanes / block kernel
  int64_t merge_grid;   // workgroups of one merge pass: a thread per storage element
  int64_t buf_elems;    // MERGE: elements of one ping-pong buffer (the storage's)
  int64_t ws_bytes;     // MERGE: header + two buffers, every array padded to 256 bytes; else 0
};

static int64_t sort_pad256(int64_t n) { return (n + 255) / 256 * 256; }

static sort_plan sort_make_plan(const rua_layout& L, int64_t H, int es) {
  sort_plan p = {-1, 0, 0, 0, 0, 0, 0, 0};
  if (!es || H <= 0 || L.B <= 0) return p;
  const int64_t bound = sm_len_bound(L);
  if (bound > SORT_MAX_LEN) return p;
  const __int128 cols = (__int128)L.B * H;
  if (bound <= SORT_LANES_MAX_LEN) {
    int G = 8;
    while (G < bound) G <<= 1;
    const int per_wg = SEG_WAVES_PER_BLOCK * (64 / G);
    const __int128 grid = (cols + per_wg - 1) / per_wg;
    if (grid > 0x7fffffffLL) return p;
    p.form = SORT_LANES;
    p.G = G;
    p.grid = (int64_t)grid;
    return p;
  }
  const int passes = sort_passes(bound, SORT_BLOCK_LOG2);
  // a workgroup per (block of a sequence, column).  CAT: block 0 of every sequence, then one unit per 2 048 storage rows
  // for the later blocks (at most one later block STARTS in such a window) — a long sequence among short ones costs
  // what its rows cost, whatever the bound.  Others: B x ceil(bound / block)
  __int128 units;
  if (L.kind == RUA_CAT) {
    units = (__int128)L.B + (passes > 0 ? ((__int128)L.n_rows + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK : 0);
  } else {
    p.maxblk = (int)((bound + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK);
    units = (__int128)L.B * p.maxblk;
  }
  const __int128 grid = units * H;
  if (grid > 0x7fffffffLL) return p;
  p.grid = (int64_t)grid;
  if (passes == 0) {
    p.form = SORT_BLOCK;
    return p;
  }
  const __int128 elems = (__int128)L.n_rows * H;
  if (elems * 24 + 4096 >= ((__int128)1 << 62)) return p;
  const __int128 mgrid = (elems + 255) / 256;
  if (mgrid > 0x7fffffffLL) return p;
  p.form = SORT_MERGE;
  p.passes = passes;
  p.merge_grid = (int64_t)mgrid;
  p.buf_elems = (int64_t)elems;
  p.ws_bytes = SORT_WS_HEADER + 2 * sort_pad256(p.buf_elems * 8) + (es == 8 ? 2 * sort_pad256(p.buf_elems * 4) : 0);
  return p;
}

}  // namespace rua
