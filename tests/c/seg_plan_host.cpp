// Host walk of rua_seg_plan.h (tests/test_seg_plan.py builds it with -fsanitize=address,undefined): the header is plain
// C++, so the cut plan, the rows grid and the lanes geometry of the per-sequence operators can be walked over sizes no
// test could allocate — n_rows up to 2^40, H up to 2^20, B from 0 to 2^31, every layout kind, every element size.
// A violation is a plan the launchers could not launch as they compute it: a grid beyond 2^31 - 1 workgroups that
// seg_rows_grid / seg_lanes_geometry did not refuse, a block or chunk count that does not cover the bound or the row,
// a workspace that is not exactly one slot per (sequence, block, chunk, padded column), or a cut outside the rule.
// seg_rows_form (al, cut and the grid of a rows launch) and seg_slab_cap (the resident slab of softmax and norm) are
// walked over the same plans: a cut without its workspace, a slab for a cut or a long sequence, a slab beyond its cap.
// The plan of the offsets scan (seg_make_scan_plan: compress, repeat_interleave) is walked here too, for both workspace
// elements, over B up to 2^40 and bounds up to 2^36: a form outside its rule, a grid that does not cover every sequence
// (or, cut, every block) or exceeds what a launch takes, a workspace that is not one element per (sequence, block).
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include "rua_seg_plan.h"
#include "plan_walk.h"

using namespace rua;

static long long plans = 0, cuts = 0, forms = 0, slabs = 0, scan_plans = 0, scan_cuts = 0, scan_forms[4] = {0, 0, 0, 0};

static void fail(const char* what, const rua_layout& L, int64_t H, int es) {
  if (++violations <= 20)
    printf("VIOLATION %s: kind=%d B=%lld n_rows=%lld T_phys=%lld T_log=%lld T=%lld H=%lld es=%d\n", what, L.kind,
           (long long)L.B, (long long)L.n_rows, (long long)L.T_phys, (long long)L.T_log, (long long)L.T, (long long)H, es);
}

static rua_layout make_layout(int kind, int64_t B, int64_t n_rows, int with_tlog) {
  static int64_t dummy;                              // PACK: a boff the plan never follows
  rua_layout L = {};
  L.kind = kind;
  L.B = B;
  L.n_rows = n_rows;
  const int64_t per = B > 0 ? (n_rows + B - 1) / B : 0;
  switch (kind) {
    case RUA_CAT:   L.len_add = 1; L.T_log = with_tlog ? per : 0; break;
    case RUA_LEFT:
    case RUA_RIGHT: L.T_phys = per; L.T_log = per; break;
    case RUA_PACK:  L.T = per; L.boff = &dummy; break;
  }
  return L;
}

static void walk_plan(const rua_layout& L, int64_t H, int es, int per_col) {
  if (sm_check_layout(&L) != 0) { fail("the walk built a layout the checks refuse", L, H, es); return; }
  if (seg_check_entry(&L, H, es) != 0) { fail("entry checks refuse a sound call", L, H, es); return; }
  const seg_plan p = seg_make_plan(L, H, es, per_col);
  ++plans;
  if (L.B == 0) {
    if (p.n_chunks || p.maxblk || p.ws_bytes) fail("a plan for an empty batch", L, H, es);
    return;
  }
  const int64_t row_bytes = H * es, bound = sm_len_bound(L);
  if ((int64_t)p.n_chunks * 128 < row_bytes || ((int64_t)p.n_chunks - 1) * 128 >= row_bytes)
    fail("the chunks do not cover the row exactly", L, H, es);
  if (p.maxblk < 0 || p.ws_bytes < 0 || (p.maxblk == 0) != (p.ws_bytes == 0)) fail("maxblk and ws_bytes disagree", L, H, es);
  if (p.maxblk > 0) {
    ++cuts;
    if (row_bytes <= 16 || L.B * p.n_chunks >= SEG_CUT_MAX_UNITS || bound < SEG_CUT_MIN_LEN)
      fail("a cut outside the rule", L, H, es);
    if ((int64_t)p.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)p.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the blocks do not cover the bound exactly", L, H, es);
    if (p.ws_bytes != L.B * p.maxblk * p.n_chunks * (128 / es) * per_col) fail("ws_bytes is not one slot per unit", L, H, es);
  }
  for (int cut = 0; cut < 2; ++cut) {
    if (cut && !p.maxblk) continue;
    const int64_t grid = seg_rows_grid(L, p, cut != 0);
    // what the kernels decode from blockIdx.x: (sequence, block, chunk), in 128-bit arithmetic so that the check
    // itself cannot wrap
    const __int128 want = (__int128)L.B * p.n_chunks * (cut ? p.maxblk : 1);
    if (grid < 0 || grid > 0x7fffffffLL) fail("a rows grid beyond what a launch takes", L, H, es);
    if (grid != 0 && (__int128)grid != want) fail("the rows grid is not maxblk * n_chunks * B", L, H, es);
    if (grid == 0 && want > 0 && want <= 0x7fffffffLL) fail("a rows grid refused that fits", L, H, es);
  }
  // the form of a rows launch: al from the row and the bases, cut only with the workspace, the grid seg_rows_grid's
  for (uint64_t bases : {(uint64_t)0x1000, (uint64_t)0x1008}) {
    for (int ws = 0; ws < 2; ++ws) {
      const seg_rows r = seg_rows_form(p, L, row_bytes, bases, ws != 0);
      ++forms;
      if (r.al != (row_bytes % 16 == 0 && bases % 16 == 0)) fail("al is not 'whole aligned vectors'", L, H, es);
      if (r.cut != (ws && p.maxblk > 0)) fail("cut without the workspace or the plan", L, H, es);
      if (r.grid != seg_rows_grid(L, p, r.cut)) fail("the form's grid is not seg_rows_grid", L, H, es);
      if (r.cut && !r.grid) fail("a cut grid that does not fit", L, H, es);
      // the resident slab: never when cut, never beyond `most`, whole rounds of slots, and it holds the bound it can
      for (int slots : {32, 64}) {
        for (int64_t most : {(int64_t)224, (int64_t)480, (int64_t)1024}) {
          const int cap = seg_slab_cap(L, r.cut, slots, most);
          const int64_t expect = L.kind == RUA_CAT && !(L.T_log > 0) ? 2 * (L.n_rows / L.B) : bound;
          ++slabs;
          if (cap < 0 || cap > most || (cap % slots && cap != most)) fail("a slab beyond its cap or of broken rounds", L, H, es);
          if ((r.cut || expect > 1024) && cap) fail("a slab for sequences that stream", L, H, es);
          if (!r.cut && expect <= 1024 && cap < most && cap < bound) fail("a slab below both the bound and its cap", L, H, es);
          if (cap >= slots + bound) fail("a slab a round larger than the bound", L, H, es);
        }
      }
    }
  }
  if (row_bytes <= 16) {
    for (uint64_t bases : {(uint64_t)0, (uint64_t)0x1000, (uint64_t)0x1008, (uint64_t)0x1004, (uint64_t)0x1002}) {
      const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
      if (ln.W < 1 || ln.W > 16 || (ln.W & (ln.W - 1)) || row_bytes % ln.W || bases % ln.W)
        fail("W does not divide the row and the bases", L, H, es);
      if (ln.W < 16 && row_bytes % (2 * ln.W) == 0 && bases % (2 * ln.W) == 0) fail("W is not the widest access", L, H, es);
      if (ln.grid < 0 || ln.grid > 0x7fffffffLL) fail("a lanes grid beyond what a launch takes", L, H, es);
      // two sequences per wave, SEG_WAVES_PER_BLOCK waves per workgroup: the grid covers every sequence, with less
      // than one workgroup to spare
      const int64_t per_wg = 2 * SEG_WAVES_PER_BLOCK;
      if (ln.grid != 0 && (ln.grid * per_wg < L.B || (ln.grid - 1) * per_wg >= L.B)) fail("the lanes grid does not cover B", L, H, es);
      if (ln.grid == 0 && (L.B + per_wg - 1) / per_wg <= 0x7fffffffLL) fail("a lanes grid refused that fits", L, H, es);
    }
  }
}

static void walk_scan_plan(const rua_layout& L, int ws_elem_bytes) {
  if (seg_check_entry(&L, 1, 1) != 0) { fail("entry checks refuse a sound call", L); return; }
  const int64_t bound = sm_len_bound(L);
  const seg_scan_plan p = seg_make_scan_plan(L, ws_elem_bytes);
  ++scan_plans;
  if (L.B == 0) {
    if (p.grid || p.ws_bytes || p.maxblk) fail("a plan for an empty batch", L);
    return;
  }
  if (p.form < 0 || p.form > 3) { fail("no such form", L); return; }
  ++scan_forms[p.form];
  if ((p.form == SEG_SCAN_CUT) != cut_rule(L, L.B)) fail("a cut outside the rule (or a rule without its cut)", L);
  if (p.form == SEG_SCAN_CUT) {
    ++scan_cuts;
    if ((int64_t)p.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)p.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the blocks do not cover the bound exactly", L);
    if (p.ws_bytes != L.B * p.maxblk * ws_elem_bytes) fail("ws_bytes is not one element per (sequence, block)", L);
    if ((__int128)p.grid != (__int128)L.B * p.maxblk || p.grid > 0x7fffffffLL) fail("the cut grid is not B * maxblk", L);
    if (p.per_wg != 1) fail("a cut unit is a workgroup's", L);
    return;
  }
  if (p.maxblk || p.ws_bytes) fail("maxblk or ws_bytes without a cut", L);
  if (p.form == SEG_SCAN_LANES && (bound > SEG_SCAN_LANES_MAX_LEN || p.per_wg != 2 * SEG_WAVES_PER_BLOCK))
    fail("lanes form outside its rule", L);
  if (p.form == SEG_SCAN_ROWS && (bound <= SEG_SCAN_LANES_MAX_LEN || bound >= SEG_BLOCK_TOK || p.per_wg != SEG_WAVES_PER_BLOCK))
    fail("rows form outside its rule", L);
  if (p.form == SEG_SCAN_LONG && (bound < SEG_BLOCK_TOK || p.per_wg != 1)) fail("long form outside its rule", L);
  const __int128 want = ((__int128)L.B + p.per_wg - 1) / p.per_wg;
  if (p.grid < 0 || p.grid > 0x7fffffffLL) fail("a grid beyond what a launch takes", L);
  if (p.grid != 0 && (__int128)p.grid != want) fail("the grid does not cover B exactly", L);
  if (p.grid == 0 && want <= 0x7fffffffLL) fail("a grid refused that fits", L);
}

int main() {
  const int kinds[4] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT};
  // (dtype, whether the operator lets int64 in, the bytes it keeps per block and padded column)
  const struct { int32_t dtype; bool i64; int accs; int extra; } ops[] = {
      {RUA_F32, false, 2, 0}, {RUA_BF16, false, 2, 0}, {RUA_F16, false, 1, 0}, {RUA_F64, false, 2, 0},
      {RUA_I64, true, 1, 0},  {RUA_F32, true, 1, 8},   {RUA_F64, true, 1, 8},  {RUA_BF16, true, 1, 8}};
  const int64_t Bs[] = {0, 1, 2, 3, 7, 8, 9, 511, 512, 1023, 1024, 1025, 65536, (1LL << 31) - 8, (1LL << 31) - 1, 1LL << 31};
  const int64_t Hs[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 1000, 4096, (1LL << 20) - 1, 1LL << 20};
  const int64_t rows[] = {0, 1, 8191, 8192, 8193, 16384, 1LL << 20, (1LL << 31) - 1, 1LL << 31, (1LL << 40) - 1, 1LL << 40};

  if (seg_esize(RUA_I64, false) != 0 || seg_esize(RUA_I64, true) != 8 || seg_esize(RUA_I32, true) != 0 ||
      seg_esize(-1, true) != 0 || seg_esize(RUA_BF16 | 0x100, false) != 0) {
    printf("VIOLATION seg_esize\n");
    ++violations;
  }
  if (seg_check_entry(nullptr, 1, 4) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }

  for (int kind : kinds)
    for (const auto& op : ops)
      for (int64_t B : Bs)
        for (int64_t H : Hs)
          for (int64_t n : rows)
            for (int with_tlog = 0; with_tlog < 2; ++with_tlog) {
              if (kind != RUA_CAT && with_tlog) continue;
              // LEFT / RIGHT / PACK describe B * T rows of storage: keep that product inside int64
              if (kind != RUA_CAT && B > 0 && (n + B - 1) / B > (1LL << 62) / B) continue;
              const int es = seg_esize(op.dtype, op.i64);
              if (!es) { printf("VIOLATION seg_esize refuses dtype %d\n", op.dtype); ++violations; continue; }
              rua_layout L = make_layout(kind, B, n, with_tlog);
              if (kind != RUA_CAT && B == 0) L.n_rows = 0;
              walk_plan(L, H, es, op.accs * (es == 8 ? 8 : 4) + op.extra);
              if (seg_too_large(&L, H, es) != ((double)L.n_rows * (double)H * es >= 9.0e18)) fail("seg_too_large", L, H, es);
            }
  for (int ws_elem_bytes : {4, 8})
    for_each_bound_layout([&](const rua_layout& L) { walk_scan_plan(L, ws_elem_bytes); });
  printf("plans %lld cuts %lld forms %lld slabs %lld scan plans %lld cuts %lld lanes %lld rows %lld long %lld violations %lld\n",
         plans, cuts, forms, slabs, scan_plans, scan_cuts, scan_forms[0], scan_forms[1], scan_forms[2], violations);
  const bool seen = cuts > 0 && scan_cuts > 0 && scan_forms[0] > 0 && scan_forms[1] > 0 && scan_forms[2] > 0;
  return violations ? 1 : (seen ? 0 : 2);
}
