// Host walk of rua_repeat_plan.h (tests/test_repeat_surface.py builds it with -fsanitize=address,undefined): the header
// is plain C++, so the choice of the plan's form, its grid, the workspace of the cut form and the grid of the move / run
// sum can be walked over sizes no test could allocate — bounds up to 2^36, B from 0 to 2^40, every layout kind, row
// widths from 1 byte to 2^40.  A violation is a plan the launcher could not launch as computed.
#include <stdint.h>
#include <stdio.h>
#include "rua_repeat_plan.h"

using namespace rua;

static long long violations = 0, plans = 0, cuts = 0, walks = 0, walk_cuts = 0, forms[4] = {0, 0, 0, 0};

static void fail(const char* what, const rua_layout& L, int64_t rb = 0) {
  if (++violations <= 20)
    printf("VIOLATION %s: kind=%d B=%lld n_rows=%lld T_phys=%lld T_log=%lld T=%lld row_bytes=%lld\n", what, L.kind,
           (long long)L.B, (long long)L.n_rows, (long long)L.T_phys, (long long)L.T_log, (long long)L.T, (long long)rb);
}

static rua_layout make_layout(int kind, int64_t B, int64_t bound, int with_tlog) {
  static int64_t dummy;                              // PACK: a boff the plan never follows
  rua_layout L = {};
  L.kind = kind;
  L.B = B;
  switch (kind) {
    case RUA_CAT:   L.len_add = 1; L.n_rows = with_tlog ? bound * 4 + 1 : bound; L.T_log = with_tlog ? bound : 0; break;
    case RUA_LEFT:
    case RUA_RIGHT: L.T_phys = bound; L.T_log = bound; L.n_rows = B * bound; break;
    case RUA_PACK:  L.T = bound; L.boff = &dummy; L.n_rows = B * bound; break;
  }
  return L;
}

static bool cut_rule(const rua_layout& L, __int128 units) {
  const int64_t bound = sm_len_bound(L);
  return units < SEG_CUT_MAX_UNITS && bound >= SEG_CUT_MIN_LEN &&
         (bound + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK <= SEG_CUT_MAX_BLOCKS;
}

static void walk_plan(const rua_layout& L) {
  if (seg_check_entry(&L, 1, 1) != 0) { fail("entry checks refuse a sound call", L); return; }
  const int64_t bound = sm_len_bound(L);
  const rp_plan p = rp_make_plan(L);
  ++plans;
  if (L.B == 0) {
    if (p.grid || p.ws_bytes || p.maxblk) fail("a plan for an empty batch", L);
    return;
  }
  if (p.form < 0 || p.form > 3) { fail("no such form", L); return; }
  ++forms[p.form];
  if ((p.form == RP_CUT) != cut_rule(L, L.B)) fail("a cut outside the rule (or a rule without its cut)", L);
  if (p.form == RP_CUT) {
    ++cuts;
    if ((int64_t)p.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)p.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the blocks do not cover the bound exactly", L);
    if (p.ws_bytes != L.B * p.maxblk * 8) fail("ws_bytes is not one int64 per (sequence, block)", L);
    if ((__int128)p.grid != (__int128)L.B * p.maxblk || p.grid > 0x7fffffffLL) fail("the cut grid is not B * maxblk", L);
    if (p.per_wg != 1) fail("a cut unit is a workgroup's", L);
    return;
  }
  if (p.maxblk || p.ws_bytes) fail("maxblk or ws_bytes without a cut", L);
  if (p.form == RP_LANES && (bound > RP_LANES_MAX_LEN || p.per_wg != 2 * SEG_WAVES_PER_BLOCK)) fail("lanes form outside its rule", L);
  if (p.form == RP_ROWS && (bound <= RP_LANES_MAX_LEN || bound >= SEG_BLOCK_TOK || p.per_wg != SEG_WAVES_PER_BLOCK))
    fail("rows form outside its rule", L);
  if (p.form == RP_LONG && (bound < SEG_BLOCK_TOK || p.per_wg != 1)) fail("long form outside its rule", L);
  const __int128 want = ((__int128)L.B + p.per_wg - 1) / p.per_wg;
  if (p.grid < 0 || p.grid > 0x7fffffffLL) fail("a grid beyond what a launch takes", L);
  if (p.grid != 0 && (__int128)p.grid != want) fail("the grid does not cover B exactly", L);
  if (p.grid == 0 && want <= 0x7fffffffLL) fail("a grid refused that fits", L);
}

static void walk_move(const rua_layout& L, int64_t rb) {
  const rp_walk w = rp_make_walk(L, rb);
  ++walks;
  if (L.B == 0 || rb <= 0) {
    if (w.grid) fail("a walk of nothing", L, rb);
    return;
  }
  const __int128 chunks = ((__int128)rb + 127) / 128;
  if (chunks > 0x7fffffff) {
    if (w.grid) fail("a row wider than a grid has chunks got a grid", L, rb);
    return;
  }
  if (w.n_chunks != (int)chunks) fail("the chunks do not cover the row", L, rb);
  if (w.lpr_log2 != (rb <= 16 ? 0 : 3)) fail("rows of one vector take a token per thread, wider ones eight threads", L, rb);
  const __int128 units = (__int128)L.B * chunks;
  const bool cut = cut_rule(L, units);
  if ((w.maxblk > 0) != cut) fail("a cut walk outside the rule", L, rb);
  if (cut) {
    ++walk_cuts;
    const int64_t bound = sm_len_bound(L);
    if ((int64_t)w.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)w.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the walk's blocks do not cover the bound exactly", L, rb);
  }
  const __int128 want = units * (cut ? w.maxblk : 1);
  if (w.grid < 0 || w.grid > 0x7fffffffLL) fail("a walk grid beyond what a launch takes", L, rb);
  if (w.grid != 0 && (__int128)w.grid != want) fail("the walk grid does not cover every unit exactly", L, rb);
  if (w.grid == 0 && want <= 0x7fffffffLL) fail("a walk grid refused that fits", L, rb);
}

int main() {
  const int kinds[4] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT};
  const int64_t Bs[] = {0, 1, 2, 3, 7, 8, 9, 127, 128, 1023, 1024, 1025, 65536, (1LL << 31) - 8, (1LL << 31) - 1, 1LL << 31,
                        (1LL << 34) - 1, 1LL << 34, 1LL << 40};
  const int64_t bounds[] = {0, 1, 31, 32, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 1LL << 20, (1LL << 31) - 1,
                            1LL << 31, (1LL << 31) + 1, 1LL << 36};
  const int64_t widths[] = {0, 1, 2, 3, 8, 10, 16, 17, 128, 129, 1000, 1024, 1LL << 20, (1LL << 38) - 1, 1LL << 38, 1LL << 40};
  if (seg_check_entry(nullptr, 1, 1) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  for (int kind : kinds)
    for (int64_t B : Bs)
      for (int64_t bound : bounds)
        for (int with_tlog = 0; with_tlog < 2; ++with_tlog) {
          if (kind != RUA_CAT && with_tlog) continue;
          if (kind != RUA_CAT && B > 0 && bound > (1LL << 62) / B) continue;      // B * T rows of storage fit int64
          const rua_layout L = make_layout(kind, B, bound, with_tlog);
          walk_plan(L);
          for (int64_t rb : widths) walk_move(L, rb);
        }
  printf("plans %lld cuts %lld lanes %lld rows %lld long %lld walks %lld walk cuts %lld violations %lld\n", plans, cuts,
         forms[0], forms[1], forms[2], walks, walk_cuts, violations);
  return violations ? 1 : (cuts > 0 && walk_cuts > 0 && forms[0] > 0 && forms[1] > 0 && forms[2] > 0 ? 0 : 2);
}
