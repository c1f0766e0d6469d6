// Host walk of rua_compress_plan.h (tests/test_compress_surface.py builds it with -fsanitize=address,undefined): the
// header is plain C++, so the choice of the plan's form, its grid and the workspace of the cut form can be walked over
// sizes no test could allocate — n_rows up to 2^40, B from 0 to 2^62, every layout kind.  A violation is a plan the
// launcher could not launch as computed: a form outside its rule, a grid that does not cover every sequence (or, cut,
// every block) or exceeds what a launch takes, a workspace that is not one int32 per (sequence, block).
#include <stdint.h>
#include <stdio.h>
#include "rua_compress_plan.h"

using namespace rua;

static long long violations = 0, plans = 0, cuts = 0, forms[4] = {0, 0, 0, 0};

static void fail(const char* what, const rua_layout& L) {
  if (++violations <= 20)
    printf("VIOLATION %s: kind=%d B=%lld n_rows=%lld T_phys=%lld T_log=%lld T=%lld\n", what, L.kind, (long long)L.B,
           (long long)L.n_rows, (long long)L.T_phys, (long long)L.T_log, (long long)L.T);
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

static void walk(const rua_layout& L) {
  if (seg_check_entry(&L, 1, 1) != 0) { fail("entry checks refuse a sound call", L); return; }
  const int64_t bound = sm_len_bound(L);
  if (cp_too_long(L) != (bound >= (1LL << 31))) fail("cp_too_long is not bound >= 2^31", L);
  const cp_plan p = cp_make_plan(L);
  ++plans;
  if (L.B == 0) {
    if (p.grid || p.ws_bytes || p.maxblk) fail("a plan for an empty batch", L);
    return;
  }
  if (p.form < 0 || p.form > 3) { fail("no such form", L); return; }
  ++forms[p.form];
  const bool cut_rule = L.B < SEG_CUT_MAX_UNITS && bound >= SEG_CUT_MIN_LEN &&
                        (bound + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK <= SEG_CUT_MAX_BLOCKS;
  if ((p.form == CP_CUT) != cut_rule) fail("a cut outside the rule (or a rule without its cut)", L);
  if (p.form == CP_CUT) {
    ++cuts;
    if ((int64_t)p.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)p.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the blocks do not cover the bound exactly", L);
    if (p.ws_bytes != L.B * p.maxblk * 4) fail("ws_bytes is not one int32 per (sequence, block)", L);
    if ((__int128)p.grid != (__int128)L.B * p.maxblk || p.grid > 0x7fffffffLL) fail("the cut grid is not B * maxblk", L);
    if (p.per_wg != 1) fail("a cut unit is a workgroup's", L);
    return;
  }
  if (p.maxblk || p.ws_bytes) fail("maxblk or ws_bytes without a cut", L);
  if (p.form == CP_LANES && (bound > CP_LANES_MAX_LEN || p.per_wg != 2 * SEG_WAVES_PER_BLOCK)) fail("lanes form outside its rule", L);
  if (p.form == CP_ROWS && (bound <= CP_LANES_MAX_LEN || bound >= SEG_BLOCK_TOK || p.per_wg != SEG_WAVES_PER_BLOCK))
    fail("rows form outside its rule", L);
  if (p.form == CP_LONG && (bound < SEG_BLOCK_TOK || p.per_wg != 1)) fail("long form outside its rule", L);
  const __int128 want = ((__int128)L.B + p.per_wg - 1) / p.per_wg;
  if (p.grid < 0 || p.grid > 0x7fffffffLL) fail("a grid beyond what a launch takes", L);
  if (p.grid != 0 && (__int128)p.grid != want) fail("the grid does not cover B exactly", L);
  if (p.grid == 0 && want <= 0x7fffffffLL) fail("a grid refused that fits", L);
}

int main() {
  const int kinds[4] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT};
  const int64_t Bs[] = {0, 1, 2, 3, 7, 8, 9, 1023, 1024, 1025, 65536, (1LL << 31) - 8, (1LL << 31) - 1, 1LL << 31,
                        (1LL << 34) - 1, 1LL << 34, 1LL << 40};
  const int64_t bounds[] = {0, 1, 31, 32, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 1LL << 20, (1LL << 31) - 1,
                            1LL << 31, (1LL << 31) + 1, 1LL << 36};
  if (seg_check_entry(nullptr, 1, 1) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  for (int kind : kinds)
    for (int64_t B : Bs)
      for (int64_t bound : bounds)
        for (int with_tlog = 0; with_tlog < 2; ++with_tlog) {
          if (kind != RUA_CAT && with_tlog) continue;
          if (kind != RUA_CAT && B > 0 && bound > (1LL << 62) / B) continue;      // B * T rows of storage fit int64
          if (with_tlog && bound > (1LL << 60)) continue;
          walk(make_layout(kind, B, bound, with_tlog));
        }
  printf("plans %lld cuts %lld lanes %lld rows %lld long %lld violations %lld\n", plans, cuts, forms[0], forms[1],
         forms[2], violations);
  return violations ? 1 : (cuts > 0 && forms[0] > 0 && forms[1] > 0 && forms[2] > 0 ? 0 : 2);
}
