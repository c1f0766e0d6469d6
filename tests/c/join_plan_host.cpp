// Host walk of rua_join_plan.h (tests/test_join_surface.py builds it with -fsanitize=address,undefined): the header is
// plain C++, so the form of the join kernel, its thread groups, its access width and its grid can be walked over sizes
// no test could allocate — bounds up to 2^36, B from 0 to 2^40, rows from 1 byte to 2^33, every layout kind and base
// alignment.  A violation is a plan the launcher could not launch as computed: a form outside its rule, a thread group
// that does not fit its workgroup or its row, a width that does not divide the row and the bases, a grid that does not
// cover every unit or exceeds what a launch takes.
#include <stdint.h>
#include <stdio.h>
#include "rua_join_plan.h"

using namespace rua;

static long long violations = 0, plans = 0, cuts = 0, forms[3] = {0, 0, 0};

static void fail(const char* what, const rua_layout& L, int64_t rb) {
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

static void walk(const rua_layout& L, int64_t rb, uint64_t bases) {
  if (seg_check_entry(&L, rb, 1) != 0) { fail("entry checks refuse a sound call", L, rb); return; }
  const jn_plan p = jn_make_plan(L, rb, bases);
  ++plans;
  if (p.W != 1 && p.W != 2 && p.W != 4 && p.W != 8 && p.W != 16) { fail("W is not a power of two up to 16", L, rb); return; }
  if (rb % p.W || bases % (uint64_t)p.W) fail("W does not divide the row and the bases", L, rb);
  if (p.W < 16 && rb % (2 * p.W) == 0 && bases % (uint64_t)(2 * p.W) == 0) fail("a wider access would divide them too", L, rb);
  if (L.B == 0) {
    if (p.grid || p.maxblk) fail("a plan for an empty batch", L, rb);
    return;
  }
  if (p.form < 0 || p.form > 2) { fail("no such form", L, rb); return; }
  ++forms[p.form];
  const int64_t bound = sm_len_bound(L);
  const int tg = 1 << p.tg_log2, g = 1 << p.g_log2;
  if (tg != 32 && tg != 64 && tg != JN_BLOCK) fail("a thread group that is no half wave, wave or workgroup", L, rb);
  if (g > tg || g > 64) fail("more threads per row than the group (or a wave) has", L, rb);
  const int64_t pieces = (rb + 15) / 16;
  if (g < 64 && g < pieces) fail("fewer threads than 16-byte pieces below a wave's width", L, rb);
  if (g > 1 && g / 2 >= pieces) fail("twice the threads a row needs", L, rb);
  const bool cut_rule = L.B < SEG_CUT_MAX_UNITS && bound >= SEG_CUT_MIN_LEN &&
                        (bound + SEG_BLOCK_TOK - 1) / SEG_BLOCK_TOK <= SEG_CUT_MAX_BLOCKS;
  if ((p.maxblk > 0) != cut_rule) fail("a cut outside the rule (or a rule without its cut)", L, rb);
  __int128 want;
  if (p.maxblk > 0) {
    ++cuts;
    if (p.form != JN_ROWS || tg != JN_BLOCK) fail("a cut unit is a workgroup's", L, rb);
    if ((int64_t)p.maxblk * SEG_BLOCK_TOK < bound || ((int64_t)p.maxblk - 1) * SEG_BLOCK_TOK >= bound)
      fail("the blocks do not cover the bound exactly", L, rb);
    want = (__int128)L.B * p.maxblk;
  } else {
    if ((p.form == JN_LANES) != (rb <= 16)) fail("lanes form is for rows of one vector", L, rb);
    if (p.form == JN_LANES && tg != 32) fail("lanes form: 32 lanes per sequence", L, rb);
    if (p.form == JN_WAVE && (tg != 64 || (__int128)bound * rb > JN_RUN_BYTES)) fail("wave form outside its rule", L, rb);
    if (p.form == JN_ROWS && (tg != JN_BLOCK || (__int128)bound * rb <= JN_RUN_BYTES)) fail("rows form outside its rule", L, rb);
    const int per_wg = JN_BLOCK / tg;
    want = ((__int128)L.B + per_wg - 1) / per_wg;
  }
  if (p.grid < 0 || p.grid > 0x7fffffffLL) fail("a grid beyond what a launch takes", L, rb);
  if (p.grid != 0 && (__int128)p.grid != want) fail("the grid does not cover every unit exactly", L, rb);
  if (p.grid == 0 && want <= 0x7fffffffLL) fail("a grid refused that fits", L, rb);
}

int main() {
  const int kinds[4] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT};
  const int64_t Bs[] = {0, 1, 2, 3, 7, 8, 9, 1023, 1024, 1025, 65536, (1LL << 31) - 8, (1LL << 31) - 1, 1LL << 31,
                        (1LL << 34) - 1, 1LL << 34, 1LL << 40};
  const int64_t bounds[] = {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1024, 2047, 2048, 2049, 8191, 8192, 8193,
                            1LL << 20, (1LL << 31) - 1, 1LL << 31, 1LL << 36};
  const int64_t rbs[] = {1, 2, 3, 8, 15, 16, 17, 20, 24, 32, 48, 128, 132, 1000, 1024, 1025, 1040, 2048, 16384, 16385,
                         1LL << 20, (1LL << 33) + 8};
  const uint64_t bases[] = {0, 1, 2, 4, 8, 16, 0x7f0000001000ULL, 0x7f0000001008ULL, 0x7f0000001003ULL};
  if (seg_check_entry(nullptr, 1, 1) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  for (int kind : kinds)
    for (int64_t B : Bs)
      for (int64_t bound : bounds)
        for (int with_tlog = 0; with_tlog < 2; ++with_tlog) {
          if (kind != RUA_CAT && with_tlog) continue;
          if (kind != RUA_CAT && B > 0 && bound > (1LL << 62) / B) continue;      // B * T rows of storage fit int64
          const rua_layout L = make_layout(kind, B, bound, with_tlog);
          for (int64_t rb : rbs)
            for (uint64_t base : bases) walk(L, rb, base);
        }
  printf("plans %lld cuts %lld lanes %lld wave %lld rows %lld violations %lld\n", plans, cuts, forms[0], forms[1],
         forms[2], violations);
  return violations ? 1 : (cuts > 0 && forms[0] > 0 && forms[1] > 0 && forms[2] > 0 ? 0 : 2);
}
