// What the host walks of the plan headers (seg_plan_host.cpp, compress_plan_host.cpp, repeat_plan_host.cpp) share: the
// violation count and report, and a layout of a given kind, B and length bound.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "rua_seg_plan.h"

static long long violations = 0;

static void fail(const char* what, const rua_layout& L, int64_t rb = 0) {
  if (++violations <= 20)
    printf("VIOLATION %s: kind=%d B=%lld n_rows=%lld T_phys=%lld T_log=%lld T=%lld row_bytes=%lld\n", what, L.kind,
           (long long)L.B, (long long)L.n_rows, (long long)L.T_phys, (long long)L.T_log, (long long)L.T, (long long)rb);
}

// a layout whose length bound (sm_len_bound) is `bound`; a CAT with T_log holds more rows than its bound
static rua_layout bound_layout(int kind, int64_t B, int64_t bound, int with_tlog) {
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

// the family's cut rule over `units` workgroups of the layout's sequences
static bool cut_rule(const rua_layout& L, __int128 units) {
  const int64_t bound = rua::sm_len_bound(L);
  return units < rua::SEG_CUT_MAX_UNITS && bound >= rua::SEG_CUT_MIN_LEN &&
         (bound + rua::SEG_BLOCK_TOK - 1) / rua::SEG_BLOCK_TOK <= rua::SEG_CUT_MAX_BLOCKS;
}

// the grid of (kind, B, bound) the walks of the offsets scan and of its operators take
static const int64_t WALK_BS[] = {0, 1, 2, 3, 7, 8, 9, 127, 128, 1023, 1024, 1025, 65536, (1LL << 31) - 8, (1LL << 31) - 1,
                                  1LL << 31, (1LL << 34) - 1, 1LL << 34, 1LL << 40};
static const int64_t WALK_BOUNDS[] = {0, 1, 31, 32, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 1LL << 20,
                                      (1LL << 31) - 1, 1LL << 31, (1LL << 31) + 1, 1LL << 36};

template <typename F> static void for_each_bound_layout(F f) {
  const int kinds[4] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT};
  for (int kind : kinds)
    for (int64_t B : WALK_BS)
      for (int64_t bound : WALK_BOUNDS)
        for (int with_tlog = 0; with_tlog < 2; ++with_tlog) {
          if (kind != RUA_CAT && with_tlog) continue;
          if (kind != RUA_CAT && B > 0 && bound > (1LL << 62) / B) continue;      // B * T rows of storage fit int64
          f(bound_layout(kind, B, bound, with_tlog));
        }
}
