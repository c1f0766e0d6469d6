// Host walk of rua_repeat_plan.h (tests/test_repeat_surface.py builds it with -fsanitize=address,undefined): the header
// is plain C++, so what repeat_interleave adds to the family's offsets scan can be walked over sizes no test could
// allocate — bounds up to 2^36, B from 0 to 2^40, every layout kind, row widths from 1 byte to 2^40: the grid of the
// move / run sum, and that the workspace rua_repeat_ws_bytes reports is one int64 per (sequence, block).  The scan plan
// itself — forms, grid, cut rule — is walked by seg_plan_host.cpp.  A violation is a plan the launcher could not launch
// as computed.
#include "rua_repeat_plan.h"
#include "plan_walk.h"

using namespace rua;

static long long plans = 0, cuts = 0, walks = 0, walk_cuts = 0;

static void walk_ws(const rua_layout& L) {
  if (seg_check_entry(&L, 1, 1) != 0) { fail("entry checks refuse a sound call", L); return; }
  const seg_scan_plan p = seg_make_scan_plan(L, RP_WS_ELEM_BYTES);
  ++plans;
  if (p.form != SEG_SCAN_CUT) return;
  ++cuts;
  if (p.ws_bytes != L.B * p.maxblk * 8) fail("ws_bytes is not one int64 per (sequence, block)", L);
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
  const int64_t widths[] = {0, 1, 2, 3, 8, 10, 16, 17, 128, 129, 1000, 1024, 1LL << 20, (1LL << 38) - 1, 1LL << 38, 1LL << 40};
  if (seg_check_entry(nullptr, 1, 1) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  if (RP_WS_ELEM_BYTES != 8) { printf("VIOLATION the workspace element of repeat is not an int64\n"); ++violations; }
  for_each_bound_layout([&](const rua_layout& L) {
    walk_ws(L);
    for (int64_t rb : widths) walk_move(L, rb);
  });
  printf("plans %lld cuts %lld walks %lld walk cuts %lld violations %lld\n", plans, cuts, walks, walk_cuts, violations);
  return violations ? 1 : (cuts > 0 && walk_cuts > 0 ? 0 : 2);
}
