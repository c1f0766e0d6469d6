// Host walk of rua_compress_plan.h (tests/test_compress_surface.py builds it with -fsanitize=address,undefined): the
// header is plain C++, so what compress adds to the family's offsets scan can be walked over sizes no test could
// allocate — B from 0 to 2^40, bounds up to 2^36, every layout kind: the length it refuses, and that the workspace
// rua_compress_ws_bytes reports is one int32 per (sequence, block).  The scan plan itself — forms, grid, cut rule — is
// walked by seg_plan_host.cpp.
#include "rua_compress_plan.h"
#include "plan_walk.h"

using namespace rua;

static long long plans = 0, cuts = 0;

static void walk(const rua_layout& L) {
  if (seg_check_entry(&L, 1, 1) != 0) { fail("entry checks refuse a sound call", L); return; }
  const int64_t bound = sm_len_bound(L);
  if (cp_too_long(L) != (bound >= (1LL << 31))) fail("cp_too_long is not bound >= 2^31", L);
  const seg_scan_plan p = seg_make_scan_plan(L, CP_WS_ELEM_BYTES);
  ++plans;
  if (p.form != SEG_SCAN_CUT) return;
  ++cuts;
  if (p.ws_bytes != L.B * p.maxblk * 4) fail("ws_bytes is not one int32 per (sequence, block)", L);
}

int main() {
  if (seg_check_entry(nullptr, 1, 1) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  if (CP_WS_ELEM_BYTES != 4) { printf("VIOLATION the workspace element of compress is not an int32\n"); ++violations; }
  for_each_bound_layout(walk);
  printf("plans %lld cuts %lld violations %lld\n", plans, cuts, violations);
  return violations ? 1 : (cuts > 0 ? 0 : 2);
}
