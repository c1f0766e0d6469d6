// Host walk of rua_pack_sums_plan.h (tests/test_pack_sums_surface.py builds it with -fsanitize=address,undefined): the
// header is plain C++, so what the entry points of pack(keep_sums=...) refuse, and the grid of the adjoint kernel, can be
// walked over sizes no test could allocate.  A violation: a refusal with another code than rua.h documents, a sound
// call refused, a grid that does not cover every (sequence, column chunk) or exceeds what a launch takes.
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include "rua_pack_sums_plan.h"

using namespace rua;

static long long violations = 0, plans = 0;
static void fail(const char* what, long long a, long long b, long long c) {
  if (++violations <= 20) printf("VIOLATION %s: %lld %lld %lld\n", what, a, b, c);
}

int main() {
  static int64_t dummy;
  // ---- the layout checks
  for (int skind : {RUA_CAT, RUA_LEFT, RUA_RIGHT, RUA_PACK, RUA_LIST})
    for (int dtype = RUA_F32 - 1; dtype <= RUA_U8 + 1; ++dtype)
      for (int64_t B : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)65536, (int64_t)1 << 40})
        for (int64_t dB : {(int64_t)0, (int64_t)1})
          for (int with_boff = 0; with_boff < 2; ++with_boff) {
            rua_layout S = {}, Pk = {};
            S.kind = skind; S.B = B; S.len_add = 1;
            Pk.kind = RUA_PACK; Pk.B = B + dB; Pk.T = 3; Pk.boff = with_boff ? &dummy : nullptr;
            const int rc = pack_sums_check(&S, &Pk, 64, dtype);
            const bool sound = (skind == RUA_CAT || skind == RUA_LEFT || skind == RUA_RIGHT) && B >= 0 && dB == 0 &&
                               with_boff && (dtype == RUA_F32 || dtype == RUA_BF16 || dtype == RUA_F16);
            if (sound != (rc == 0) || (rc != 0 && rc != RUA_EINVAL)) fail("layout check", skind, dtype, B);
          }
  {
    rua_layout S = {}, Pk = {};
    S.kind = RUA_CAT; Pk.kind = RUA_PACK;
    if (pack_sums_check(nullptr, &Pk, 8, RUA_F32) != RUA_EINVAL || pack_sums_check(&S, nullptr, 8, RUA_F32) != RUA_EINVAL ||
        pack_sums_check(&S, &Pk, -1, RUA_F32) != RUA_EINVAL)
      fail("null / negative", 0, 0, 0);
    S.lens = &dummy;                                   // CAT with lengths but no offsets
    if (pack_sums_check(&S, &Pk, 8, RUA_F32) != RUA_EINVAL) fail("CAT lens without off", 0, 0, 0);
  }
  // ---- the adjoint's grid
  for (int esize : {2, 4})
    for (int sh = 0; sh <= 40; ++sh)
      for (int64_t dB : {(int64_t)-1, (int64_t)0, (int64_t)1})
        for (int hs = 0; hs <= 24; ++hs)
          for (int64_t dH : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3})
            for (uintptr_t ptrs : {(uintptr_t)0x1000, (uintptr_t)0x1008, (uintptr_t)0x1004}) {
              const int64_t B = ((int64_t)1 << sh) + dB, H = ((int64_t)1 << hs) + dH;
              if (B < 0 || H <= 0) continue;
              const PackSumsBackwardPlan P = plan_pack_sums_backward(B, H, esize, ptrs);
              ++plans;
              const int epl = 16 / esize;
              const bool aligned = H % epl == 0 && ptrs % 16 == 0;
              if (!aligned) { if (P.err != RUA_EALIGN) fail("misaligned call not refused", B, H, esize); continue; }
              const int64_t lpr = H / epl, chunks = (lpr + 63) / 64;
              const bool fits = (__int128)B * chunks <= 0x7fffffffLL;
              if (!fits) { if (P.err != RUA_ERANGE) fail("a grid beyond a launch not refused", B, H, esize); continue; }
              if (P.err) { fail("a sound call refused", B, H, esize); continue; }
              if (P.n_chunks != chunks || (int64_t)P.grid != B * chunks) fail("grid does not cover the units", B, H, esize);
              if (P.lp_log2 < 0 || P.lp_log2 > 6 || ((int64_t)1 << P.lp_log2) < (lpr < 64 ? lpr : 64))
                fail("lanes per row", B, H, esize);
              if (P.n_chunks * 64 * epl < H) fail("chunks do not cover the row", B, H, esize);
            }
  printf("pack_sums plan walk: %lld plans, violations %lld\n", plans, violations);
  return violations ? 1 : 0;
}
