// Host walk of rua_sort_plan.h (tests/test_sort_surface.py builds it with -fsanitize=address,undefined): the header is
// plain C++, so the arithmetic the merge kernel runs per element — passes, run pairing, destination, buffer parity —
// is run here on the host, with a block length passed in small (4 and 8) as well as the real one so that many passes
// are cheap, on keys from {0, 1, 2} so that stability is exercised, and compared with std::stable_sort on (key,
// position).  The plan itself is walked over sizes no test could allocate: every grid fits a launch, the workspace is
// the documented formula and nothing overflows.  A violation is a wrong order or a plan that could not be launched as
// computed.
#include <algorithm>
#include <vector>
#include "rua_sort_plan.h"
#include "plan_walk.h"

using namespace rua;

struct elem { uint32_t key, pos; };
static bool less(const elem& a, const elem& b) { return a.key < b.key || (a.key == b.key && a.pos < b.pos); }

static long long sorts = 0, merges = 0, odd_runs = 0, plans = 0, merge_plans = 0;

// what the block kernel and the merge launches do to ONE sequence, with the header's functions
static void walk_sort(int64_t len, int blk_log2, uint32_t seed, bool descending) {
  ++sorts;
  std::vector<elem> in(len);
  for (int64_t i = 0; i < len; ++i) {
    seed = seed * 1664525u + 1013904223u;
    const uint32_t key = (seed >> 24) % 3;
    in[i] = {descending ? ~key : key, (uint32_t)i};
  }
  std::vector<elem> want = in;
  std::stable_sort(want.begin(), want.end(), [](const elem& a, const elem& b) { return a.key < b.key; });
  const int64_t blk = (int64_t)1 << blk_log2;
  std::vector<elem> buf[2] = {in, std::vector<elem>(len)}, out(len, elem{7, 0xffffffffu});
  for (int64_t t0 = 0; t0 < len; t0 += blk) std::sort(buf[0].begin() + t0, buf[0].begin() + std::min(len, t0 + blk), less);
  const int passes = sort_passes(len, blk_log2);
  if (len <= blk && passes != 0) { printf("VIOLATION a sequence of one block needs %d passes (len %lld)\n", passes, (long long)len); ++violations; }
  if (len > blk && ((blk << passes) < len || (blk << (passes - 1)) >= len)) {
    printf("VIOLATION %d passes do not cover len %lld with blocks of %lld exactly\n", passes, (long long)len, (long long)blk);
    ++violations;
  }
  if (passes == 0) out = buf[0];
  for (int pass = 0; pass < passes; ++pass) {
    ++merges;
    const std::vector<elem>& src = buf[sort_src_buffer(pass)];
    std::vector<elem>& dst = pass == passes - 1 ? out : buf[1 - sort_src_buffer(pass)];
    std::vector<char> hit(len, 0);
    for (int64_t t = 0; t < len; ++t) {
      int64_t base, mid, end;
      sort_pairing(t, len, blk_log2 + pass, base, mid, end);
      if (base > t || t >= end || mid < base || mid > end || end > len) {
        if (++violations <= 20) printf("VIOLATION pairing of t=%lld len=%lld pass=%d\n", (long long)t, (long long)len, pass);
        return;
      }
      int64_t dest = t;
      if (mid < end) {
        const elem me = src[t];
        int64_t lo, hi;
        if (t < mid) {
          lo = mid; hi = end;
          while (lo < hi) { const int64_t m = lo + ((hi - lo) >> 1); if (less(src[m], me)) lo = m + 1; else hi = m; }
          dest = sort_dest(base, mid, t, lo - mid);
        } else {
          lo = base; hi = mid;
          while (lo < hi) { const int64_t m = lo + ((hi - lo) >> 1); if (less(me, src[m])) hi = m; else lo = m + 1; }
          dest = sort_dest(base, mid, t, lo - base);
        }
      } else if (t == base) {
        ++odd_runs;
      }
      if (dest < base || dest >= end || hit[dest]) {
        if (++violations <= 20) printf("VIOLATION destination %lld of t=%lld len=%lld pass=%d (taken or outside its pair)\n", (long long)dest, (long long)t, (long long)len, pass);
        return;
      }
      hit[dest] = 1;
      dst[dest] = src[t];
    }
  }
  for (int64_t i = 0; i < len; ++i)
    if (out[i].key != want[i].key || out[i].pos != want[i].pos) {
      if (++violations <= 20) printf("VIOLATION order: len=%lld blk=%lld rank %lld is (%u, %u), std::stable_sort says (%u, %u)\n", (long long)len, (long long)blk, (long long)i, out[i].key, out[i].pos, want[i].key, want[i].pos);
      return;
    }
}

static void walk_plan(const rua_layout& L, int64_t H, int es) {
  if (seg_check_entry(&L, H, es) != 0) { fail("entry checks refuse a sound call", L, H); return; }
  const sort_plan p = sort_make_plan(L, H, es);
  ++plans;
  const int64_t bound = sm_len_bound(L);
  if (L.B == 0 || H == 0) { if (p.form >= 0 || p.grid || p.ws_bytes) fail("a plan of nothing", L, H); return; }
  if (bound > SORT_MAX_LEN) { if (p.form >= 0) fail("a bound of 2^31 or more got a plan", L, H); return; }
  if (p.form < 0) {                                            // refused: something must not fit
    const __int128 cols = (__int128)L.B * H;
    const __int128 elems = (__int128)L.n_rows * H;
    if (cols <= 0x7fffffffLL && elems < ((__int128)1 << 31) && bound <= SEG_BLOCK_TOK) fail("a plan refused that fits", L, H);
    return;
  }
  if (p.grid <= 0 || p.grid > 0x7fffffffLL || p.merge_grid < 0 || p.merge_grid > 0x7fffffffLL || p.ws_bytes < 0)
    fail("a grid or workspace beyond what a launch takes", L, H);
  if ((p.form == SORT_LANES) != (bound <= SORT_LANES_MAX_LEN)) fail("the lanes form outside its bound", L, H);
  if (p.form == SORT_LANES && (p.G < bound || p.G < 8 || p.G > 64 || (p.G & (p.G - 1)) ||
                               (__int128)p.grid * SEG_WAVES_PER_BLOCK * (64 / p.G) < (__int128)L.B * H))
    fail("the lanes geometry does not hold every (sequence, column)", L, H);
  if ((p.form == SORT_MERGE) != (bound > SEG_BLOCK_TOK)) fail("the merge form outside its bound", L, H);
  if (p.form != SORT_MERGE) { if (p.ws_bytes || p.passes) fail("a workspace nobody needs", L, H); return; }
  ++merge_plans;
  if (((int64_t)SEG_BLOCK_TOK << p.passes) < bound || ((int64_t)SEG_BLOCK_TOK << (p.passes - 1)) >= bound)
    fail("the passes do not cover the bound exactly", L, H);
  const __int128 elems = (__int128)L.n_rows * H;
  const __int128 want = 256 + 2 * ((elems * 8 + 255) / 256 * 256) + (es == 8 ? 2 * ((elems * 4 + 255) / 256 * 256) : 0);
  if ((__int128)p.ws_bytes != want) fail("ws_bytes is not the documented formula", L, H);
  if ((__int128)p.merge_grid * 256 < elems) fail("the merge grid does not cover every element", L, H);
  if (L.kind != RUA_CAT && (__int128)p.maxblk * SEG_BLOCK_TOK < bound) fail("the blocks do not cover the bound", L, H);
}

int main(int argc, char** argv) {
  const int real_log2 = SORT_BLOCK_LOG2;
  const int blk_log2s[] = {2, 3, real_log2};
  for (int bl : blk_log2s) {
    const int64_t blk = (int64_t)1 << bl;
    const int64_t prime = bl == real_log2 ? 1000003 : 10007;
    const int64_t lens[] = {0, 1, 2, blk - 1, blk, blk + 1, 2 * blk - 1, 2 * blk, 2 * blk + 1, 3 * blk, 5 * blk + 3, 7 * blk + 1,
                            8 * blk, prime};
    uint32_t seed = 1;
    for (int64_t len : lens)
      for (int desc = 0; desc < 2; ++desc) walk_sort(len, bl, seed += 77, desc != 0);
  }
  if (argc > 1) printf("(arguments are ignored: %s)\n", argv[1]);
  if (seg_check_entry(nullptr, 1, 4) != RUA_EINVAL) { printf("VIOLATION a null layout passes\n"); ++violations; }
  const int64_t Hs[] = {0, 1, 3, 8, 33, 512, 1LL << 20, 1LL << 33};
  for_each_bound_layout([&](const rua_layout& L) {
    for (int64_t H : Hs)
      for (int es : {2, 4, 8}) {
        if (L.n_rows > 0 && H > 0 && (double)L.n_rows * (double)H * 24 >= 9.0e18) continue;      // seg_too_large refuses first
        walk_plan(L, H, es);
      }
  });
  printf("sorts %lld merges %lld odd runs %lld plans %lld merge plans %lld violations %lld\n", sorts, merges, odd_runs, plans,
         merge_plans, violations);
  return violations ? 1 : (merges > 0 && odd_runs > 0 && merge_plans > 0 ? 0 : 2);
}
