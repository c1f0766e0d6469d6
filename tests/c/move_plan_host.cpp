// Host walk of rua_move_plan.h (tests/test_move_plan.py builds it with -fsanitize=address,undefined): the header is plain
// C++, so the row mover's whole decision can be walked over sizes no test could allocate — every pair of layout kinds,
// row widths from 1 byte to past the span kernel's limit, n_rows and n_tiles on both sides of every span threshold and
// of the 2^31 - 1 grid limit, every tile code the host can ask for and some it cannot, every flag that changes the
// geometry, payload addresses of every alignment.  A violation is a plan the launcher of rua_move.hip could not launch
// as it stands, or one that breaks what a kernel relies on: the invariants are spelled out in check() below.
#include <stdint.h>
#include <stdio.h>
#include "rua_move_plan.h"

using namespace rua;

static long long violations = 0, plans = 0, forms[MOVE_ROWS + 1], errors[4], setitems = 0;

static void fail(const char* what, const rua_layout& D, const rua_layout& S, int64_t rb, int flags, const MoveRowsPlan& P) {
  if (++violations <= 20)
    printf("VIOLATION %s: dst kind=%d n_rows=%lld code=%#x n_tiles=%lld src kind=%d row_bytes=%lld flags=%#x form=%d vec=%d grid=%u "
           "per_xcd=%lld tile_rows=%d\n", what, D.kind, (long long)D.n_rows, (unsigned)D.tile_t_log2, (long long)D.n_tiles, S.kind,
           (long long)rb, (unsigned)flags, P.form, P.vec, P.grid, (long long)P.per_xcd, P.tile_rows);
}

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// the instantiations rua_move.hip has, restated by hand
static bool lds_tile_kernel(int vec, int ttl, int trl) {
  const bool lane = vec == 16 || vec == 8 || vec == 4 || vec == 2 || vec == 1;
  return (lane && trl == 4 && ttl >= 4 && ttl <= 6) || (vec == 2 && ttl == 7 && trl == 6) || (vec == 1 && ttl == 7 && trl == 7);
}
static bool vec_tile_kernel(int vec, int ttl, int trl, bool to_pack) {
  return (vec == 16 && ttl == 6 && trl == 4 && to_pack) || (vec == 8 && ((ttl == 7 && trl == 4) || (ttl == 6 && trl == 5))) ||
         (vec == 4 && ((ttl == 7 && trl == 5) || (ttl == 6 && trl == 6)));
}

static void check(const rua_layout& D, const rua_layout& S, int tmap, int64_t targ, uintptr_t da, uintptr_t sa, int64_t rb,
                  int64_t pad_row, int flags) {
  const MoveRowsPlan P = plan_move_rows(&D, &S, tmap, targ, da, sa, rb, pad_row, flags);
  ++plans;
  auto bad = [&](const char* what) { fail(what, D, S, rb, flags, P); };
  if (P.err) {
    if (P.err != RUA_EINVAL && P.err != RUA_ERANGE) bad("an error code the entry does not document");
    if (P.form != MOVE_NONE) bad("an error with a form");
    ++errors[-P.err];
    return;
  }
  if (P.form < MOVE_NONE || P.form > MOVE_ROWS) { bad("no such form"); return; }
  ++forms[P.form];
  if (P.form == MOVE_NONE) {
    if (D.n_rows != 0 && rb != 0) bad("nothing to launch for a destination with rows");
    return;
  }
  if (P.grid < 1 || P.grid > 0x7fffffffu) bad("grid outside 1 .. 2^31 - 1");
  if (P.block != RUA_BLOCK && !(P.form == MOVE_ROWS && P.block == MOVE_BLOCK)) bad("block");
  if (P.lds < 0 || P.lds > (48 << 10)) bad("LDS bytes beyond 48 KiB");
  if (!(P.R == 1 || P.R == 2 || P.R == 4 || P.R == 8) || (P.R > 1 && P.R * rb != 128) || P.phase < 0 || P.phase >= P.R) bad("R / phase");
  if (P.R > 1 && (P.form != MOVE_TILES_LDS || P.to_pack)) bad("line-aligned windows outside P.cat's staged tiles");
  // the tiles the launch covers
  const rua_layout& Pk = P.to_pack ? D : S;
  int64_t tiles = -1;
  switch (P.form) {
    case MOVE_TILES_LDS:
      tiles = Pk.n_tiles;
      if (!lds_tile_kernel(P.vec, P.ttl, P.trl)) bad("no pack_tile_lds_kernel for (vec, ttl, trl)");
      if (P.lpr * P.vec != rb || P.lds != ((1 << (P.ttl + P.trl)) + (1 << P.trl)) * rb) bad("staged tile: lanes or LDS bytes");
      break;
    case MOVE_TILES_VEC:
      tiles = Pk.n_tiles;
      if (!vec_tile_kernel(P.vec, P.ttl, P.trl, P.to_pack) || rb != P.vec) bad("no pack_tile_vec_kernel for (vec, ttl, trl)");
      break;
    case MOVE_ROLL_STEPS:
      tiles = D.n_tiles;
      if (P.trl != ((D.tile_t_log2 >> 8) & 0xff) || tmap != RUA_T_ROLL) bad("roll steps");
      break;
    case MOVE_SEQ_COPY: {
      if (P.spw != 1 && P.spw != 2 && P.spw != 4 && P.spw != SEQ_PER_WAVE) bad("sequences per wave");
      if ((__int128)P.grid * RUA_WAVES_PER_BLOCK * P.spw < D.B) bad("the waves do not cover the sequences");
      if (P.span || P.per_xcd) bad("a span for workgroups of waves");
      break;
    }
    case MOVE_NARROW:
      tiles = (D.n_rows + RUA_BLOCK * NARROW_CH - 1) / (RUA_BLOCK * NARROW_CH);
      if (rb != P.vec) bad("lane-per-row kernel for a row of more than one vector");
      break;
    case MOVE_ROLL_TILES:
      tiles = D.n_tiles;
      if (P.vec != 16 || P.ttl < 4 || P.ttl > 6 || P.lpr * 16 != rb) bad("no pack_roll_tile_kernel for (vec, ttl)");
      break;
    case MOVE_SPAN: {
      const int step = (rb & 15) == 0 ? 1 : (rb & 7) ? 4 : 2;
      tiles = (D.n_rows + P.tile_rows - 1) / P.tile_rows;
      if (P.tile_rows < 1 || P.tile_rows > RUA_BLOCK || P.tile_rows * rb > SPAN_TILE_BYTES || P.tile_rows % step) bad("span tile rows");
      if (rb > 0x7fffffff || ((da | sa) & 15) || (rb & 3)) bad("span kernel: row bytes or alignment");
      break;
    }
    case MOVE_ROWS:
      tiles = (D.n_rows + (int64_t)P.tile_rows * P.rpt - 1) / ((int64_t)P.tile_rows * P.rpt);
      if (!pow2(P.tile_rows) || P.tile_rows < 4 || P.tile_rows > 256 || P.tile_rows > MOVE_BLOCK) bad("tile rows");
      if ((P.vec != 16 || P.tail8) && P.tile_rows != 16 && P.tile_rows != 64 && P.tile_rows != MOVE_TILE) bad("tile rows of a narrow lane");
      if (P.rpt != 1 && !(P.rpt == NARROW_RPT && P.vec == 16 && !P.scatter && !P.tail8 && P.tile_rows == MOVE_TILE && !P.span)) bad("RPT variant");
      if (P.lpr != (rb + P.vec - 1) / P.vec || P.cpr * RUA_WAVE < P.lpr || (P.cpr - 1) * RUA_WAVE >= P.lpr) bad("lanes per row");
      if (P.lp_log2 < 0 || P.lp_log2 > 6 || ((1 << P.lp_log2) < P.lpr && P.lp_log2 < 6) || (P.lp_log2 > 0 && (1 << (P.lp_log2 - 1)) >= P.lpr)) bad("lp_log2");
      if (P.tail8 ? (rb & 15) != 8 || ((da | sa) & 7) : (rb % P.vec || ((da | sa) % P.vec))) bad("lane width against row bytes / addresses");
      break;
  }
  if (!pow2(P.vec) || P.vec > 16) bad("vec");
  if (tiles >= 0) {
    if (P.span ? (P.grid != 8 * P.per_xcd || P.per_xcd * 8 < tiles || (P.per_xcd - 1) * 8 >= tiles) : (P.per_xcd != 0 || P.grid != tiles))
      bad("XCD-span geometry");
    if ((flags & RUA_MOVE_XCD_SPAN_OFF) && P.span) bad("a span against RUA_MOVE_XCD_SPAN_OFF");
  }
}

int main() {
  static int64_t mem[8];                             // pointers the plan never follows
  const int64_t rows[] = {0, 1, 3, 255, 256, 257, 2047, 2048 * 4, (2048 << 8) - 1, 2048 << 8, (1LL << 19) * 16 - 1, (1LL << 19) * 16,
                          (1LL << 31) - 1, 1LL << 31, ((1LL << 31) - 8) * 4, ((1LL << 31) - 1) * 4 + 1, 1LL << 35, (1LL << 41) + 1, 1LL << 44};
  const int64_t tile_counts[] = {1, 2047, 2048, (1 << 18) - 1, 1 << 18, (1 << 19) - 1, 1 << 19, (1LL << 31) - 8, (1LL << 31) - 7, (1LL << 31) - 1, 1LL << 31};
  const int64_t widths[] = {1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 68, 72, 100, 128, 136, 640, 656, 1000, 1024, 1032, 1040,
                            2000, 2160, 4100, 8176, 8192, 8208, 16384, 16400, 1 << 20};
  const int codes[] = {0, 4 | 4 << 8, 5 | 4 << 8, 6 | 4 << 8, 6 | 5 << 8, 6 | 6 << 8, 7 | 4 << 8, 7 | 5 << 8, 7 | 6 << 8, 7 | 7 << 8,
                       6 | 4 << 8 | 8 << 16, 5 | 4 << 8 | 4 << 16, 4 | 4 << 8 | 2 << 16, 6 | 4 << 8 | 1 << 24, 7 | 5 << 8 | 1 << 24,
                       10 << 8 | 1 << 25, 14 << 8 | 1 << 25, 1 << 25, 3 | 4 << 8, 8 | 4 << 8, 6 | 8 << 8, 6 | 4 << 8 | 3 << 16, 7 | 7 << 8 | 8 << 16};
  const int flag_sets[] = {0, RUA_MOVE_SCATTER, RUA_MOVE_NT_ON, RUA_MOVE_XCD_SPAN_ON, RUA_MOVE_XCD_SPAN_OFF, RUA_MOVE_XCD_SPAN_ON | RUA_MOVE_XCD_SPAN_OFF,
                           RUA_MOVE_NO_TAIL8, RUA_MOVE_NO_NARROW, RUA_MOVE_TILE_LOG2(2), RUA_MOVE_TILE_LOG2(8), RUA_MOVE_TILE_LOG2(5) | RUA_MOVE_SCATTER, 4096};
  const uintptr_t bases[] = {0x10000, 0x10010, 0x10020, 0x10040, 0x10008, 0x10004, 0x10002, 0x10001};
  const int kinds[] = {RUA_CAT, RUA_LEFT, RUA_PACK, RUA_RIGHT, RUA_LIST};
  for (int dk : kinds)
    for (int sk : kinds)
      for (int64_t n : rows)
        for (int64_t rb : widths)
          for (int code : codes)
            for (int64_t nt : tile_counts) {
              if (code != codes[1] && nt != tile_counts[0] && nt != tile_counts[9] && (dk != RUA_PACK && sk != RUA_PACK)) continue;   // (tile counts only matter with a table)
              rua_layout S = {};
              S.kind = sk; S.n_rows = n > 0 ? n : 1; S.B = 5000; S.T_phys = S.T_log = n / 4096 > 0 ? n / 4096 : 1; S.T = 40;
              S.lens = mem; S.off = mem + 1; S.boff = mem + 2; S.sorted = mem + 3; S.bsz = mem + 4; S.tile_start = mem + 5; S.tptr = mem + 6;
              S.tile_t_log2 = code; S.n_tiles = nt; S.n_tchunks = S.T;
              rua_layout D = S;
              D.kind = dk; D.n_rows = n;
              for (int fl : flag_sets)
                for (int tmap = RUA_T_SHIFT; tmap <= RUA_T_REV_S; ++tmap) {
                  const uintptr_t da = bases[(plans / 3) % 8], sa = bases[(plans / 7) % 8] + 0x100000;
                  check(D, S, tmap, tmap == RUA_T_ROLL ? 3 : 0, da, sa, rb, -1, fl);
                }
            }
  // the validation's own answers
  {
    rua_layout L = {};
    L.kind = RUA_LEFT; L.n_rows = 8; L.B = 1; L.T_phys = 8;
    const MoveRowsPlan a = plan_move_rows(nullptr, &L, 0, 0, 16, 16, 16, -1, 0), b = plan_move_rows(&L, &L, 5, 0, 16, 16, 16, -1, 0),
                       c = plan_move_rows(&L, &L, 0, 0, 0, 16, 16, -1, 0), d = plan_move_rows(&L, &L, 0, 0, 16, 16, 16, 8, 0),
                       e = plan_move_rows(&L, &L, 0, 0, 16, 16, 0, -1, 0);
    if (a.err != RUA_EINVAL || b.err != RUA_EINVAL || c.err != RUA_EINVAL || d.err != RUA_EINVAL || e.err != 0 || e.form != MOVE_NONE) {
      ++violations;
      printf("VIOLATION the entry checks: %d %d %d %d %d\n", a.err, b.err, c.err, d.err, e.err);
    }
  }
  // rua_setitem_backward's plan: the same lanes helper, one wave per 64 entries
  for (int64_t n : rows)
    for (int64_t rb : widths)
      for (uintptr_t base : bases) {
        if (n == 0) continue;
        const SetitemBackwardPlan P = plan_setitem_backward(n, n, rb, base, 0);
        ++setitems;
        const bool fits = (n + RUA_BLOCK - 1) / RUA_BLOCK <= 0x7fffffffLL;
        if ((P.err == 0) != fits || (P.err && P.err != RUA_ERANGE)) { ++violations; printf("VIOLATION setitem range n=%lld\n", (long long)n); continue; }
        if (P.err) continue;
        if ((int64_t)P.grid * RUA_BLOCK < n || P.lpr != (rb + P.vec - 1) / P.vec || P.cpr * RUA_WAVE < P.lpr ||
            (P.tail8 ? P.vec != 16 || (rb & 15) != 8 || (base & 7) : rb % P.vec || base % P.vec) || P.lp_log2 != lanes_log2(P.lpr)) {
          ++violations;
          printf("VIOLATION setitem plan n=%lld rb=%lld base=%#llx vec=%d\n", (long long)n, (long long)rb, (unsigned long long)base, P.vec);
        }
      }
  printf("plans %lld setitem %lld errors EINVAL %lld ERANGE %lld forms", plans, setitems, errors[1], errors[3]);
  for (int f = 0; f <= MOVE_ROWS; ++f) printf(" %lld", forms[f]);
  for (int f = 0; f <= MOVE_ROWS; ++f)
    if (forms[f] == 0) { ++violations; printf("\nVIOLATION the walk never reached form %d", f); }
  if (errors[1] == 0 || errors[3] == 0) { ++violations; printf("\nVIOLATION the walk never saw an error code"); }
  printf("\nviolations %lld\n", violations);
  return violations ? 1 : 0;
}
