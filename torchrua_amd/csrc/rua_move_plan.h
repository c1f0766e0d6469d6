// rua_move_plan.h — what the row mover decides BEFORE its first HIP call, as plain host C++ (no HIP header): validation,
// the lane width, which kernel family takes the call and every launch parameter that is not a pointer or a layout.
// plan_move_rows / plan_setitem_backward are the one place these live: rua_move.hip launches what a plan says, the
// dispatch trace and rua_debug_move_plan print it, and a machine without a GPU can ask for it.
#pragma once
#include "rua.h"
#include "rua_wave.h"

namespace rua {

#ifndef RUA_MOVE_BLOCK        // developer knob for A/B builds (scripts/pack_ab.py)
#define RUA_MOVE_BLOCK 256
#endif
constexpr int MOVE_BLOCK = RUA_MOVE_BLOCK;          // threads per workgroup of the generic mover
constexpr int MOVE_TILE = MOVE_BLOCK;               // one lane per row in phase 1
constexpr int64_t MOVE_TILE_BYTES = 16 << 10;       // destination bytes one workgroup takes (rows: a power of two, 4..256)
constexpr int64_t MOVE_SPAN_MIN_TILES = 2048;       // launches at least this large give every XCD one contiguous span ...
constexpr int64_t MOVE_SPAN_MIN_TILES_DENSE = 1 << 19;   // ... when the destination is padded (two thirds of a pad's
// traffic is stores, and a span per XCD is worth 11-13 % to them at every size measured); a gather into a dense
// destination (C / P) only draws level from ~8 GB up and LOSES 2-5 % below (cfg2's 0.5 GB: 183 -> 173 us with plain
// blockIdx order; gpurun_out/r4j/midsize_ab.txt, r4k/span_ab.txt -> profiles/r04_span_ab.txt)
// The (rank x time) tiles of narrow rows have their own rule (profiles/r04_narrow_span_ab.txt): neighbouring tiles share
// the 128-byte lines their 512-byte runs straddle, and only a span keeps the two on one XCD's L2.  Pack and the roll
// tiles gain at every size (16-byte rows: 3.0 -> 4.5 and 3.7 -> 4.4-4.6 TB/s; 32: 3.7 -> 4.9 and 4.5 -> 5.0); P.cat,
// whose stores are whole 1-KiB runs either way, gains from ~8 GB (4-9 %) and loses 2-8 % at 1-3 GB.
constexpr int64_t TILE_SPAN_MIN_TILES_FROM_PACK = 1 << 18;
constexpr int64_t TILE_MAX_ROW_BYTES = 64;       // rows up to this take the tile kernel (pack_tile_lds_kernel)
constexpr int TILE_SHIFT_MAX = 8;                // R <= 8: rows of 16 bytes (line-aligned runs: TileTables, rua_move.hip)
constexpr int TILE_FULL_GRID = 1 << 24;   // rua_layout::tile_t_log2 bit 24: tiles cover the whole (sequence x step) grid
constexpr int TILE_STEP_ROWS = 1 << 25;   // ... bit 25: tiles of ONE time step x (1 << bits 8-15) ranks (pack_roll_steps_kernel)
constexpr int SPAN_TILE_BYTES = 16 << 10;        // LDS of move_rows_span_kernel: the destination bytes of one tile
constexpr int SEQ_PER_WAVE = 8;        // seq_copy_kernel at narrow rows; rows from 256 bytes up (odd widths) give a wave ONE sequence
constexpr int NARROW_RPT = 4;          // rows per lane of the same-PackedSequence variant of move_rows_kernel
constexpr int NARROW_CH = 8;           // rows in flight per lane of move_rows_narrow_kernel
constexpr int64_t COPY_ROW_BYTES = 1024;     // stream_copy sees its bytes as rows of this size
constexpr int MOVE_SPAN_FLAGS = RUA_MOVE_XCD_SPAN_ON | RUA_MOVE_XCD_SPAN_OFF;

inline int check_layout(const rua_layout* L, bool is_dst) {
  if (!L || L->B < 0 || L->n_rows < 0) return RUA_EINVAL;
  switch (L->kind) {
    case RUA_CAT: return L->lens && !L->off ? RUA_EINVAL : 0;
    case RUA_LEFT:
    case RUA_RIGHT: return L->T_phys >= 0 ? 0 : RUA_EINVAL;
    case RUA_PACK: return L->T > 0 && !L->boff ? RUA_EINVAL : 0;
    case RUA_LIST: return is_dst && (L->n_rows == 0 || L->tptr) ? 0 : RUA_EINVAL;     // (a destination only)
  }
  return RUA_EINVAL;
}

// rua_layout::tile_t_log2, decoded ONCE.  A zero ttl / trl field = 4 (a caller of ABI <= 3, 16 x 16 tiles) — except trl
// under step_rows (ABI 5), where the field is the log2 of the ranks per one-step tile as it stands.
struct TileCode { int ttl, trl, R; bool full_grid, step_rows; };
inline TileCode tile_code(int32_t code) {
  TileCode c = {code & 0xff, (code >> 8) & 0xff, (code >> 16) & 0xff, (code & TILE_FULL_GRID) != 0, (code & TILE_STEP_ROWS) != 0};
  if (c.ttl == 0) c.ttl = 4;
  if (c.trl == 0 && !c.step_rows) c.trl = 4;
  return c;
}
// tile shapes that exist: 16 ranks x 16 / 32 / 64 steps for any vector width (32 ranks per tile were measured too at
// >= 16-byte rows: slower, not instantiated), and — [r5] rows of ONE vector below 16 bytes — 32 x 64 (8-byte rows),
// 64 x 64 (4), 64 x 128 (2), 128 x 128 (1): 16 KiB of payload per tile at every width, runs of 128 .. 512 bytes on both
// sides.  (The taller tiles — 16 x 128 at 8 bytes, 32 x 128 at 4 — are what the host asks for OUT of a PackedSequence:
// the batch-major side is then the one written, and its runs are 1 KiB / 512 B instead of 512 / 256.)
inline bool tile_shape_narrow(int vec, int64_t lpr, int ttl, int trl) {
  return lpr == 1 && ((vec == 8 && trl == 5 && ttl == 6) || (vec == 4 && trl == 6 && ttl == 6) ||
                      (vec == 8 && trl == 4 && ttl == 7) || (vec == 4 && trl == 5 && ttl == 7) ||   // out of a PackedSequence
                      (vec == 2 && trl == 6 && ttl == 7) || (vec == 1 && trl == 7 && ttl == 7));
}
inline bool tile_shape_exists(int vec, int64_t row_bytes, const TileCode& c) {
  return (c.trl == 4 && c.ttl >= 4 && c.ttl <= 6) || tile_shape_narrow(vec, (row_bytes + vec - 1) / vec, c.ttl, c.trl);
}

// The XCD-span geometry, in ONE place.  Workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8): from `min_tiles`
// tiles up (RUA_MOVE_XCD_SPAN_ON / _OFF override) every XCD takes ONE contiguous span of per_xcd tiles instead of every
// eighth tile, and the grid is rounded up to 8 spans; per_xcd == 0 = plain blockIdx order.
struct XcdGrid { int err; bool span; int64_t per_xcd, grid; };     // err: 0, or RUA_ERANGE (grid > 2^31 - 1)
inline XcdGrid xcd_grid(int64_t tiles, int64_t min_tiles, int flags) {
  const bool span = (flags & RUA_MOVE_XCD_SPAN_OFF) ? false : (flags & RUA_MOVE_XCD_SPAN_ON) ? true : tiles >= min_tiles;
  const int64_t per_xcd = span ? (tiles + 7) / 8 : 0, grid = span ? per_xcd * 8 : tiles;
  return {grid > 0x7fffffffLL ? RUA_ERANGE : 0, span, per_xcd, grid};
}
constexpr int64_t NEVER_SPAN = 0x7fffffffffffffffLL;     // a `min_tiles` no launch reaches

// widest power-of-two access (<= 16 bytes) that divides the row size and every base address in `addrs` (their OR)
inline int move_vec(int64_t row_bytes, uintptr_t addrs) {
  const uint64_t mix = (uint64_t)row_bytes | (uint64_t)addrs | 16u;
  return (int)(mix & (~mix + 1));
}
// rows that are a multiple of 8 but not of 16 bytes: 16-byte lanes at 8-byte-aligned addresses + an 8-byte tail.
// Only rows that really END in an 8-byte piece: vec == 8 also comes from a base pointer that is only 8-byte aligned
// under rows of a multiple of 16 bytes (a view at a storage offset), and those have no tail — they keep 8-byte lanes.
inline bool move_tail8(int vec, int64_t row_bytes) { return vec == 8 && (row_bytes & 15) == 8 && row_bytes >= 24; }
// streaming (non-temporal) accesses: forced / forbidden by the flags, else on when the destination cannot stay in cache
inline bool move_nt(int64_t n_rows, int64_t row_bytes, int flags) {
  return (flags & RUA_MOVE_NT_ON) ? true : (flags & RUA_MOVE_NT_OFF) ? false : (double)n_rows * (double)row_bytes >= (double)(512ll << 20);
}
// lanes per row, the log2 of the lanes a wave gives one row per instruction, 64-lane column chunks per row (move_rows_kernel)
struct RowLanes { int64_t lpr; int lp_log2, cpr; };
inline RowLanes row_lanes(int64_t row_bytes, int vec) {
  const int64_t lpr = (row_bytes + vec - 1) / vec;
  return {lpr, lanes_log2(lpr), (int)((lpr + RUA_WAVE - 1) / RUA_WAVE)};
}

// `form`: the kernel family of rua_move.hip that takes the call, in the order plan_move_rows tries them
enum { MOVE_NONE,            // nothing to launch (no rows, or rows of no bytes)
       MOVE_TILES_LDS,       // pack_tile_lds_kernel: (rank x time) tiles between a PackedSequence and a batch-major layout
       MOVE_TILES_VEC,       // pack_tile_vec_kernel: ... their lane-group form, rows of ONE 16-, 8- or 4-byte vector
       MOVE_ROLL_STEPS,      // pack_roll_steps_kernel: a roll inside one PackedSequence, time step by time step
       MOVE_SEQ_COPY,        // seq_copy_kernel: the segmented memcpy between two batch-major layouts
       MOVE_NARROW,          // move_rows_narrow_kernel: rows of one vector, a lane per row
       MOVE_ROLL_TILES,      // pack_roll_tile_kernel: roll / rev inside one PackedSequence on the (rank x time) tiles
       MOVE_SPAN,            // move_rows_span_kernel: the destination tile leaves LDS as one aligned span
       MOVE_ROWS };          // move_rows_kernel: the generic mover (rpt == NARROW_RPT: narrow_same_pack; tail8)
struct MoveRowsPlan {
  int err;                  // 0, or the RUA_E* the call answers without launching anything
  int form, vec;            // vec: bytes per lane (MOVE_ROWS with tail8: 16)
  bool scatter, nt, tail8, to_pack, span;
  int ttl, trl, R, lds;     // the tile kernels: log2 steps / ranks per tile, rows per 128-byte line (1: plain windows), LDS bytes
  int tile_rows, rpt, spw;  // rows per workgroup tile (MOVE_ROWS: TROWS, MOVE_SPAN: trows); rows per lane; sequences per wave
  int lp_log2, cpr, block;
  int64_t phase, lpr, per_xcd;
  unsigned grid;
};

// Of the layouts only scalars, the null-ness of pointers and whether two pointers are EQUAL are read; the payload
// addresses only give alignments.  The order of the tests is the precedence between the forms.
inline MoveRowsPlan plan_move_rows(const rua_layout* dst, const rua_layout* src, int32_t tmap, int64_t tmap_arg,
                                   uintptr_t dst_data, uintptr_t src_data, int64_t row_bytes, int64_t pad_row, int32_t flags) {
  MoveRowsPlan P = {};
  P.R = P.rpt = 1; P.block = RUA_BLOCK;
  auto fail = [&](int e) { P.err = e; P.form = MOVE_NONE; return P; };
  // the launch's XcdGrid into the plan; false: RUA_ERANGE.  (No min_tiles: plain blockIdx order whatever the flags.)
  auto geometry = [&](int64_t tiles, int64_t min_tiles = NEVER_SPAN) {
    const XcdGrid g = xcd_grid(tiles, min_tiles, min_tiles == NEVER_SPAN ? 0 : flags);
    P.span = g.span; P.per_xcd = g.per_xcd; P.grid = (unsigned)g.grid; P.err = g.err;
    return g.err == 0;
  };
  if ((P.err = check_layout(dst, true)) != 0 || (P.err = check_layout(src, false)) != 0) return P;
  if (tmap < RUA_T_SHIFT || tmap > RUA_T_ZERO || row_bytes < 0) return fail(RUA_EINVAL);
  if (dst->n_rows == 0 || row_bytes == 0) return P;
  if (!dst_data || !src_data) return fail(RUA_EINVAL);
  if (pad_row < -1 || pad_row >= src->n_rows) return fail(RUA_EINVAL);
  const int vec = P.vec = move_vec(row_bytes, dst_data | src_data);
  const TileCode dc = tile_code(dst->tile_t_log2), sc = tile_code(src->tile_t_log2);

  // narrow rows between a PackedSequence and a batch-major layout: (rank x time) tiles
  const int span_flags = MOVE_SPAN_FLAGS | RUA_MOVE_NO_TAIL8 | RUA_MOVE_NO_NARROW;
  if ((flags & ~span_flags) == 0 && tmap == RUA_T_SHIFT && tmap_arg == 0 && row_bytes <= TILE_MAX_ROW_BYTES) {
    const bool to_pack = dst->kind == RUA_PACK && (src->kind == RUA_CAT || src->kind == RUA_LEFT || src->kind == RUA_RIGHT);
    // [r5] a padded destination takes the tiles too when the caller asks for the FULL (sequence x step) grid
    // (rua_layout::tile_t_log2 bit 24): every slot is then written, tokens and fill, in the one pass
    const bool full_grid = src->kind == RUA_PACK && sc.full_grid;
    const bool from_pack = src->kind == RUA_PACK && (dst->kind == RUA_CAT || (full_grid && pad_row < 0 &&
                                                     (dst->kind == RUA_LEFT || dst->kind == RUA_RIGHT)));
    const rua_layout* pk = to_pack ? dst : src;
    const TileCode& tc = to_pack ? dc : sc;
    // (a table built for a tile shape this vector width has no kernel for — rows of 8 bytes at a base that is only
    // 4-byte aligned, say — is simply not used)
    if ((to_pack || from_pack) && (pk->tile_start || full_grid) && pk->bsz && pk->n_tiles > 0 && pk->boff &&
        (!full_grid || (!to_pack && dst->kind != RUA_CAT)) && !tc.step_rows && tile_shape_exists(vec, row_bytes, tc)) {
      if (!geometry(pk->n_tiles, to_pack || full_grid ? MOVE_SPAN_MIN_TILES : TILE_SPAN_MIN_TILES_FROM_PACK)) return fail(P.err);
      if (tc.full_grid && (to_pack || (dst->kind != RUA_LEFT && dst->kind != RUA_RIGHT))) return fail(RUA_EINVAL);
      P.to_pack = to_pack; P.ttl = tc.ttl; P.trl = tc.trl; P.lpr = (row_bytes + vec - 1) / vec;
      // the batch-major side's runs start on 128-byte lines (TileTables): R rows per line, if the host built the table for
      // it, the rows divide a line and the payload's own address does not spoil it (its offset inside a line, in rows)
      // ... and only where the batch-major side is the one WRITTEN (P.cat): what costs is a partial-line STORE — the shifted
      // windows trade whole lines on the batch-major side for fragments on the PackedSequence's, so they gain 2-20 % for
      // P.cat and LOSE 6-15 % for the pack, whose packed-side fragments would then be the stores (same-box A/B of both
      // directions at 16 / 32 / 64-byte rows: profiles/r04_tile_shift_ab.txt)
      const uintptr_t major = to_pack ? src_data : dst_data;
      const int R = tc.R;
      if (!(to_pack || tc.full_grid || R < 2 || R > TILE_SHIFT_MAX || (R & (R - 1)) != 0 || R * row_bytes != 128 ||
            (major & 127) % (uintptr_t)row_bytes != 0)) {
        P.R = R; P.phase = (int64_t)((major & 127) / (uintptr_t)row_bytes);
      }
#ifdef RUA_TILE_NO_SHIFT          // developer A/B build
      P.R = 1; P.phase = 0;
#endif
      const int64_t lds = ((((int64_t)1 << (tc.ttl + tc.trl)) + ((int64_t)1 << tc.trl)) * P.lpr) * vec;   // the staged tile + one padding row per rank
      if (lds > (48 << 10)) return fail(RUA_EINVAL);                      // (the host picks the tile by row width: 32 KiB staged at most)
      // 16-byte rows INTO a PackedSequence take the lane-group kernel too (one cell per lane, relative liveness tables: +4 %
      // over the staged kernel, r5r); out of one the staged kernel's line-aligned windows are worth more (-5 % without them)
      const bool lane_group = (to_pack && vec == 16 && P.lpr == 1 && tc.trl == 4 && tc.ttl == 6) ||
                              (vec >= 4 && tile_shape_narrow(vec, P.lpr, tc.ttl, tc.trl));
      P.form = lane_group ? MOVE_TILES_VEC : MOVE_TILES_LDS;
      P.lds = lane_group ? 0 : (int)lds;
      return P;
    }
  }
  P.nt = move_nt(dst->n_rows, row_bytes, flags);
  // Launch geometry (profiles/r02_copy_probe.txt, r02_mover_geometry.txt): HBM rewards a launch whose
  // in-flight addresses form a small window sweeping the destination in order, so a workgroup takes only ~16 KiB
  // of destination rows (workgroups are dispatched in blockIdx order), and on big launches every XCD sweeps ONE
  // contiguous span of the destination instead of every eighth tile.  At the north-star shape (1 KiB rows):
  // 256-row tiles 5.6 TB/s -> 16-row tiles 6.15 TB/s for C->P, 5.3 -> 6.1 for P->C.
  int tile_rows = MOVE_TILE;
  for (int64_t tb = MOVE_TILE * row_bytes; tile_rows > 4 && tb > MOVE_TILE_BYTES; tb >>= 1) tile_rows >>= 1;
  const int tsel = (flags >> 4) & 0xf;               // developer override: RUA_MOVE_TILE_LOG2 / RUA_MOVE_XCD_SPAN_*
  if (tsel >= 2 && tsel <= 8) tile_rows = 1 << tsel;
  if (tile_rows > MOVE_BLOCK) tile_rows = MOVE_BLOCK;
  // (RUA_MOVE_NO_TAIL8, a developer flag, keeps the 8-byte lanes for A/B runs)
  const bool tail8 = move_tail8(vec, row_bytes) && !(flags & RUA_MOVE_NO_TAIL8);
  // 16-byte rows get every tile size; the narrower vector widths (odd row sizes) a coarser choice
  if (vec != 16) tile_rows = tile_rows <= 16 ? 16 : tile_rows <= 64 ? 64 : MOVE_TILE;
  const int64_t nr = dst->n_rows;
  const bool padded_dst = dst->kind == RUA_LEFT || dst->kind == RUA_RIGHT;
  const int64_t rows_min_tiles = padded_dst ? MOVE_SPAN_MIN_TILES : MOVE_SPAN_MIN_TILES_DENSE;
  const bool scatter = P.scatter = (flags & RUA_MOVE_SCATTER) != 0;
  const bool both_pack = dst->kind == RUA_PACK && src->kind == RUA_PACK;
  const bool same_pack = both_pack && dst->bsz && dst->boff && dst->boff == src->boff && dst->sorted == src->sorted &&
                         dst->len_add == 0 && src->len_add == 0 && dst->T == src->T && dst->T > 0;
  // [r5] a roll inside one PackedSequence, time step by time step, when the caller handed over the table of one-step tiles
  if (same_pack && dc.step_rows && dst->tile_start && dst->n_tchunks == dst->T && dst->n_tiles > 0 && tmap == RUA_T_ROLL &&
      pad_row < 0 && (flags & ~MOVE_SPAN_FLAGS) == 0) {
    if (!geometry(dst->n_tiles, MOVE_SPAN_MIN_TILES_DENSE)) return fail(P.err);
    P.form = MOVE_ROLL_STEPS; P.trl = dc.trl;
    return P;
  }
  // [r5] narrow rows between two batch-major layouts: the segmented memcpy (seq_copy_kernel)
  const bool major_d = dst->kind == RUA_CAT || dst->kind == RUA_LEFT || dst->kind == RUA_RIGHT;
  const bool major_s = src->kind == RUA_CAT || src->kind == RUA_LEFT || src->kind == RUA_RIGHT;
  const bool same_lens = dst->lens == src->lens && dst->len_add == src->len_add;
  // the longest sequence either side can hold: the storage's own T for the padded layouts, the caller's hint for a
  // CattedSequence (rua_layout::T_log, 0 = unknown).  One wave walks a sequence whole: none may be a large share
  const int64_t long_d = dst->kind == RUA_CAT ? dst->T_log : dst->T_phys;
  const int64_t long_s = src->kind == RUA_CAT ? src->T_log : src->T_phys;
  const int64_t longest = long_d > long_s ? long_d : long_s;
  const bool balanced = long_d > 0 && long_s > 0 && dst->B >= 4096 && longest <= nr / 1024;
  // (rows wider than 64 bytes that are not a multiple of 16 were tried here too: one wave per sequence streams at the
  // walk's 4.5 - 5.4 TB/s whatever the alignment, below what tiles in destination order give: move_rows_span_kernel)
  if (major_d && major_s && !scatter && !(flags & RUA_MOVE_NO_NARROW) && tsel == 0 && pad_row < 0 &&
      row_bytes <= 64 && dst->B == src->B && (tmap == RUA_T_SHIFT || (tmap == RUA_T_ROLL && same_lens)) && balanced &&
      (dst->kind != RUA_CAT || dst->off || !dst->lens) && (src->kind != RUA_CAT || src->off || !src->lens)) {
    // sequences per wave: about 16 KiB of tokens (8 at narrow rows, 1 from a few hundred bytes per row up)
    const int64_t seq_bytes = nr / (dst->B > 0 ? dst->B : 1) * row_bytes;
    P.spw = seq_bytes >= 8192 ? 1 : seq_bytes >= 4096 ? 2 : seq_bytes >= 2048 ? 4 : SEQ_PER_WAVE;
    const int64_t waves = (dst->B + P.spw - 1) / P.spw;
    if (!geometry((waves + RUA_WAVES_PER_BLOCK - 1) / RUA_WAVES_PER_BLOCK)) return fail(P.err);
    P.form = MOVE_SEQ_COPY;
    return P;
  }
  // [r5] rows of one vector (1-D payloads: 1 .. 16 bytes): a lane per row from resolution to store, eight rows in flight
  // per lane (move_rows_narrow_kernel).  The roll tiles below keep 16-byte rows inside one PackedSequence.
  const bool one_vec = row_bytes == vec && !(flags & RUA_MOVE_NO_NARROW) && tsel == 0;
  const bool roll_tiles = vec == 16 && both_pack && dst->tile_start && dst->bsz && !dc.step_rows &&
                          dst->boff == src->boff && !scatter;
  if (one_vec && !roll_tiles) {
    const int64_t per_tile = (int64_t)RUA_BLOCK * NARROW_CH;
    if (!geometry((nr + per_tile - 1) / per_tile, rows_min_tiles)) return fail(P.err);
    P.form = MOVE_NARROW;
    return P;
  }
  // roll / rev inside ONE PackedSequence with rows of at most 32 B (3.1 -> 3.9 TB/s; no gain at 64 B): RPT rows per lane (the kernel's `same_pack` test)
  const bool narrow_same_pack = !scatter && vec == 16 && row_bytes <= 32 && same_pack;
  // ... and on the (rank x time) tiles when the caller handed the tile table over (pack_roll_tile_kernel)
  if (narrow_same_pack && dst->tile_start && !dc.step_rows && dst->n_tiles > 0 && dst->lens && dst->sorted &&
      pad_row < 0 && (flags & ~MOVE_SPAN_FLAGS) == 0 &&
      (tmap == RUA_T_ROLL || tmap == RUA_T_REV_S || tmap == RUA_T_REV_D || tmap == RUA_T_SHIFT)) {
    if (!geometry(dst->n_tiles, MOVE_SPAN_MIN_TILES)) return fail(P.err);
    if (dc.ttl < 4 || dc.ttl > 6) return fail(RUA_EINVAL);
    P.form = MOVE_ROLL_TILES; P.ttl = dc.ttl; P.lpr = (row_bytes + vec - 1) / vec;
    return P;
  }
  // [r5] a gather of rows that are a multiple of 4 but not of 16 bytes: the destination tile goes through LDS and leaves as
  // one aligned span (move_rows_span_kernel)
  // ([r5, late] and of rows that ARE a multiple of 16 bytes but not of a 128-byte line — 2 000-byte rows, H = 1 000 in
  // bf16: the row mover's 16-byte lanes are aligned there, but every wave instruction straddles one line more than it
  // fills and every row boundary is two partial lines; as a span the tile is stored in whole lines)
  const bool off16 = (row_bytes & 15) != 0 && (row_bytes & 3) == 0;
  // (from 1 KiB up: at 640 / 656-byte rows the row mover is level or ahead — 5.41 / 5.40 against 5.36 / 5.00 TB/s for the
  // pack, profiles/r05_span16_ab.txt)
  const bool off128 = (row_bytes & 15) == 0 && (row_bytes & 127) != 0 && row_bytes > 1024;
  if (!scatter && (off16 || off128) && row_bytes >= 64 && row_bytes <= SPAN_TILE_BYTES / 2 && (dst_data & 15) == 0 &&
      (src_data & 15) == 0 && tsel == 0 && !(flags & RUA_MOVE_NO_TAIL8)) {
    // rows per tile: a multiple of 2 (rows of 8 mod 16 bytes) or 4 (4 / 12 mod 16), so that every tile starts on a
    // 16-byte boundary (any number of rows of whole vectors: only the two ends of a tile are partial lines then); as many
    // as fit 16 KiB of LDS (16 rows of 1 000 bytes, 8 of 2 000), one resolving lane each
    const int step = off128 ? 1 : (row_bytes & 7) ? 4 : 2;
    int trows = (int)(SPAN_TILE_BYTES / row_bytes) / step * step;
    if (trows > RUA_BLOCK) trows = RUA_BLOCK / step * step;
    if (trows > 0) {        // (a line-aligned tile of some widths would not fit the 16 KiB: the row mover takes those)
      if (!geometry((nr + trows - 1) / trows, rows_min_tiles)) return fail(P.err);
      P.form = MOVE_SPAN; P.tile_rows = trows;
      return P;
    }
  }
  P.form = MOVE_ROWS; P.block = MOVE_BLOCK; P.tail8 = tail8; P.vec = tail8 ? 16 : vec;
  const RowLanes rl = row_lanes(row_bytes, P.vec);
  P.lpr = rl.lpr; P.lp_log2 = rl.lp_log2; P.cpr = rl.cpr;
  P.rpt = narrow_same_pack ? NARROW_RPT : 1;       // (vec == 16, gather: see move_rows_kernel<..., RPT>; plain blockIdx order)
  P.tile_rows = narrow_same_pack ? MOVE_TILE : tile_rows;
  const int64_t per_tile = (int64_t)P.tile_rows * P.rpt;
  if (!geometry((nr + per_tile - 1) / per_tile, narrow_same_pack ? NEVER_SPAN : rows_min_tiles)) return fail(P.err);
  return P;
}

// rua_setitem_backward's gather-and-zero kernel: one wave per 64 list entries.  `ptrs`: the OR of grad, grad_value and
// grad_raw; `dst_rows`: the rows of the larger output (the mover's streaming rule).
struct SetitemBackwardPlan { int err, vec; bool tail8, nt; int lp_log2, cpr; int64_t lpr; unsigned grid; };
inline SetitemBackwardPlan plan_setitem_backward(int64_t list_rows, int64_t dst_rows, int64_t row_bytes, uintptr_t ptrs, int32_t flags) {
  SetitemBackwardPlan P = {};
  P.vec = move_vec(row_bytes, ptrs);
  if ((P.tail8 = move_tail8(P.vec, row_bytes))) P.vec = 16;
  P.nt = move_nt(dst_rows, row_bytes, flags);
  const RowLanes rl = row_lanes(row_bytes, P.vec);
  P.lpr = rl.lpr; P.lp_log2 = rl.lp_log2; P.cpr = rl.cpr;
  const XcdGrid g = xcd_grid(((list_rows + RUA_WAVE - 1) / RUA_WAVE + RUA_WAVES_PER_BLOCK - 1) / RUA_WAVES_PER_BLOCK, NEVER_SPAN, 0);
  P.err = g.err; P.grid = (unsigned)g.grid;
  return P;
}

}  // namespace rua
