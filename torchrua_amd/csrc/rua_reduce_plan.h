// rua_reduce_plan.h — what the segmented reduce decides BEFORE its first HIP call, as plain host C++ (no HIP header):
// alignment, lanes per row, the ranks / team / split thresholds and the grids.  plan_reduce / plan_backward are the one
// place these live: the launchers (rua_reduce_impl.h) launch what a plan says, the dispatch trace and
// rua_debug_reduce_plan print it (rua_reduce.hip), and a machine without a GPU can ask for it.
#pragma once
#include <stdint.h>
#include "rua.h"
#include "rua_wave.h"

namespace rua {

#ifndef RUA_UNROLL_T
#define RUA_UNROLL_T 8
#endif
constexpr int REDUCE_UNROLL_T = RUA_UNROLL_T;           // rows in flight per wave (RUA_UNROLL_T overrides it in A/B builds)
constexpr int64_t REDUCE_TEAM_MAX_UNITS = 16384;        // beyond this one wave per unit keeps the chip balanced by itself
constexpr int COMBINE_WAVES_MAX = 16;
constexpr int REDUCE_HINT_NO_EMPTY = 1, REDUCE_HINT_SHORT_SEQS = 2;    // plan_reduce's `hints`
constexpr int64_t RANKS_MIN_WAVES = 4096;   // adjacent-rank waves (RANKS) only when B / ranks-per-wave still fills the chip
constexpr int64_t RANKS_MIN_WAVES_SHORT = 512;   // ... of SHORT sequences (plan_reduce)
constexpr int COMBINE_SOLO = 32;
constexpr int64_t COMBINE_GRID = 512;   // 2 workgroups per CU
constexpr int BROWS_MAX = 256;
constexpr int64_t SPLIT_GRID_CAP = 16384;   // tail / combine grids: 2x the wave slots of the chip, then stride
// `extra_count` of the backward kernels: bit 0 = the old destination row of a scatter_* took part (MEAN's divisor,
// PROD's factors); bit 1 = RUA_BWD_TIES_POSITIVE
constexpr int BWD_SELF_COUNTS = 1, BWD_TIES_POSITIVE = 2;

// The reducer's wave-team rule (seg_reduce_team_kernel), in ONE place: plan_reduce and the host planner that prices
// long-sequence splitting (rua_reduce_team_waves -> _meta.reduce_split_rows) both call it.
// Vector path only (16-byte lanes, rows up to 1 KiB): a team of 2 or 4 waves shares a unit when an average unit holds
// at least 4 row groups per wave and there are at most `REDUCE_TEAM_MAX_UNITS` units.
inline int reduce_team_waves(int64_t n_rows, int64_t B, int lp_log2, int64_t units, int unroll_t = REDUCE_UNROLL_T) {
  if (units <= 0 || units > REDUCE_TEAM_MAX_UNITS) return 1;
  const int64_t rows_per_group = (int64_t)(RUA_WAVE >> lp_log2) * unroll_t;
  const int64_t groups = n_rows / (B > 0 ? B : 1) / rows_per_group;       // row groups of an average unit
  return groups >= 4 * 4 ? 4 : groups >= 4 * 2 ? 2 : 1;
}

// (lanes_log2, the lanes a row occupies in a wave instruction: rua_wave.h)
// streaming (non-temporal) accesses for a payload that cannot stay in cache
inline bool reduce_nt(int64_t n_rows, int64_t H, int esize) {
  return (double)n_rows * (double)H * (double)esize >= (double)(512ll << 20);
}
// the long-sequence split (see SplitWs): extra parts at most, and the grid of the kernels that stride over them
inline int64_t split_max_extra(int64_t n_rows, int64_t split) { return split > 0 ? n_rows / split : 0; }
inline unsigned split_grid(int64_t max_u) { return (unsigned)(max_u < SPLIT_GRID_CAP ? max_u : SPLIT_GRID_CAP); }

enum { REDUCE_RANKS, REDUCE_TEAM, REDUCE_SEQ };     // seg_reduce_ranks_kernel / _team_kernel / seg_reduce_kernel
struct ReducePlan {
  int err;                  // 0, or the RUA_E* the call answers without launching anything
  int form, esize, op, epl, lp_log2, cpw, wpb, team, glog, check, no_empty;
  bool ties, nt, copy, split;       // ties: max / min count their ties (the _T ops); split: tail + combine follow
  int64_t n_chunks, split_rows, max_u;
  unsigned grid;            // WAVES of the main kernel (SEQ with wpb == 2 launches (grid + 1) / 2 workgroups)
};

enum { BWD_ROWS, BWD_RANKS, BWD_WALK, BWD_SEQ };    // seg_backward_rows_ / _ranks_ / _walk_kernel, seg_backward_kernel
struct BackwardPlan {
  int err;
  int form, esize, op, epl, lp_log2, n_phases, tv[2], tile_rows;    // tv: the kernels' TIES of each launch, in order
  bool nt, span, do_split, phased, ties_final, pad_memset;
  int64_t n_chunks, per_xcd, split_rows, max_u;
  unsigned grid;
};

// `ptrs`: the OR of the payload pointers (data, out, copy, ties).  Of `L` only scalars and the null-ness of pointers are read.
// (The kernels' comments call this decision by its earlier name, dispatch_reduce_main.)
inline ReducePlan plan_reduce(const rua_layout& L, int esize, int64_t H, int op, int include_self, bool perm, bool ws,
                              bool ties, bool copy, uintptr_t ptrs, int64_t split, int hints) {
  ReducePlan P = {};
  P.form = REDUCE_SEQ; P.esize = esize; P.op = op; P.team = 1; P.copy = copy; P.ties = ties && !copy;
  P.no_empty = (hints & REDUCE_HINT_NO_EMPTY) ? 1 : 0; P.split_rows = split;
  const bool short_seqs = (hints & REDUCE_HINT_SHORT_SEQS) != 0;
  if (op < RUA_SUM || op > RUA_LOGSUMEXP) { P.err = RUA_EINVAL; return P; }
  const int FULL = 16 / esize;
  const int HALF = FULL >= 4 ? FULL / 2 : 1;      // 8-byte loads: hidden sizes that are a multiple of 8 bytes only
  const bool aligned_ok = (H % FULL == 0) && (ptrs % 16 == 0);
  // Rows of 8 (mod 16) bytes (H = 500 in bf16): every other row starts on an 8-byte boundary only and the last lane of
  // a row would hold half a vector.  gfx950 takes a dwordx4 at any dword-aligned address, and the LAST lane simply
  // covers the last FULL elements of the row, overlapping its neighbour by half a vector: both lanes fold the same
  // elements in the same order and store the same results (make_unit clamps the column).  Round 2 used 8-byte lanes
  // there — two column chunks, two waves per row, 4.0 TB/s for segment_max over a CattedSequence at H = 500.
  // (Not with include_self == 1: the store then reads the old row, and two lanes would fold it in twice.)
  const bool tail_ok = !aligned_ok && FULL > 1 && H > FULL && (H + FULL - 1) / FULL <= RUA_WAVE &&
                       (H * (int64_t)esize) % 8 == 0 && (ptrs % 8 == 0) && include_self != 1 && !copy;
  const bool vec_ok = aligned_ok || tail_ok;
  // (H = 300 or 650 in bf16 — GloVe vectors, PTB-sized LSTMs: the scalar path moves 128 B per wave instruction and
  // measured 2.9 TB/s; 8-byte lanes move 512 B)
  const bool half_ok = !vec_ok && HALF > 1 && (H % HALF == 0) && (ptrs % 8 == 0);
  P.epl = vec_ok ? FULL : half_ok ? HALF : 1;
  const int64_t lpr = (H + P.epl - 1) / P.epl;  // lanes per row
  const int lp_log2 = P.lp_log2 = lanes_log2(lpr);
  // rows wider than one wave instruction (1 KiB): one wave owns 4 column chunks, i.e. up to 4 KiB of the row
  // (the same for 8-byte lanes: H = 500 in bf16 is 125 lanes — as two column chunks two waves each read every other
  // 512-byte half of the rows: reduce over P at H = 500 5.0 -> 5.7 TB/s
  // — over a PackedSequence only: over the batch-major layouts, whose sequences are contiguous, the two waves per row
  // were the better half of the bytes in flight: 4.0 -> 2.7 TB/s when tried)
  const bool wide = (vec_ok || (half_ok && L.kind == RUA_PACK)) && lpr > RUA_WAVE;
  P.cpw = wide ? 4 : 1;
  P.n_chunks = (lpr + RUA_WAVE * P.cpw - 1) / (RUA_WAVE * P.cpw);
  const int64_t blocks = L.B * P.n_chunks;  // one wave per unit
  if (blocks > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
  P.nt = vec_ok && reduce_nt(L.n_rows, H, esize);       // (the 8-byte and scalar lanes have no streaming form)
  P.grid = (unsigned)blocks;
  if (copy && !aligned_ok) { P.err = RUA_EALIGN; return P; }   // fused pack + reduce: vector path only (caller falls back to two launches)
  // (only when that still leaves >= 4 waves per SIMD: with fewer sequences one wave per sequence fills the chip better)
  // (RUA_OP_SHORT_SEQS: the caller knows the longest sequence and vouches that none is far above the average — the
  // wave walks to the longest of its sequences, so ONE long sequence among short ones would be walked by one lane group)
  bool cat_ranks = L.kind == RUA_CAT && L.lens && L.len_add == 0 && lp_log2 < 6;
  int glog = 0;                                   // log2 of the row slots of one sequence's lane group (make_unit)
  if (cat_ranks) {
    const int64_t side = RUA_WAVE >> lp_log2;     // sequences side by side with one row slot each
    const int64_t short_avg = 4 * side < 16 ? 16 : (4 * side > 64 ? 64 : 4 * side);
    if (L.n_rows > short_avg * L.B) {             // longer than that on average:
      if (lp_log2 <= 1) glog = 4 - lp_log2;       // FOUR sequences per wave at rows of <= 32 bytes (16 / 8 rows of each
      else cat_ranks = false;                     // per instruction; the wave checks its own lengths), else one wave each
    }                                             // (short on average, no word about the longest: the waves check, `check`)
    // ([r5] a batch too small to fill the chip with every row slot its own sequence still fills it four to a wave at
    // rows of <= 32 bytes)
    if (cat_ranks && glog == 0 && lp_log2 <= 1 && (L.B >> (6 - lp_log2)) < RANKS_MIN_WAVES_SHORT) glog = 4 - lp_log2;
  }
  // How many side-by-side waves are enough: RANKS_MIN_WAVES when the sequences may be long (a wave then walks hundreds of
  // steps one after the other, and only plenty of them keep the chip busy); a few hundred when they are SHORT — a
  // CattedSequence that is short on average, a PackedSequence of at most 128 time steps — where the alternative is one
  // wave per sequence at one row per instruction: 200 000 x U(1,32) rows of 16 bytes are 3 125 waves of 64 sequences
  const bool short_form = (cat_ranks && glog == 0) || (L.kind == RUA_PACK && L.T > 0 && L.T <= 128);
  const int64_t ranks_min_waves = short_form ? RANKS_MIN_WAVES_SHORT : RANKS_MIN_WAVES;
  // ([r5] with the long-sequence split armed — lengths nobody vouches for — the four-per-wave form splits by itself)
  const int ranks_check = (cat_ranks && !short_seqs) ? 1 : 0;
  const bool ranks_split = split > 0 && ws && cat_ranks && (glog > 0 || ranks_check) && vec_ok && split_max_extra(L.n_rows, split) > 0;
  if (((L.kind == RUA_PACK && L.sorted) || cat_ranks) && !copy && !perm && lp_log2 < 6 && (!(split > 0 && ws) || ranks_split) &&
      (L.B >> (6 - lp_log2 - glog)) >= ranks_min_waves) {
    // narrow rows of a PackedSequence: adjacent ranks share a wave instruction
    // (tried for a CattedSequence with 32-byte rows too — groups = adjacent sequences: 4.0 -> 2.8 TB/s at U(8,512),
    // unsorted neighbours differ too much in length — so C keeps one wave per sequence, EXCEPT for batches of short
    // sequences, when the caller says so: there a wave per sequence is bound by the rate at which workgroups can be
    // dispatched at all — 4 M singletons: 2.98 ms, 1.3 workgroups per ns; 500 000 sequences of 16 rows on average:
    // 0.40 -> 0.06-0.07 ms at 16 / 32-byte rows, 0.43 -> 0.21 at 128: profiles/r04_cat_ranks_ab.txt.  And at rows of
    // <= 32 bytes a whole sequence of a few hundred rows is a handful of wave instructions behind a chain of dependent
    // loads — 2.2 / 4.1 TB/s at 16 / 32 bytes with U(8,512) lengths — so there FOUR sequences share a wave, sixteen /
    // eight rows of each per instruction.  Every row slot its own sequence only under the caller's word that no sequence
    // is far above the average, because the wave walks to the longest of its sequences; the four-per-wave form checks
    // that by itself, wave by wave (seg_reduce_ranks_kernel), so it also serves lengths that live on the device only)
    const int64_t rpw = RUA_WAVE >> (lp_log2 + glog);
    const int64_t nblk = (L.B + rpw - 1) / rpw;
    if (nblk > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
    P.form = REDUCE_RANKS; P.wpb = 1; P.glog = glog; P.check = ranks_check; P.split = ranks_split;
    P.grid = (unsigned)nblk;
    P.max_u = ranks_split ? split_max_extra(L.n_rows, split) : 0;      // (one column chunk per row here)
    if (P.max_u > 0x7fffffffLL) P.err = RUA_ERANGE;
    return P;
  }
  // few-but-long units: a team of waves per unit (seg_reduce_team_kernel) — vector path, rows up to 1 KiB, no split
  if (vec_ok && !wide && !copy && !(split > 0 && ws)) {
    const int team = reduce_team_waves(L.n_rows, L.B, lp_log2, blocks);   // (the one rule)
    if (team > 1) {
      P.form = REDUCE_TEAM; P.wpb = P.team = team;
      return P;
    }
  }
  P.max_u = split_max_extra(L.n_rows, split) * P.n_chunks;
  P.split = split > 0 && ws && P.max_u > 0;
  if (P.split && P.max_u > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
  // Two INDEPENDENT waves per workgroup over the batch-major layouts (C / L / R): neighbouring sequences are
  // neighbouring storage, and halving the number of workgroups is worth 6-9 % there (cfg3 segment_sum 108.8 -> 101.3 us,
  // north-star segment_sum(c) 2.86 -> 2.70 ms); four are no better, and over a PackedSequence — walked longest sequence
  // first, every rank its own slot — two LOSE 7 % (2.64 -> 2.84 ms): one wave per workgroup stays there
  // (profiles/r04_reduce_wpb_ab.txt, measured with a temporary environment knob).
  // Rows of at least 512 bytes only: at 16 / 32-byte rows (a whole short sequence per wave instruction) two waves per
  // workgroup lose 7-10 % (final width sweep of round 4: 2.36 -> 2.20, 4.40 -> 3.95 TB/s).
  P.wpb = (copy || P.cpw != 1 || P.split) ? 1 : ((L.kind != RUA_PACK && H * (int64_t)esize >= 512) ? 2 : 1);
  return P;
}

// `ptrs`: the OR of data, out, grad_out, grad_in, ties and self_in.  ties_final: the forward already counted the ties
// (RUA_MAX_T / RUA_MIN_T) -> the apply phase alone, ONE walk.
inline BackwardPlan plan_backward(const rua_layout& L, int esize, int64_t H, int op, int extra_count, bool perm, bool ws,
                                  bool ties, bool ties_final, bool self_in, bool fill_padding, uintptr_t ptrs,
                                  int64_t split) {
  BackwardPlan P = {};
  P.form = BWD_SEQ; P.esize = esize; P.op = op; P.n_phases = 1; P.ties_final = ties_final; P.split_rows = split;
  if (op < RUA_SUM || op > RUA_LOGSUMEXP) { P.err = RUA_EINVAL; return P; }
  const int FULL = 16 / esize;
  const int HALF = FULL >= 4 ? FULL / 2 : 1;
  const bool vec_ok = (H % FULL == 0) && (ptrs % 16 == 0);
  const bool half_ok = !vec_ok && HALF > 1 && (H % HALF == 0) && (ptrs % 8 == 0);
  P.epl = vec_ok ? FULL : half_ok ? HALF : 1;
  const int64_t lpr = (H + P.epl - 1) / P.epl;
  const int lp_log2 = P.lp_log2 = lanes_log2(lpr);
  P.n_chunks = (lpr + RUA_WAVE - 1) / RUA_WAVE;
  const int64_t blocks = L.B * P.n_chunks;
  if (blocks > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
  P.grid = (unsigned)blocks;
  const bool extreme_op = op == RUA_MAX || op == RUA_MIN;
  // one storage row at a time (seg_backward_rows_kernel): every op whose row gradient needs no walk over the sequence
  const bool rows_op = op == RUA_SUM || op == RUA_MEAN || op == RUA_LOGSUMEXP || (extreme_op && ties && ties_final);
  const bool plain = !perm && !self_in && !(extra_count & BWD_SELF_COUNTS);     // no indirection, no old destination row
  // — for the BATCH-MAJOR layouts: consecutive storage rows there belong to one sequence and share its out / grad /
  // ties rows (L1 hits); consecutive rows of a PackedSequence belong to 16 different sequences, each with its own
  // three rows to fetch — measured 3.4 TB/s for sum over P against 6.0 for the walk, which loads them once per sequence
  // (ops that read x: rows up to 1 KiB — one wave instruction per row; wider rows leave a wave one row of a 4-row
  // tile and the walk's 4.4 TB/s beats 3.5)
  // ([r5] every width: at rows wider than 1 KiB the waves of a workgroup take the column chunks of the same few rows)
  if (vec_ok && plain && rows_op && L.kind != RUA_PACK && H * (int64_t)esize >= 64) {
    const int64_t row_bytes = H * (int64_t)esize;
    P.tile_rows = BROWS_MAX;
    for (int64_t tb = BROWS_MAX * row_bytes; P.tile_rows > 4 && tb > (16 << 10); tb >>= 1) P.tile_rows >>= 1;
    const int64_t ntiles = (L.n_rows + P.tile_rows - 1) / P.tile_rows;
    P.span = ntiles >= 2048;
    P.per_xcd = P.span ? (ntiles + 7) / 8 : 0;
    const int64_t grid = P.span ? P.per_xcd * 8 : ntiles;
    if (grid > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
    P.form = BWD_ROWS; P.grid = (unsigned)grid; P.nt = reduce_nt(L.n_rows, H, esize);
    return P;
  }
  // the walk-per-sequence kernels write token rows only: zero the padding rows of a padded layout first when asked to
  P.pad_memset = fill_padding && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT);
  if (L.kind == RUA_PACK && L.sorted && !perm && (!ties || ties_final) && lp_log2 < 6 && !(split > 0 && ws) &&
      !(extra_count & BWD_SELF_COUNTS) && !self_in && (L.B >> (6 - lp_log2)) >= RANKS_MIN_WAVES) {
    // narrow rows of a PackedSequence: adjacent ranks share a wave instruction
    const int64_t rpw = RUA_WAVE >> lp_log2;
    const int64_t nblk = (L.B + rpw - 1) / rpw;
    if (nblk > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
    P.form = BWD_RANKS; P.grid = (unsigned)nblk;
    P.tv[0] = (extreme_op && ties) ? 2 : 0;
    return P;
  }
  // whole sequences, no indirection, an op whose row gradient needs no counting walk: the lean walk (one wave per
  // (sequence, column chunk) — a PackedSequence of wide rows, and x-reading ops over rows wider than 1 KiB)
  if (plain && rows_op && !(split > 0 && ws)) {
    P.form = BWD_WALK;
    P.nt = reduce_nt(L.n_rows, H, esize);
    return P;
  }
  P.phased = extreme_op && ties;        // count phase, then apply phase
  P.max_u = split_max_extra(L.n_rows, split) * P.n_chunks;
  // PROD keeps whole sequences: its zero-factor special case needs the zero count and the product of the other
  // factors of the whole sequence, and a product combined by atomics would not be reproducible
  P.do_split = split > 0 && ws && P.max_u > 0 && (!extreme_op || P.phased) && op != RUA_PROD;
  if (P.do_split && P.max_u > 0x7fffffffLL) { P.err = RUA_ERANGE; return P; }
  P.tv[0] = P.phased ? (ties_final ? 2 : 1) : 0;
  if (P.phased && !ties_final) { P.n_phases = 2; P.tv[1] = 2; }
  return P;
}

}  // namespace rua
