// rua_move.hip — the row mover: every layout conversion / select of the hot path as ONE
// two-phase kernel (gfx950, wave64, HBM-bound; no MFMA — this is byte movement).
//
//   phase 1 (index generation, one lane per row): for the tile's 256 destination rows, turn
//            row j -> token (b,t) -> source row with the closed forms of rua_dev.h; the
//            (load_row, store_row) pairs are staged in LDS.  Integer work happens once per ROW.
//   phase 2 (payload, one lane per 16 bytes): the 4 waves stream the tile, each wave
//            instruction moving 1 KiB (64 lanes x dwordx4), 4 loads in flight per lane,
//            addresses = LDS row index * row_bytes + column.  Padding rows store the fill
//            pattern without loading, so padded outputs are written exactly once.
//
// Tiles are contiguous in the DESTINATION storage, so stores are perfectly coalesced and every
// tile carries the same number of bytes (no ragged load imbalance); loads are row-granular
// gathers (>= 128 B lines, 1 KiB at the north-star shape).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <type_traits>
#include "rua_dev.h"
#include "rua_move_plan.h"      // the thresholds, the launch geometry and WHICH of the kernels below takes a call

namespace rua {

#ifndef RUA_MOVE_UNROLL       // developer knob for A/B builds (scripts/pack_ab.py), like RUA_MOVE_BLOCK
#define RUA_MOVE_UNROLL 4
#endif
constexpr int UNROLL = RUA_MOVE_UNROLL;             // row groups in flight per wave in phase 2

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));     // a 16-byte piece that only sits on an 8-byte boundary
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));     // ... or on a 4-byte one (gfx950 takes a dwordx4 at any dword-aligned address)

template <int VEC> struct vec_of;
template <> struct vec_of<16> { using type = u32x4; };
template <> struct vec_of<8>  { using type = u32x2; };
template <> struct vec_of<4>  { using type = uint32_t; };
template <> struct vec_of<2>  { using type = uint16_t; };
template <> struct vec_of<1>  { using type = uint8_t; };

template <int VEC> __device__ __forceinline__ typename vec_of<VEC>::type fill_of(uint4 p);
template <> __device__ __forceinline__ u32x4    fill_of<16>(uint4 p) { u32x4 v = {p.x, p.y, p.z, p.w}; return v; }
template <> __device__ __forceinline__ u32x2    fill_of<8>(uint4 p)  { u32x2 v = {p.x, p.y}; return v; }
template <> __device__ __forceinline__ uint32_t fill_of<4>(uint4 p)  { return p.x; }
template <> __device__ __forceinline__ uint16_t fill_of<2>(uint4 p)  { return (uint16_t)p.x; }
template <> __device__ __forceinline__ uint8_t  fill_of<1>(uint4 p)  { return (uint8_t)p.x; }

// NT: non-temporal (streaming) accesses for payloads far larger than the 256 MiB Infinity Cache —
// every byte is touched exactly once, so keeping it in L2/MALL only evicts the index vectors.
// Measured at the north-star shape: 6.53 -> 6.26 ms (+4 %).  Small payloads keep the default policy
// so that a following kernel can still find them in cache.
template <typename V, bool NT> __device__ __forceinline__ V ld_row(const char* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
  return *reinterpret_cast<const V*>(p);
}
template <typename V, bool NT> __device__ __forceinline__ void st_row(char* p, V v) {
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
  else *reinterpret_cast<V*>(p) = v;
}

// Rows that are a multiple of 8 but not of 16 bytes (H = 500 in bf16: 1 000-byte rows): every other row starts on an
// 8-byte boundary only.  With 8-byte lanes such a row is two wave instructions of 512 and 488 bytes (measured 4.2 TB/s
// where 1 024-byte rows move at 6.1); gfx950 takes a dwordx4 at any dword-aligned address, so the row goes as 62
// sixteen-byte lanes and one 8-byte lane instead — ONE wave instruction again (TAIL8).
template <bool NT> __device__ __forceinline__ u32x4 ld_row_a8(const char* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4_a8*>(p));
  return *reinterpret_cast<const u32x4_a8*>(p);
}
template <bool NT> __device__ __forceinline__ void st_row_a8(char* p, u32x4 v) {
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4_a8*>(p));
  else *reinterpret_cast<u32x4_a8*>(p) = v;
}

// The other side of the wave's enumerated rows: lane i holds enumerated row jw0 + i of `D` (i < nw; ALL 64 lanes must
// call) and gets the row of `S` it maps to — the source row of a gather, the destination row of a scatter — or -1 (fill /
// skip), or `pad_row` for a padding row of a padded destination.  The wave resolves its rows TOGETHER (coop_resolve).
// `win` (may be NULL): a window of D's offsets computed ONCE for rows at or before jw0 (wave_window) — the narrow-row
// kernel resolves 64 * CH consecutive rows per wave from one 64-ary search instead of CH.
struct WaveWindow { int64_t lo, W; };
__device__ __forceinline__ bool wave_window(const rua_layout& D, int64_t jw0, int lane1, WaveWindow& w) {
  if (D.kind == RUA_PACK && D.T > 0 && D.boff) { coop_window([&](int64_t k) { return D.boff[k]; }, D.T, jw0, lane1, w.lo, w.W); return true; }
  if (D.kind == RUA_CAT && D.off && D.B > 0) { coop_window([&](int64_t k) { return cat_off(D, k); }, D.B, jw0, lane1, w.lo, w.W); return true; }
  return false;
}
template <bool SCATTER>
__device__ __forceinline__ int64_t resolve_wave_rows(const rua_layout& D, const rua_layout& S, int32_t tmap, int64_t targ,
                                                     int64_t pad_row, int64_t jw0, int nw, int lane1, bool same_pack,
                                                     const WaveWindow* win = nullptr) {
  const int64_t j = jw0 + lane1;
  const bool mine = lane1 < nw;
  int64_t b = 0, t = 0, other = -1;
  bool token = false;
  bool resolved = false;
  bool done = false;
  if (D.kind == RUA_PACK && D.T > 0 && D.boff) {
    int64_t bt;
    const bool ok = win ? coop_lookup(win->W, win->lo, D.T, j, t, bt)
                        : coop_resolve([&](int64_t k) { return D.boff[k]; }, D.T, jw0, nw, lane1, t, bt);
    if (same_pack) {
      // roll / rev inside ONE PackedSequence: the rank r of a row is its own source rank, and its length is
      // #{t : bsz[t] > r} — read off batch_sizes instead of two random gathers per row.  The wave looks its rows'
      // lengths up TOGETHER (a 10-step binary search per row was the longest dependent chain of the tile: cfg4's
      // P.roll, 2-KiB rows): -bsz is non-decreasing, len = 1 + the largest k with -bsz[k] <= -(r + 1); the rows
      // of a wave are neighbouring ranks, whose lengths sit within one 64-entry window of the smallest of them.
      constexpr int64_t BIG = 0x7fffffffffffffffLL;
      const bool have = mine && ok && j - bt >= 0 && j - bt < D.bsz[0];
      const int64_t r = have ? j - bt : 0;
      const int64_t x = have ? -(r + 1) : BIG;
      int64_t base = x;
#pragma unroll
      for (int d = RUA_WAVE / 2; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(base, d, RUA_WAVE);
        base = o < base ? o : base;
      }
      int64_t wlo = 0, W = BIG, k = 0, fk = 0;
      bool hit = false;
      if (base != BIG) {                                          // wave-uniform
        coop_window([&](int64_t q) { return -D.bsz[q]; }, D.T, base, lane1, wlo, W);
        hit = coop_lookup(W, wlo, D.T, x, k, fk);
      }
      if (mine && ok) {
        resolved = true;
        int64_t len = 0;
        if (have) {
          if (hit && fk <= x) {
            len = k + 1;
          } else {                                                // the window did not reach: search alone
            int64_t lo = 0, hi = D.T;
            while (lo < hi) {
              const int64_t mid = (lo + hi) >> 1;
              if (D.bsz[mid] > r) lo = mid + 1; else hi = mid;
            }
            len = lo;
          }
        }
        const int64_t ts = apply_tmap(tmap, targ, t, len, len);
        if (have && ts >= 0 && ts < len) other = S.boff[ts] + r;
        if (other >= S.n_rows) other = -1;
        done = true;
      }
    } else if (mine && ok) {
      resolved = true;
      const int64_t r = j - bt;
      if (r >= 0 && r < D.B) {
        b = D.sorted ? D.sorted[r] : r;
        token = b >= 0 && b < D.B;
      }
    }
  } else if (D.kind == RUA_CAT && D.off && D.B > 0) {
    int64_t ob;
    const bool ok = win ? coop_lookup(win->W, win->lo, D.B, j, b, ob)
                        : coop_resolve([&](int64_t k) { return cat_off(D, k); }, D.B, jw0, nw, lane1, b, ob);
    if (mine && ok) { resolved = true; token = true; t = j - ob; }
  }
  if (mine && !done) {
    if (!resolved) token = row_to_token(D, j, b, t);
    if (token) {
      // caller-supplied (batch_ptr, token_ptr) pairs are range-checked: a bad pair yields the fill /
      // is skipped instead of faulting the GPU (the reference raises an IndexError there)
      if (D.kind == RUA_LIST) {
        if (!D.bptr) { if (t < 0) t += S.n_rows; }        // a flat row list wraps negatives like torch's indexing
        else if (b < 0 || b >= S.B) { b = 0; t = -1; }
      }
      const int64_t slen = seq_len(S, b);
      const int64_t dlen = D.kind == RUA_LIST ? slen : seq_len(D, b);
      const int64_t ts = apply_tmap(tmap, targ, t, slen, dlen);
      if (ts >= 0 && ts < slen) other = token_to_row(S, b, ts, slen);
      // metadata that does not match the storage (lengths summing past the payload, a corrupt
      // PackedSequence) must not become an out-of-bounds access: such rows read as padding
      if (other >= S.n_rows) other = -1;
    } else {
      other = pad_row;  // padding row: fill (-1) or a copy of one fixed source row
    }
  }
  (void)SCATTER;
  return mine ? other : -1;
}

// lpr      : lanes (VEC-byte columns) per row = ceil(row_bytes / VEC)
// lp_log2  : log2 of lanes a wave gives one row per instruction (<= 6); rows narrower than
//            1 KiB share a wave instruction (64 >> lp_log2 rows at a time)
// cpr      : 64-lane column chunks per row (1 unless row_bytes > 64*VEC)
// RPT      : destination rows per lane in phase 1 (1; 4 = the narrow-row variant of roll / rev inside one
//            PackedSequence, see below)
// TROWS    : destination rows per workgroup tile (<= MOVE_BLOCK; RPT == 1).  Small tiles in launch order make the
//            chip sweep the destination almost sequentially (see tile_of below and DESIGN.md §4).
// tiles_per_xcd > 0: workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8); give every XCD ONE contiguous
//            span of tiles_per_xcd tiles instead of every eighth tile.
// TAIL8    : VEC == 16, rows end in an 8-byte piece and start on 8-byte boundaries (see above)
template <int VEC, bool SCATTER, bool NT, int RPT = 1, int TROWS = MOVE_TILE, int BLOCK = MOVE_BLOCK, int UNR = UNROLL,
          bool TAIL8 = false>
__global__ __launch_bounds__(BLOCK) void move_rows_kernel(rua_layout D, rua_layout S, int32_t tmap,
                                                              int64_t targ, char* __restrict__ dst,
                                                              const char* __restrict__ src, int64_t row_bytes,
                                                              int64_t lpr, int lp_log2, int cpr, uint4 fillpat,
                                                              int64_t pad_row, int64_t tiles_per_xcd) {
  using V = typename vec_of<VEC>::type;
  constexpr int TILE = TROWS * RPT;
  __shared__ int64_t s_ld[TILE];
  __shared__ int64_t s_st[TILE];

  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
  const int64_t tile0 = tile * TILE;
  const int64_t left = D.n_rows - tile0;
  if (left <= 0 || (tiles_per_xcd > 0 && (int64_t)(blockIdx.x >> 3) >= tiles_per_xcd)) return;
  const int nrows = left < TILE ? (int)left : TILE;

  // ---- phase 1: one lane per destination row
  const bool same_pack = !SCATTER && D.kind == RUA_PACK && S.kind == RUA_PACK && D.bsz && D.boff == S.boff &&
                         D.sorted == S.sorted && D.len_add == 0 && S.len_add == 0 && D.T == S.T;
  if (RPT > 1) {
    // Rows of at most 32 B inside one PackedSequence (the host only picks this variant when `same_pack` holds): a
    // 256-row tile is 8 KiB, and a workgroup spends its life in the two dependent-load searches of phase 1
    // (measured 3.1 TB/s at 32-byte rows).  Each lane therefore takes RPT rows and runs their searches in
    // LOCKSTEP — fixed trip counts, RPT independent loads in flight per step — so the tile is RPT times larger
    // for the same latency.
    int64_t j[RPT], lo[RPT], hi[RPT], t[RPT], r[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) { j[k] = tile0 + threadIdx.x + k * BLOCK; lo[k] = 0; hi[k] = D.T; }
    for (int64_t span = D.T; span > 1; span = (span + 1) >> 1) {     // largest t with boff[t] <= j
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const int64_t mid = (lo[k] + hi[k]) >> 1;
        const bool go = hi[k] - lo[k] > 1;
        const int64_t v = go ? D.boff[mid] : 0;
        if (go) { if (v <= j[k]) lo[k] = mid; else hi[k] = mid; }
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) { t[k] = lo[k]; r[k] = j[k] - D.boff[t[k]]; lo[k] = 0; hi[k] = D.T; }
    for (int64_t span = D.T; span > 0; span >>= 1) {                  // len = #{t : bsz[t] > r}
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const bool go = lo[k] < hi[k];
        const int64_t mid = (lo[k] + hi[k]) >> 1;
        const int64_t v = go ? D.bsz[mid] : 0;
        if (go) { if (v > r[k]) lo[k] = mid + 1; else hi[k] = mid; }
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int i = threadIdx.x + k * BLOCK;
      if (i < nrows) {
        const int64_t len = lo[k];
        const int64_t ts = apply_tmap(tmap, targ, t[k], len, len);
        int64_t other = -1;
        if (ts >= 0 && ts < len) other = S.boff[ts] + r[k];
        if (other >= S.n_rows) other = -1;
        s_ld[i] = other;
        s_st[i] = j[k];
      }
    }
  } else {
    // every wave resolves the (up to) 64 tile rows that sit in its lanes
    const int i = threadIdx.x;
    const int lane1 = threadIdx.x & (RUA_WAVE - 1);
    const int w0 = i - lane1;                                     // first tile row of this wave
    const int nw = nrows - w0 < RUA_WAVE ? nrows - w0 : RUA_WAVE; // rows in this wave (<= 0: none)
    if (nw > 0) {                                                 // wave-uniform
      const int64_t other = resolve_wave_rows<SCATTER>(D, S, tmap, targ, pad_row, tile0 + w0, nw, lane1, same_pack);
      if (i < nrows) {
        const int64_t j = tile0 + i;
        if (SCATTER) { s_ld[i] = j; s_st[i] = other; }   // enumerated rows are the source
        else         { s_ld[i] = other; s_st[i] = j; }   // enumerated rows are the destination
      }
    }
  }
  __syncthreads();

  // ---- phase 2: stream the payload
  const int lane = threadIdx.x & (RUA_WAVE - 1), wave = threadIdx.x >> 6;
  const int rpw = RUA_WAVE >> lp_log2;           // rows per wave instruction
  const int rsub = lane >> lp_log2;              // which of those rows this lane serves
  const int64_t col0 = lane & ((1 << lp_log2) - 1);
  const V fillv = fill_of<VEC>(fillpat);

  for (int g0 = wave; g0 * rpw < nrows; g0 += (BLOCK / RUA_WAVE) * UNR) {
    for (int c = 0; c < cpr; ++c) {
      const int64_t col = col0 + (int64_t)c * RUA_WAVE;
      const bool colok = col < lpr;
      V val[UNR];
      int64_t st[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int r = (g0 + u * (BLOCK / RUA_WAVE)) * rpw + rsub;
        st[u] = -1;
        val[u] = fillv;
        if (colok && r < nrows) {
          const int64_t ld = s_ld[r];
          st[u] = s_st[r];
          if (ld >= 0 && st[u] >= 0) {
            if constexpr (TAIL8) {
              const char* p = src + ld * row_bytes + col * VEC;
              if (col == lpr - 1) {                       // the row's last, 8-byte piece
                const u32x2 h = ld_row<u32x2, NT>(p);
                const u32x4 v2 = {h.x, h.y, 0u, 0u};
                val[u] = v2;
              } else {
                val[u] = ld_row_a8<NT>(p);
              }
            } else {
              val[u] = ld_row<V, NT>(src + ld * row_bytes + col * VEC);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        if (st[u] >= 0) {
          if constexpr (TAIL8) {
            char* p = dst + st[u] * row_bytes + col * VEC;
            if (col == lpr - 1) { u32x2 h = {val[u].x, val[u].y}; st_row<u32x2, NT>(p, h); }
            else st_row_a8<NT>(p, val[u]);
          } else {
            st_row<V, NT>(dst + st[u] * row_bytes + col * VEC, val[u]);
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// [r5] GATHERS of rows that are a multiple of 4 but not of 16 bytes (H = 500 in bf16: 1 000-byte rows; 500-byte rows in
// fp32 ...).  Such rows start off 16-byte boundaries, and a row-granular mover moves them with misaligned 16-byte lanes on
// both sides: 4.0 TB/s for the pack at 1 000-byte rows, 4.3 even for a streaming copy, where 1 024-byte rows move at
// 6.0 - 6.3.  But a tile of consecutive DESTINATION rows is ONE contiguous span of bytes that starts on a 16-byte boundary
// (the tile holds a multiple of 16 rows).  So the tile goes through LDS: every source row is fetched with ALIGNED 16-byte
// loads — the aligned vectors that overlap it, its first and last vector holding a few bytes of its neighbours — and laid
// down in LDS at its own offset in dword pieces; then the whole span is stored with aligned 16-byte lanes.  Fill rows are
// laid down as the pattern.  Both sides of HBM see aligned full lanes; what is off-boundary happens inside LDS.
template <bool NT>
__global__ __launch_bounds__(RUA_BLOCK) void move_rows_span_kernel(rua_layout D, rua_layout S, int32_t tmap, int64_t targ,
                                                                   char* __restrict__ dst, const char* __restrict__ src,
                                                                   int rb, int tile_rows, uint4 fillpat, int64_t pad_row,
                                                                   int64_t tiles_per_xcd) {
  __shared__ int64_t s_ld[RUA_BLOCK];
  __shared__ __attribute__((aligned(16))) uint32_t stage[SPAN_TILE_BYTES / 4];
  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
  const int64_t tile0 = tile * tile_rows;
  const int64_t left = D.n_rows - tile0;
  if (left <= 0 || (tiles_per_xcd > 0 && (int64_t)(blockIdx.x >> 3) >= tiles_per_xcd)) return;
  const int nrows = left < tile_rows ? (int)left : tile_rows;
  const bool same_pack = D.kind == RUA_PACK && S.kind == RUA_PACK && D.bsz && D.boff == S.boff && D.sorted == S.sorted &&
                         D.len_add == 0 && S.len_add == 0 && D.T == S.T;
  {
    const int i = threadIdx.x, lane1 = threadIdx.x & (RUA_WAVE - 1), w0 = i - lane1;
    const int nw = nrows - w0 < RUA_WAVE ? nrows - w0 : RUA_WAVE;
    if (nw > 0) {
      const int64_t other = resolve_wave_rows<false>(D, S, tmap, targ, pad_row, tile0 + w0, nw, lane1, same_pack);
      if (i < nrows) s_ld[i] = other;
    }
  }
  __syncthreads();
  // ---- the rows into LDS: item = (row, aligned 16-byte vector l of the source that overlaps it)
  const int vpr = ((rb + 12) >> 4) + 1;                     // vectors that can overlap a row that starts 0 .. 12 bytes in
  const int n_items = nrows * vpr;
  const uint32_t pat[4] = {fillpat.x, fillpat.y, fillpat.z, fillpat.w};
  constexpr int UN = 4;
  for (int it0 = threadIdx.x; it0 < n_items; it0 += RUA_BLOCK * UN) {
    u32x4 x[UN];
    int k0[UN], base[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int idx = it0 + u * RUA_BLOCK;
      k0[u] = -1000000;                                     // (nothing to lay down)
      if (idx >= n_items) continue;
      const int row = idx / vpr, l = idx - row * vpr;
      const int64_t ld = s_ld[row];
      base[u] = row * rb;
      if (ld < 0) {                                         // a fill row: the pattern, phase = the row's own offset
        if ((l << 4) < rb) { k0[u] = l << 4; x[u] = u32x4{pat[0], pat[1], pat[2], pat[3]}; }
        continue;
      }
      const int64_t A = ld * (int64_t)rb;
      const int shift = (int)(A & 15);
      const int kk = (l << 4) - shift;                      // the vector holds bytes kk .. kk + 15 of the row
      if (kk >= rb || kk + 16 <= 0) continue;
      const char* p = src + (A - shift) + ((int64_t)l << 4);
      if (kk + 16 <= rb || ld + 1 < S.n_rows) {             // (the bytes behind the row belong to the next row: readable)
        x[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)) : *reinterpret_cast<const u32x4*>(p);
      } else {                                              // the storage's last row: stop at its end
        uint32_t w[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; ++q) if (kk + 4 * q < rb) w[q] = reinterpret_cast<const uint32_t*>(p)[q];
        x[u] = u32x4{w[0], w[1], w[2], w[3]};
      }
      k0[u] = kk;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (k0[u] < -16) continue;
      const uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
      if (((k0[u] | rb | base[u]) & 15) == 0) {             // whole vectors (rows of a multiple of 16 bytes: always)
        if (k0[u] >= 0 && k0[u] < rb) *reinterpret_cast<u32x4*>(&stage[(base[u] + k0[u]) >> 2]) = x[u];
      } else if (((k0[u] | rb | base[u]) & 7) == 0) {       // 8-byte pieces (rows of 8 mod 16 bytes: always)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int k = k0[u] + 8 * q;
          if (k >= 0 && k < rb) *reinterpret_cast<u32x2*>(&stage[(base[u] + k) >> 2]) = u32x2{w[2 * q], w[2 * q + 1]};
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0[u] + 4 * q;
          if (k >= 0 && k < rb) stage[(base[u] + k) >> 2] = w[q];
        }
      }
    }
  }
  __syncthreads();
  // ---- the span out: aligned 16-byte lanes
  const int nbytes = nrows * rb;
  char* d = dst + tile0 * (int64_t)rb;
  const int nvec = nbytes >> 4;
  for (int v = threadIdx.x; v < nvec; v += RUA_BLOCK) {
    const u32x4 o = *reinterpret_cast<const u32x4*>(&stage[v << 2]);
    if (NT) __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(d + (v << 4)));
    else *reinterpret_cast<u32x4*>(d + (v << 4)) = o;
  }
  const int tail = (nbytes & 15) >> 2;
  if ((int)threadIdx.x < tail) reinterpret_cast<uint32_t*>(d + (nvec << 4))[threadIdx.x] = stage[(nvec << 2) + threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// [r5] Rows of ONE vector — 1, 2, 4, 8 or 16 bytes: 1-D payloads (int64 token ids, fp32 scalars, bool masks), the
// commonest thing `C.new([...]).left()` is called on.  The generic kernel gives such a row a lane in phase 1 and a lane in
// phase 2 and a workgroup 256 rows: 2 KiB per workgroup at 8-byte rows behind a chain of dependent index loads — 5.8 ms
// for 500 M rows (0.09 T rows/s, 1.4 TB/s at 8 bytes, 0.17 at 1 byte), whatever the width.  Here a lane keeps its row
// from resolution to store (no LDS, no barrier) and has CH rows in flight: a wave takes 64 * CH consecutive enumerated
// rows, chunk by chunk (every chunk one contiguous run of 64 rows on the enumerated side), all CH loads are issued before
// the first store.  Same row maps as the generic kernel (resolve_wave_rows): every layout pair, gather and scatter,
// pad_row.  A gather between a PackedSequence and a batch-major layout still reads one row per cache line this way — that
// pair belongs to the (rank x time) tiles below, which this kernel only replaces when the host withholds the tile table.
template <int VEC, bool SCATTER, bool NT, int CH>
__global__ __launch_bounds__(RUA_BLOCK) void move_rows_narrow_kernel(rua_layout D, rua_layout S, int32_t tmap, int64_t targ,
                                                                     char* __restrict__ dst, const char* __restrict__ src,
                                                                     uint4 fillpat, int64_t pad_row,
                                                                     int64_t tiles_per_xcd) {
  using V = typename vec_of<VEC>::type;
  constexpr int TILE = RUA_BLOCK * CH;
  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
  const int64_t tile0 = tile * TILE;
  if (tile0 >= D.n_rows || (tiles_per_xcd > 0 && (int64_t)(blockIdx.x >> 3) >= tiles_per_xcd)) return;
  const bool same_pack = !SCATTER && D.kind == RUA_PACK && S.kind == RUA_PACK && D.bsz && D.boff == S.boff &&
                         D.sorted == S.sorted && D.len_add == 0 && S.len_add == 0 && D.T == S.T;
  const int lane = threadIdx.x & (RUA_WAVE - 1), wave = threadIdx.x >> 6;
  const int64_t jw = tile0 + (int64_t)wave * (RUA_WAVE * CH);
  const V fillv = fill_of<VEC>(fillpat);
  V val[CH];
  int64_t st[CH];
  WaveWindow ww;
  const bool have_win = jw < D.n_rows && wave_window(D, jw, lane, ww);      // (wave-uniform)
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int64_t jw0 = jw + c * RUA_WAVE;
    const int64_t left = D.n_rows - jw0;
    st[c] = -1;
    val[c] = fillv;
    if (left <= 0) continue;                                          // wave-uniform
    const int nw = left < RUA_WAVE ? (int)left : RUA_WAVE;
    const int64_t other = resolve_wave_rows<SCATTER>(D, S, tmap, targ, pad_row, jw0, nw, lane, same_pack, have_win ? &ww : nullptr);
    if (lane < nw) {
      const int64_t j = jw0 + lane;
      const int64_t ld = SCATTER ? j : other;
      st[c] = SCATTER ? other : j;
      if (ld >= 0 && st[c] >= 0) val[c] = ld_row<V, NT>(src + ld * VEC);
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (st[c] >= 0) st_row<V, NT>(dst + st[c] * VEC, val[c]);
}

// ---------------------------------------------------------------------------------------------
// [r5] Narrow rows between two BATCH-MAJOR layouts (C.left(), L.cat(), C.right(), R.left(), C.roll(s), trunc / head of a
// padded batch ...): a sequence's tokens are one contiguous run of bytes on both sides, so the cast is a SEGMENTED
// MEMCPY — per sequence at most two runs to copy (a roll wraps once) and the rest of the destination's slots to fill —
// and rows stop mattering: a lane moves 16 bytes whatever the row width.  The row kernels give every ROW a lane and its
// own index arithmetic: 6.3 ms for C.left() of 500 M 8-byte rows (1.9 TB/s), 4.2 ms for C.roll.  Here a wave takes
// SEQ_PER_WAVE consecutive sequences (their lengths and offsets arrive in one coalesced load, lane i holding sequence
// i's), and streams every run with 16-byte lanes at whatever dword-aligned address it starts (gfx950 takes a dwordx4
// there), four vectors in flight per lane; runs whose two ends are not a multiple of 4 bytes apart (rows of 1 or 2
// bytes: bool masks, int16) go through a byte shift in registers (copy_bytes_any).  The launcher takes it when no
// sequence can be a large share of the launch (one wave walks a whole sequence).
// A run of bytes copied by NTHR threads with 16-byte lanes, WHATEVER the two addresses' alignment: the destination is
// brought to a dword boundary by a few single bytes, then every lane stores an aligned-to-4 dwordx4 assembled from FIVE
// aligned source dwords shifted by the two addresses' distance mod 4 (v_alignbyte: rows of 1 or 2 bytes, 6, 18 ...),
// or loaded as it is when that distance is zero (rows that are a multiple of 4 bytes).  (Aligning BOTH sides to 16 bytes —
// two aligned loads per lane and a shift — was measured and is slower: C.left() of 8-byte rows 2.3 -> 3.6 ms, r5n.)
template <bool NT, int NTHR>
__device__ __forceinline__ void copy_bytes_any(char* __restrict__ d, const char* __restrict__ s, int64_t nbytes, int tid) {
  if (nbytes <= 0) return;
  int head = (int)((4 - ((uintptr_t)d & 3)) & 3);
  if (head > nbytes) head = (int)nbytes;
  if (tid < head) d[tid] = s[tid];
  d += head; s += head; nbytes -= head;
  const int m = (int)((uintptr_t)s & 3);
  const char* sa = s - m;                                          // dword-aligned; sa + m = s
  const int64_t nvec = nbytes >> 4;
  constexpr int UN = NTHR == RUA_WAVE ? 8 : 4;          // vectors in flight per lane
  for (int64_t v0 = 0; v0 < nvec; v0 += NTHR * UN) {
    u32x4 x[UN];
    uint32_t e[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t v = v0 + u * NTHR + tid;
      e[u] = 0;
      if (v < nvec) {
        x[u] = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(sa + (v << 4)))
                  : *reinterpret_cast<const u32x4_a4*>(sa + (v << 4));
        if (m) e[u] = *reinterpret_cast<const uint32_t*>(sa + (v << 4) + 16);      // (holds bytes of this very run)
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t v = v0 + u * NTHR + tid;
      if (v < nvec) {
        u32x4 o = x[u];
        if (m) {
          o.x = __builtin_amdgcn_alignbyte(x[u].y, x[u].x, m);
          o.y = __builtin_amdgcn_alignbyte(x[u].z, x[u].y, m);
          o.z = __builtin_amdgcn_alignbyte(x[u].w, x[u].z, m);
          o.w = __builtin_amdgcn_alignbyte(e[u], x[u].w, m);
        }
        if (NT) __builtin_nontemporal_store(o, reinterpret_cast<u32x4_a4*>(d + (v << 4)));
        else *reinterpret_cast<u32x4_a4*>(d + (v << 4)) = o;
      }
    }
  }
  const int tail = (int)(nbytes & 15);
  if (tid < tail) d[(nvec << 4) + tid] = s[(nvec << 4) + tid];
}
template <bool NT>
__device__ __forceinline__ void wave_copy_bytes(char* __restrict__ d, const char* __restrict__ s, int64_t nbytes, int lane) {
  copy_bytes_any<NT, RUA_WAVE>(d, s, nbytes, lane);
}
// ... and filled: the pattern repeats every element (1, 2, 4, 8 or 16 bytes) and a run starts on an element boundary, so
// a dword-aligned vector of it is the pattern itself (elements wider than a dword: the run's start is a multiple of the
// element, hence the vector's phase is a multiple of 4 inside the element — rotate by it), single bytes are indexed by
// their address.
template <bool NT>
__device__ __forceinline__ void wave_fill_bytes(char* __restrict__ d, int64_t nbytes, u32x4 pat, int lane) {
  if (nbytes <= 0) return;
  // (byte k of the run holds pattern byte k mod 16: the run starts on an element boundary and 16 is a multiple of it)
  auto pat_byte = [&](int k) -> char {
    const uint32_t w = (k & 8) ? ((k & 4) ? pat.w : pat.z) : ((k & 4) ? pat.y : pat.x);
    return (char)(w >> (8 * (k & 3)));
  };
  int head = (int)((4 - ((uintptr_t)d & 3)) & 3);
  if (head > nbytes) head = (int)nbytes;
  if (lane < head) d[lane] = pat_byte(lane & 15);
  char* d4 = d + head;
  nbytes -= head;
  u32x4 rot = pat;                                                 // the pattern as seen from byte `head` of the run
  if (head) {
    const uint32_t w[4] = {pat.x, pat.y, pat.z, pat.w};
    rot.x = __builtin_amdgcn_alignbyte(w[1], w[0], head);
    rot.y = __builtin_amdgcn_alignbyte(w[2], w[1], head);
    rot.z = __builtin_amdgcn_alignbyte(w[3], w[2], head);
    rot.w = __builtin_amdgcn_alignbyte(w[0], w[3], head);
  }
  const int64_t nvec = nbytes >> 4;
  for (int64_t v = lane; v < nvec; v += RUA_WAVE) {
    if (NT) __builtin_nontemporal_store(rot, reinterpret_cast<u32x4_a4*>(d4 + (v << 4)));
    else *reinterpret_cast<u32x4_a4*>(d4 + (v << 4)) = rot;
  }
  const int tail = (int)(nbytes & 15);
  if (lane < tail) d4[(nvec << 4) + lane] = pat_byte((head + lane) & 15);
}

template <bool NT>
__global__ __launch_bounds__(RUA_BLOCK) void seq_copy_kernel(rua_layout D, rua_layout S, int32_t tmap, int64_t targ,
                                                             char* __restrict__ dst, const char* __restrict__ src,
                                                             int64_t rb, uint4 fillpat, int spw) {
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int64_t wave_id = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b0 = wave_id * spw;
  if (b0 >= D.B) return;                                            // wave-uniform
  const int64_t bl = b0 + lane;
  const bool have = lane < spw && bl < D.B;
  int64_t my_dlen = 0, my_slen = 0, my_dbase = 0, my_sbase = 0;
  if (have) {
    my_dlen = seq_len(D, bl);
    my_slen = bl < S.B ? seq_len(S, bl) : 0;
    if (my_dlen < 0) my_dlen = 0;
    if (my_slen < 0) my_slen = 0;
    my_dbase = token_to_row(D, bl, 0, my_dlen);
    my_sbase = bl < S.B ? token_to_row(S, bl, 0, my_slen) : 0;
  }
  const u32x4 pat = fill_of<16>(fillpat);
  const bool padded = D.kind == RUA_LEFT || D.kind == RUA_RIGHT;
#pragma unroll 1
  for (int i = 0; i < spw; ++i) {
    const int64_t b = b0 + i;
    if (b >= D.B) break;                                            // wave-uniform
    int64_t dlen = __shfl(my_dlen, i, RUA_WAVE), slen = __shfl(my_slen, i, RUA_WAVE);
    const int64_t dbase = __shfl(my_dbase, i, RUA_WAVE), sbase = __shfl(my_sbase, i, RUA_WAVE);
    // metadata that does not match the storage must not become an out-of-bounds access
    if (dbase < 0 || dbase > D.n_rows) continue;
    if (dbase + dlen > D.n_rows) dlen = D.n_rows - dbase;
    if (sbase < 0 || sbase > S.n_rows) slen = 0;
    else if (sbase + slen > S.n_rows) slen = S.n_rows - sbase;
    // destination tokens [lo, hi) come from the source tokens that start at `from`; a roll adds the wrapped run [0, lo)
    int64_t lo = 0, hi = 0, from = 0, wrap_from = -1;
    if (tmap == RUA_T_SHIFT) {
      lo = targ < 0 ? -targ : 0;
      hi = slen - targ < dlen ? slen - targ : dlen;
      if (lo > dlen) lo = dlen;
      if (hi < lo) hi = lo;
      from = lo + targ;
    } else {                                                        // RUA_T_ROLL (the launcher checked dlen == slen)
      const int64_t n = dlen < slen ? dlen : slen;
      int64_t k = 0;
      if (n > 0) { k = targ % n; if (k < 0) k += n; }
      lo = k; hi = n; from = 0; wrap_from = n - k;                  // dst [k, n) <- src [0, n - k);  dst [0, k) <- src [n - k, n)
      dlen = n;
    }
    char* drow = dst + dbase * rb;
    const char* srow = src + sbase * rb;
    if (wrap_from >= 0) { if (lo > 0) wave_copy_bytes<NT>(drow, srow + wrap_from * rb, lo * rb, lane); }
    else if (lo > 0) wave_fill_bytes<NT>(drow, lo * rb, pat, lane);
    if (hi > lo) wave_copy_bytes<NT>(drow + lo * rb, srow + from * rb, (hi - lo) * rb, lane);
    if (dlen > hi) wave_fill_bytes<NT>(drow + hi * rb, (dlen - hi) * rb, pat, lane);
    if (padded) {                                                   // the slots of the sequence that hold no token
      const int64_t slot0 = b * D.T_phys;
      const int64_t dl = __shfl(my_dlen, i, RUA_WAVE);              // (the unclipped length: where the tokens sit)
      int64_t front = dbase - slot0, back0 = dbase + dl;            // LEFT: front = 0; RIGHT: front = T_log - len
      if (front > 0) wave_fill_bytes<NT>(dst + slot0 * rb, front * rb, pat, lane);
      int64_t back = slot0 + D.T_phys - back0;
      if (back0 + back > D.n_rows) back = D.n_rows - back0;
      if (back > 0) wave_fill_bytes<NT>(dst + back0 * rb, back * rb, pat, lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Narrow rows (<= 128 B): C/L/R <-> P is a transpose of the (rank, time) plane — C is contiguous along
// time, P along rank — and a destination-row-major tile makes the other side a one-row-granular gather:
// a 32-byte row out of every 128-byte line, i.e. 4x over-fetch (measured 1.3 TB/s at 32-byte rows).
// Here a tile is TR ranks x TT time steps, so BOTH sides move 16-row runs, and phase 2 walks it in 4x4
// sub-tiles.  (At >= 1 KiB rows the same tiling changes nothing — a row already fills whole lines — so
// wide rows keep the generic kernel.)  Phase 1 needs no search: rank r is live at time t iff r < bsz[t].
constexpr int TR_MAX = 128;       // a tile is (1 << TRL) ranks x (1 << TTL) time steps, TRL = 4 .. 7, TTL = 4 .. 7 (rua_layout::tile_t_log2)
constexpr int TT_MAX = 128;

// [r4] A tile's life is one chain of dependent loads in front of its payload, and eight resident workgroups per CU
// cannot feed the HBM through it when the chain carries 8 KiB (32-byte rows, 16 x 16 tiles: 4.3 TB/s for the pack, 3.6
// for P.cat).  Two changes.  (1) Phase 1 no longer resolves every (rank, time) cell by itself (five loads per cell,
// three of them dependent): a cell's rows are AFFINE in the tile — batch-major row = base[rank] + time, PackedSequence
// row = boff[time] + rank — so sixteen lanes fetch their rank's sequence (sorted -> offset / length) and TT lanes their
// time step's (boff, bsz), and phase 2 computes every row from those two small tables.  (2) The tile grows ALONG TIME
// as rows get narrower (1 << TTL steps, chosen by the host: 64 at <= 16 B, 32 at <= 32 B, 16 at 64 B — 16 KiB of payload
// per chain, eight workgroups per CU), which also makes the batch-major side's runs 1 KiB instead of 512 / 256 B.
// Measured (8 GB payloads, profiles/r04_tile_ab.txt, r03_width_sweep.txt): pack 4.0-4.3 -> 4.9 TB/s at 32-byte rows,
// 3.3 -> 4.9 at 16; P.cat 3.3-3.6 -> 3.9, 3.1 -> 4.2; 64-byte rows unchanged (5.2 / 4.4).  32 KiB tiles and 32 ranks
// per tile: slower.
// (3) [r4, late] LINE-ALIGNED RUNS ON THE BATCH-MAJOR SIDE (P.cat only: see launch_pack_tiles).  A rank's run in a tile
// is TT rows = 1 KiB of one sequence, at whatever 32-byte offset the sequence happens to start: both ends of every run
// were partial 128-byte lines, shared with the neighbouring time chunk's tile — which runs much later, on another CU —
// i.e. over-fetched by the pack and written as partial lines by P.cat.  Measured with all-equal lengths (scripts/exp/aligned_pcat.py, 32-byte rows):
// everything aligned 6.0 / 5.6 TB/s (pack / P.cat); only the PackedSequence's runs misaligned 5.6 / 5.35; only the
// batch-major runs misaligned 5.1 / 4.35; ragged lengths 4.5 / 3.8.  So every rank gets its OWN time origin: with
// R = 128 / row_bytes rows per line and s = (first row of the sequence) mod R, the rank's windows are
// [c TT - s, (c + 1) TT - s) — whole lines on the batch-major side, except where a sequence begins and ends.  The
// PackedSequence side pays: a tile touches TT + R - 1 time steps, and at the R - 1 steps on either edge only some of
// the sixteen ranks (the cheap kind of misalignment, above).  The host builds the tile table for the shifted windows
// (chunk c needs the ranks alive at step c TT - (R - 1)) and says so in rua_layout::tile_t_log2 bits 16..23
// (TILE_SHIFT_MAX, rua_move_plan.h: R <= 8, rows of 16 bytes).
struct TileTables {
  int64_t obase[TR_MAX];  // batch-major storage row of the rank's window start: first row of the sequence - shift + t0
  int64_t olen[TR_MAX];   // the sequence's length (0: no such sequence)
  int shift[TR_MAX];      // the rank's time shift s in [0, R)
  int64_t ofill[TR_MAX];  // padded destination (full-grid tiles): storage row of the sequence's slot 0, -1: no such sequence
  int nlive_t[TR_MAX];    // [r5] steps of the tile the rank's sequence holds a token at: clamp(len - t0, 0, TT), clipped to the storage
  int nlive_r[TT_MAX + TILE_SHIFT_MAX];   // ranks of the tile alive at the step: clamp(bsz - r0, 0, TR), clipped to the storage
  int64_t pboff[TT_MAX + TILE_SHIFT_MAX];  // first PackedSequence row of time step t0 - (R - 1) + k
  int64_t pbsz[TT_MAX + TILE_SHIFT_MAX];   // sequences alive at that step (0 before 0 and past T)
};

template <int TTL, int TRL>
__device__ __forceinline__ void tile_tables(const rua_layout& Pk, const rua_layout& Ot, int64_t tile, TileTables& tb,
                                            int64_t& r0_out, int64_t& t0_out, int R = 1, int64_t phase = 0) {
  constexpr int TT = 1 << TTL, TR = 1 << TRL;
  int64_t lo = 0;
  int64_t r0;
  if (Pk.tile_t_log2 & TILE_FULL_GRID) {
    // [r5] a PADDED destination (P.left() / P.right()): the tiles cover the whole (sequence x step) grid, rank groups
    // fastest — no table: every chunk holds ceil(B / TR) of them — and a cell that holds no token is written as fill
    const int64_t groups = (Pk.B + TR - 1) >> TRL;
    lo = tile / groups;
    r0 = (tile - lo * groups) << TRL;
  } else {
    // which time chunk does this tile belong to?  largest c with tile_start[c] <= tile.  Up to 64 chunks
    // every lane loads one entry and a ballot counts them: ONE load instead of a six-step chain of dependent ones
    int64_t hi = Pk.n_tchunks;
    if (Pk.n_tchunks <= RUA_WAVE) {
      const int lane = threadIdx.x & (RUA_WAVE - 1);
      const int64_t v = lane < Pk.n_tchunks ? Pk.tile_start[lane] : 0x7fffffffffffffffLL;
      lo = (int64_t)__popcll(__ballot(v <= tile)) - 1;
      if (lo < 0) lo = 0;
    } else {
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (Pk.tile_start[mid] <= tile) lo = mid; else hi = mid;
      }
    }
    r0 = (tile - Pk.tile_start[lo]) * TR;
  }
  const int64_t t0 = lo * TT;
  r0_out = r0;
  t0_out = t0;
  for (int i = threadIdx.x; i < TR; i += RUA_BLOCK) {          // the ranks: sequence -> first row, length
    const int64_t r = r0 + i;
    int64_t base = 0, len = 0, slot0 = -1;
    if (r < Pk.B) {
      const int64_t b = Pk.sorted ? Pk.sorted[r] : r;
      if (b >= 0 && b < Ot.B) {
        len = seq_len(Ot, b);
        base = token_to_row(Ot, b, 0, len);
        if (Ot.kind == RUA_LEFT || Ot.kind == RUA_RIGHT) slot0 = b * Ot.T_phys;
      }
    }
    const int s = R > 1 ? (int)((base + phase) & (int64_t)(R - 1)) : 0;
    tb.shift[i] = s;
    tb.obase[i] = base - s + t0;                  // batch-major row of the rank's window start (a whole-line boundary)
    tb.olen[i] = len;
    tb.ofill[i] = slot0;
    int64_t nl = len - t0;                          // (plain windows only: the callers that shift do not read these)
    if (Ot.n_rows - (base + t0) < nl) nl = Ot.n_rows - (base + t0);
    tb.nlive_t[i] = nl < 0 ? 0 : nl > TT ? TT : (int)nl;
  }
  // the time steps t0 - (R - 1) .. t0 + TT - 1 (threads from the far end: the first ones hold a rank already)
  for (int k = RUA_BLOCK - 1 - (int)threadIdx.x; k < TT + R - 1; k += RUA_BLOCK) {
    const int64_t t = t0 - (R - 1) + k;
    const bool ok = t >= 0 && t < Pk.T;
    const int64_t first = ok ? Pk.boff[t] : 0;
    tb.pboff[k] = first;
    tb.pbsz[k] = ok ? Pk.bsz[t] : 0;
    int64_t nl = tb.pbsz[k] - r0;
    if (Pk.n_rows - (first + r0) < nl) nl = Pk.n_rows - (first + r0);
    tb.nlive_r[k] = nl < 0 ? 0 : nl > TR ? TR : (int)nl;
  }
}

// The tile goes through LDS: read in the source's contiguous order, written in the destination's (measured at 32-byte
// rows: pack 3.5 -> 4.0 TB/s against a 4x4 sub-tile walk without staging).  Rows of 128 B and more take the generic
// mover: since round 2 (16 KiB tiles, cooperative row resolution) it is the faster one there — 5.5 / 5.8 TB/s for
// C->P / P->C at 128 B against 5.3 / 5.2 for the tile kernels; at 64 B the tiles win 4.8 to 3.2, at 32 B 3.9 to 1.6
// (a round-2 A/B, profiles/r02_width_sweep.txt).
template <int VEC, bool TO_PACK, int TTL, int TRL>
__global__ __launch_bounds__(RUA_BLOCK) void pack_tile_lds_kernel(rua_layout Pk, rua_layout Ot, char* __restrict__ dst,
                                                              const char* __restrict__ src, int64_t row_bytes,
                                                              int64_t lpr, int64_t tiles_per_xcd, int R, int64_t phase,
                                                              uint4 fillpat) {
  using V = typename vec_of<VEC>::type;
  constexpr int TT = 1 << TTL, TR = 1 << TRL, TILE = TR * TT;
  static_assert(TT <= TT_MAX && TR <= TR_MAX, "TileTables holds the tile's ranks and time steps");
  __shared__ TileTables tb;

  int64_t tile = blockIdx.x;                  // (block-uniform) one contiguous span of tiles per XCD, as in the row mover
  if (tiles_per_xcd > 0) {
    tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= tiles_per_xcd || tile >= Pk.n_tiles) return;
  }
  int64_t r0, t0;
  tile_tables<TTL, TRL>(Pk, Ot, tile, tb, r0, t0, R, phase);
  __syncthreads();

  // ---- phase 2: the tile goes through LDS.  It is read in the SOURCE's contiguous order (consecutive lanes =
  // consecutive 16-byte pieces of consecutive rows of one run) and written in the DESTINATION's contiguous order,
  // so both sides see whole runs per wave instruction (16 ranks on the PackedSequence's side, TT time steps on the
  // batch-major side).  Cell (rank, j), j = the slot in the rank's OWN window (see TileTables): time t = t0 + j - shift[rank],
  // batch-major row obase[rank] + j, PackedSequence row pboff[k] + r0 + rank with k = j - shift[rank] + R - 1 (the step's
  // slot in the tile's table); live iff the sequence has a token there (0 <= t < len) and the rank is alive at the step.
  extern __shared__ __attribute__((aligned(16))) unsigned char s_stage_raw[];
  V* stage = reinterpret_cast<V*>(s_stage_raw);
  // one padding ROW (lpr slots) per rank: the transposed order strides over TT * lpr slots, which would otherwise land
  // the sixteen ranks of a time step on the same LDS banks; with (TT + 1) * lpr the sixteen lanes of a 128-bit LDS
  // pass — ranks x pieces — fall on sixteen different bank groups (a single slot of padding left piece 1 of rank r
  // on the banks of piece 0 of rank r + 1)
#define RUA_SLOT(rank, j, piece) (((((rank) << TTL) | (j)) + (rank)) * (int)lpr + (piece))
#define RUA_CELL(rank, j, k, orow, prow, live)                                                                     \
  const int64_t t_ = t0 + (j) - tb.shift[rank];                                                                    \
  const int64_t orow = tb.obase[rank] + (j), prow = tb.pboff[k] + r0 + (rank);                                     \
  const bool live = t_ >= 0 && t_ < tb.olen[rank] && r0 + (rank) < tb.pbsz[k] && orow < Ot.n_rows && prow < Pk.n_rows
  const int n_major = TILE * (int)lpr;                        // batch-major order: (rank, j), j fastest
  const int n_packed = (TT + R - 1) * TR * (int)lpr;          // PackedSequence order: (k, rank), rank fastest
  if (TO_PACK) {
#pragma unroll 4
    for (int idx = threadIdx.x; idx < n_major; idx += RUA_BLOCK) {
      const int pos = idx / (int)lpr, piece = idx - pos * (int)lpr;
      const int rank = pos >> TTL, j = pos & (TT - 1), k = j - tb.shift[rank] + R - 1;
      RUA_CELL(rank, j, k, orow, prow, live);
      (void)prow;
      if (live) stage[RUA_SLOT(rank, j, piece)] = ld_row<V, false>(src + orow * row_bytes + (int64_t)piece * VEC);
    }
    __syncthreads();
#pragma unroll 4
    for (int idx = threadIdx.x; idx < n_packed; idx += RUA_BLOCK) {
      const int pos = idx / (int)lpr, piece = idx - pos * (int)lpr;
      const int rank = pos & (TR - 1), k = pos >> TRL, j = k - (R - 1) + tb.shift[rank];
      if (j < 0 || j >= TT) continue;
      RUA_CELL(rank, j, k, orow, prow, live);
      (void)orow;
      if (live) st_row<V, false>(dst + prow * row_bytes + (int64_t)piece * VEC, stage[RUA_SLOT(rank, j, piece)]);
    }
  } else {
#pragma unroll 4
    for (int idx = threadIdx.x; idx < n_packed; idx += RUA_BLOCK) {
      const int pos = idx / (int)lpr, piece = idx - pos * (int)lpr;
      const int rank = pos & (TR - 1), k = pos >> TRL, j = k - (R - 1) + tb.shift[rank];
      if (j < 0 || j >= TT) continue;
      RUA_CELL(rank, j, k, orow, prow, live);
      (void)orow;
      if (live) stage[RUA_SLOT(rank, j, piece)] = ld_row<V, false>(src + prow * row_bytes + (int64_t)piece * VEC);
    }
    __syncthreads();
    const bool padded = (Pk.tile_t_log2 & TILE_FULL_GRID) != 0;      // (R == 1 then: the host asks for plain windows)
    const V fillv = fill_of<VEC>(fillpat);
#pragma unroll 4
    for (int idx = threadIdx.x; idx < n_major; idx += RUA_BLOCK) {
      const int pos = idx / (int)lpr, piece = idx - pos * (int)lpr;
      const int rank = pos >> TTL, j = pos & (TT - 1), k = j - tb.shift[rank] + R - 1;
      RUA_CELL(rank, j, k, orow, prow, live);
      (void)prow;
      if (live) st_row<V, false>(dst + orow * row_bytes + (int64_t)piece * VEC, stage[RUA_SLOT(rank, j, piece)]);
      else if (padded && tb.ofill[rank] >= 0 && t_ >= tb.olen[rank] && t_ < Ot.T_phys) {
        // a slot of the padded destination that holds no token: LEFT keeps its tokens in front (slot = step), RIGHT
        // at the end of the logical width (the dead steps len .. T_log - 1 are the slots 0 .. T_log - len - 1 in front)
        const int64_t slot = (Ot.kind == RUA_RIGHT && t_ < Ot.T_log) ? t_ - tb.olen[rank] : t_;
        st_row<V, false>(dst + (tb.ofill[rank] + slot) * row_bytes + (int64_t)piece * VEC, fillv);
      }
    }
  }
#undef RUA_CELL
#undef RUA_SLOT
}

// [r5] The same transpose for rows of ONE 8- or 4-byte vector (1-D int64 / fp32 payloads), SIXTEEN BYTES PER LANE.  At these
// widths the kernel above is bound by instructions, not bytes: a lane moves one row per trip (a global load, an LDS write,
// an LDS read, a global store and ~60 instructions of cell arithmetic for 8 bytes) — 2.5 ms for 500 M 8-byte rows,
// 2.0 ms for as many 4-byte rows.  Here a lane takes CPL = 16 / RB consecutive cells along the side's CONTIGUOUS axis — steps
// of one rank on the batch-major side, ranks of one step on the PackedSequence's — as one 16-byte global access (any
// dword-aligned address will do on gfx950) and CPL row-sized LDS accesses; a group that straddles the end of a sequence
// or of a time step falls back to its cells one by one.  Tiles: 32 ranks x 64 steps (8-byte rows), 64 x 64 (4-byte).
template <int RB, bool TO_PACK, int TTL, int TRL>
__global__ __launch_bounds__(RUA_BLOCK) void pack_tile_vec_kernel(rua_layout Pk, rua_layout Ot, char* __restrict__ dst,
                                                                  const char* __restrict__ src, int64_t tiles_per_xcd,
                                                                  uint4 fillpat) {
  using E = typename vec_of<RB>::type;
  constexpr int CPL = 16 / RB, TT = 1 << TTL, TR = 1 << TRL;
  constexpr int CPL_LOG2 = RB == 16 ? 0 : RB == 8 ? 1 : 2;
  constexpr int JG_LOG2 = TTL - CPL_LOG2, RG_LOG2 = TRL - CPL_LOG2;     // groups per rank / per step
  static_assert(RB == 16 || RB == 8 || RB == 4, "rows of one 16-, 8- or 4-byte vector");
  union Vec { u32x4 v; E e[CPL]; };
  __shared__ TileTables tb;
  __shared__ E stage[TR * (TT + 1)];             // one padding cell per rank: the transposed walk strides over TT + 1 cells
  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) {
    tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= tiles_per_xcd || tile >= Pk.n_tiles) return;
  }
  int64_t r0, t0;
  tile_tables<TTL, TRL>(Pk, Ot, tile, tb, r0, t0);
  __syncthreads();
  const bool padded = (Pk.tile_t_log2 & TILE_FULL_GRID) != 0;
  Vec fillv;
  fillv.v = fill_of<16>(fillpat);
  // cell (rank, j): step t0 + j of the rank's sequence; batch-major row obase[rank] + j, PackedSequence row pboff[j] + r0 + rank
#define RUA_LIVE(rank, j) ((j) < tb.nlive_t[rank] && (rank) < tb.nlive_r[j])
#define RUA_STG(rank, j) stage[(rank) * (TT + 1) + (j)]
  // ---- the batch-major side: a group = CPL consecutive steps of one rank
  auto major_pass = [&](auto&& both, auto&& one) {
    for (int idx = threadIdx.x; idx < (TR << JG_LOG2); idx += RUA_BLOCK) {
      const int rank = idx >> JG_LOG2, j = (idx & ((1 << JG_LOG2) - 1)) * CPL;
      bool all = true;
#pragma unroll
      for (int c = 0; c < CPL; ++c) all = all && RUA_LIVE(rank, j + c);
      if (all) both(rank, j);
      else {
#pragma unroll
        for (int c = 0; c < CPL; ++c) one(rank, j + c, RUA_LIVE(rank, j + c));
      }
    }
  };
  // ---- the PackedSequence's side: a group = CPL consecutive ranks of one step
  auto packed_pass = [&](auto&& both, auto&& one) {
    for (int idx = threadIdx.x; idx < (TT << RG_LOG2); idx += RUA_BLOCK) {
      const int j = idx >> RG_LOG2, rank = (idx & ((1 << RG_LOG2) - 1)) * CPL;
      bool all = true;
#pragma unroll
      for (int c = 0; c < CPL; ++c) all = all && RUA_LIVE(rank + c, j);
      if (all) both(rank, j);
      else {
#pragma unroll
        for (int c = 0; c < CPL; ++c) one(rank + c, j, RUA_LIVE(rank + c, j));
      }
    }
  };
  if (TO_PACK) {
    major_pass(
        [&](int rank, int j) {
          Vec v;
          v.v = *reinterpret_cast<const u32x4_a4*>(src + (tb.obase[rank] + j) * RB);
#pragma unroll
          for (int c = 0; c < CPL; ++c) RUA_STG(rank, j + c) = v.e[c];
        },
        [&](int rank, int j, bool live) {
          if (live) RUA_STG(rank, j) = *reinterpret_cast<const E*>(src + (tb.obase[rank] + j) * RB);
        });
    __syncthreads();
    packed_pass(
        [&](int rank, int j) {
          Vec v;
#pragma unroll
          for (int c = 0; c < CPL; ++c) v.e[c] = RUA_STG(rank + c, j);
          *reinterpret_cast<u32x4_a4*>(dst + (tb.pboff[j] + r0 + rank) * RB) = v.v;
        },
        [&](int rank, int j, bool live) {
          if (live) *reinterpret_cast<E*>(dst + (tb.pboff[j] + r0 + rank) * RB) = RUA_STG(rank, j);
        });
  } else {
    packed_pass(
        [&](int rank, int j) {
          Vec v;
          v.v = *reinterpret_cast<const u32x4_a4*>(src + (tb.pboff[j] + r0 + rank) * RB);
#pragma unroll
          for (int c = 0; c < CPL; ++c) RUA_STG(rank + c, j) = v.e[c];
        },
        [&](int rank, int j, bool live) {
          if (live) RUA_STG(rank, j) = *reinterpret_cast<const E*>(src + (tb.pboff[j] + r0 + rank) * RB);
        });
    __syncthreads();
    major_pass(
        [&](int rank, int j) {
          Vec v;
#pragma unroll
          for (int c = 0; c < CPL; ++c) v.e[c] = RUA_STG(rank, j + c);
          *reinterpret_cast<u32x4_a4*>(dst + (tb.obase[rank] + j) * RB) = v.v;
        },
        [&](int rank, int j, bool live) {
          if (live) {
            *reinterpret_cast<E*>(dst + (tb.obase[rank] + j) * RB) = RUA_STG(rank, j);
          } else if (padded && tb.ofill[rank] >= 0 && t0 + j >= tb.olen[rank] && t0 + j < Ot.T_phys) {
            // a slot of the padded destination that holds no token (see pack_tile_lds_kernel)
            const int64_t t_ = t0 + j;
            const int64_t slot = (Ot.kind == RUA_RIGHT && t_ < Ot.T_log) ? t_ - tb.olen[rank] : t_;
            *reinterpret_cast<E*>(dst + (tb.ofill[rank] + slot) * RB) = fillv.e[0];
          }
        });
  }
#undef RUA_STG
#undef RUA_LIVE
}

// roll / rev INSIDE one PackedSequence at rows of <= 32 bytes, on the same (rank x time) tiles: both sides are in the
// PackedSequence's own order (runs of sixteen ranks), so nothing is transposed and nothing is staged — a cell's source
// row is boff[t'] + rank with t' = the token map of t under the rank's length.  The generic mover's variant for these
// rows (four rows per lane, two 10-step binary searches in lockstep) spends its life in ~20 dependent loads per tile;
// here the chain is tile_start -> (sorted -> lens | boff, bsz of the tile's steps) -> boff[t'] -> payload.
template <int VEC, int TTL>
__global__ __launch_bounds__(RUA_BLOCK) void pack_roll_tile_kernel(rua_layout Pk, int32_t tmap, int64_t targ,
                                                               char* __restrict__ dst, const char* __restrict__ src,
                                                               int64_t row_bytes, int64_t lpr, uint4 fillpat,
                                                               int64_t tiles_per_xcd) {
  using V = typename vec_of<VEC>::type;
  constexpr int TT = 1 << TTL, TR = 16, TILE = TR * TT;
  __shared__ TileTables tb;
  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) {
    tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= tiles_per_xcd || tile >= Pk.n_tiles) return;
  }
  int64_t r0, t0;                                  // (no shift here: both sides are the PackedSequence's own runs, so
  tile_tables<TTL, 4>(Pk, Pk, tile, tb, r0, t0);   //  pboff / pbsz [time] are those of step t0 + time, olen[rank] the length)
  __syncthreads();
  const V fillv = fill_of<VEC>(fillpat);
  const int n_pieces = TILE * (int)lpr;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < n_pieces; idx += RUA_BLOCK) {
    const int pos = idx / (int)lpr, piece = idx - pos * (int)lpr;
    const int rank = pos & (TR - 1), time = pos >> 4;
    const int64_t len = tb.olen[rank];
    if (t0 + time < len && r0 + rank < tb.pbsz[time]) {
      const int64_t t = t0 + time;
      const int64_t ts = apply_tmap(tmap, targ, t, len, len);
      const int64_t drow = tb.pboff[time] + r0 + rank;
      V val = fillv;
      if (ts >= 0 && ts < len) {
        const int64_t srow = Pk.boff[ts] + r0 + rank;
        if (srow < Pk.n_rows) val = ld_row<V, false>(src + srow * row_bytes + (int64_t)piece * VEC);
      }
      if (drow < Pk.n_rows) st_row<V, false>(dst + drow * row_bytes + (int64_t)piece * VEC, val);
    }
  }
}

// [r5] roll INSIDE one PackedSequence at narrow rows, time step by time step.  out[boff[t] + r] = in[boff[ts] + r] with
// ts = (t - s) mod len_r: for every rank that does not wrap at step t, ts = t - s is the SAME step, and those ranks are a
// prefix [0, bsz[max(t, ts)]) — so a step's rows are ONE contiguous run copied from ONE contiguous run, plus the few
// ranks that wrap (those whose sequence ends between the two steps; all ranks of the first |s| steps), which are
// gathered row by row.  A tile = one time step x (16 KiB / row bytes) ranks (the host's table: rua_layout::tile_start
// with TILE_STEP_ROWS set), moved with 16 bytes per lane whatever the row width.  The row kernels resolve every row by
// itself: 5.2 ms for 500 M 8-byte rows (1.5 TB/s).
template <bool NT>
__global__ __launch_bounds__(RUA_BLOCK) void pack_roll_steps_kernel(rua_layout Pk, int64_t shift, char* __restrict__ dst,
                                                                    const char* __restrict__ src, int64_t rb, int trl,
                                                                    int64_t tiles_per_xcd) {
  int64_t tile = blockIdx.x;
  if (tiles_per_xcd > 0) {
    tile = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= tiles_per_xcd) return;
  }
  if (tile >= Pk.n_tiles) return;
  int64_t t = 0, hi = Pk.n_tchunks;                       // largest t with tile_start[t] <= tile (block-uniform)
  while (hi - t > 1) {
    const int64_t mid = (t + hi) >> 1;
    if (Pk.tile_start[mid] <= tile) t = mid; else hi = mid;
  }
  const int64_t r0 = (tile - Pk.tile_start[t]) << trl;
  int64_t n = Pk.bsz[t] - r0;
  if (n > ((int64_t)1 << trl)) n = (int64_t)1 << trl;
  const int64_t drow0 = Pk.boff[t] + r0;
  if (n <= 0 || drow0 + n > Pk.n_rows) return;
  // the ranks that do not wrap: alive at step ts = t - shift as well (a prefix of the ranks)
  const int64_t ts = t - shift;
  int64_t nd = 0, srow0 = 0;
  if (ts >= 0 && ts < Pk.T) {
    nd = Pk.bsz[ts] - r0;
    if (nd > n) nd = n;
    if (nd < 0) nd = 0;
    srow0 = Pk.boff[ts] + r0;
    if (srow0 + nd > Pk.n_rows) nd = 0;
  }
  if (nd > 0) copy_bytes_any<NT, RUA_BLOCK>(dst + drow0 * rb, src + srow0 * rb, nd * rb, threadIdx.x);
  // the ranks that wrap at this step, one row per thread
  const bool dw4 = (rb & 3) == 0 && (((uintptr_t)dst | (uintptr_t)src) & 3) == 0;
  for (int64_t i = nd + threadIdx.x; i < n; i += RUA_BLOCK) {
    const int64_t r = r0 + i;
    int64_t lo = 0, hh = Pk.T;                             // len = #{t : bsz[t] > r}
    while (lo < hh) {
      const int64_t mid = (lo + hh) >> 1;
      if (Pk.bsz[mid] > r) lo = mid + 1; else hh = mid;
    }
    const int64_t tsr = apply_tmap(RUA_T_ROLL, shift, t, lo, lo);
    if (tsr < 0 || tsr >= lo) continue;
    const int64_t srow = Pk.boff[tsr] + r;
    if (srow >= Pk.n_rows) continue;
    const char* sp = src + srow * rb;
    char* dp = dst + (drow0 + i) * rb;
    if (dw4) { for (int w = 0; w < (int)(rb >> 2); ++w) reinterpret_cast<uint32_t*>(dp)[w] = reinterpret_cast<const uint32_t*>(sp)[w]; }
    else { for (int w = 0; w < (int)rb; ++w) dp[w] = sp[w]; }
  }
}

extern std::atomic<int> g_trace_on;        // the dispatch trace (rua_reduce.hip)
void trace_add(const char* rec);
static inline bool tracing() { return g_trace_on.load(std::memory_order_relaxed) != 0; }

// ---- the launcher: a plan (rua_move_plan.h) says WHAT to launch; these helpers turn its run-time values into the
// kernels' template arguments, one compile-time value per generic lambda — the instantiations that exist, no more.
template <int V> using int_c = std::integral_constant<int, V>;
#define RUA_V(x) decltype(x)::value
template <typename F> static void with_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
template <typename F> static void with_vec(int vec, F&& f) {
  switch (vec) { case 16: return f(int_c<16>{}); case 8: return f(int_c<8>{}); case 4: return f(int_c<4>{}); case 2: return f(int_c<2>{}); }
  f(int_c<1>{});
}
// rows per tile of move_rows_kernel: 16-byte lanes get every size (FINE); the narrower lanes and the tail form 16 / 64 / 256
template <bool FINE, typename F> static void with_tile_rows(int rows, F&& f) {
  if constexpr (FINE)
    switch (rows) { case 4: return f(int_c<4>{}); case 8: return f(int_c<8>{}); case 32: return f(int_c<32>{}); case 128: return f(int_c<128>{}); }
  switch (rows) { case 16: return f(int_c<16>{}); case 64: return f(int_c<64>{}); default: return f(int_c<MOVE_TILE>{}); }
}
template <typename F> static void with_ttl(int ttl, F&& f) {       // 16 / 32 / 64 time steps per tile
  switch (ttl) { case 4: return f(int_c<4>{}); case 5: return f(int_c<5>{}); default: return f(int_c<6>{}); }
}
// the (VEC, TTL, TRL) of pack_tile_lds_kernel: 16 ranks at any width; 64 x 128 (2-byte rows), 128 x 128 (1) ...
template <typename F> static void with_lds_tile(int vec, int ttl, int trl, F&& f) {
  if (trl == 6) return f(int_c<2>{}, int_c<7>{}, int_c<6>{});
  if (trl == 7) return f(int_c<1>{}, int_c<7>{}, int_c<7>{});
  with_vec(vec, [&](auto v) { with_ttl(ttl, [&](auto tt) { f(v, tt, int_c<4>{}); }); });
}
// ... and the (RB, TTL, TRL) of pack_tile_vec_kernel (tile_shape_narrow, and 16-byte rows into a PackedSequence)
template <typename F> static void with_vec_tile(int vec, int ttl, F&& f) {
  if (vec == 16) return f(int_c<16>{}, int_c<6>{}, int_c<4>{});
  if (vec == 8) return ttl == 7 ? f(int_c<8>{}, int_c<7>{}, int_c<4>{}) : f(int_c<8>{}, int_c<6>{}, int_c<5>{});
  return ttl == 7 ? f(int_c<4>{}, int_c<7>{}, int_c<5>{}) : f(int_c<4>{}, int_c<6>{}, int_c<6>{});
}

static int launch_move_rows(const MoveRowsPlan& P, hipStream_t s, const rua_layout& D, const rua_layout& S, int32_t tmap,
                            int64_t targ, char* dst, const char* src, int64_t row_bytes, const void* fill16, int64_t pad_row) {
  const uint32_t* f16 = (const uint32_t*)fill16;
  const uint4 fp = f16 ? make_uint4(f16[0], f16[1], f16[2], f16[3]) : make_uint4(0, 0, 0, 0);
  const dim3 g(P.grid), b(P.block);
  const rua_layout &Pk = P.to_pack ? D : S, &Ot = P.to_pack ? S : D;     // the tile kernels: the PackedSequence and its other side
  switch (P.form) {
    case MOVE_TILES_LDS:
      with_bool(P.to_pack, [&](auto tp) { with_lds_tile(P.vec, P.ttl, P.trl, [&](auto v, auto tt, auto tr) {
        hipLaunchKernelGGL((pack_tile_lds_kernel<RUA_V(v), RUA_V(tp), RUA_V(tt), RUA_V(tr)>), g, b, (size_t)P.lds, s, Pk, Ot,
                           dst, src, row_bytes, P.lpr, P.per_xcd, P.R, P.phase, fp);
      }); }); break;
    case MOVE_TILES_VEC:
      with_bool(P.to_pack, [&](auto tp) { with_vec_tile(P.vec, P.ttl, [&](auto v, auto tt, auto tr) {
        hipLaunchKernelGGL((pack_tile_vec_kernel<RUA_V(v), RUA_V(tp), RUA_V(tt), RUA_V(tr)>), g, b, 0, s, Pk, Ot, dst, src, P.per_xcd, fp);
      }); }); break;
    case MOVE_ROLL_STEPS:
      with_bool(P.nt, [&](auto nt) { hipLaunchKernelGGL(pack_roll_steps_kernel<RUA_V(nt)>, g, b, 0, s, D, targ, dst, src, row_bytes, P.trl, P.per_xcd); }); break;
    case MOVE_SEQ_COPY:
      with_bool(P.nt, [&](auto nt) { hipLaunchKernelGGL(seq_copy_kernel<RUA_V(nt)>, g, b, 0, s, D, S, tmap, targ, dst, src, row_bytes, fp, P.spw); }); break;
    case MOVE_NARROW:
      with_vec(P.vec, [&](auto v) { with_bool(P.scatter, [&](auto sc) { with_bool(P.nt, [&](auto nt) {
        hipLaunchKernelGGL((move_rows_narrow_kernel<RUA_V(v), RUA_V(sc), RUA_V(nt), NARROW_CH>), g, b, 0, s, D, S, tmap, targ, dst, src, fp, pad_row, P.per_xcd);
      }); }); }); break;
    case MOVE_ROLL_TILES:
      with_ttl(P.ttl, [&](auto tt) { hipLaunchKernelGGL((pack_roll_tile_kernel<16, RUA_V(tt)>), g, b, 0, s, D, tmap, targ, dst, src, row_bytes, P.lpr, fp, P.per_xcd); }); break;
    case MOVE_SPAN:
      with_bool(P.nt, [&](auto nt) {
        hipLaunchKernelGGL(move_rows_span_kernel<RUA_V(nt)>, g, b, 0, s, D, S, tmap, targ, dst, src, (int)row_bytes, P.tile_rows, fp, pad_row, P.per_xcd);
      }); break;
    case MOVE_ROWS:
      with_bool(P.nt, [&](auto nt) {
        auto go = [&](auto v, auto sc, auto rpt, auto tr, auto t8) {
          hipLaunchKernelGGL((move_rows_kernel<RUA_V(v), RUA_V(sc), RUA_V(nt), RUA_V(rpt), RUA_V(tr), MOVE_BLOCK, UNROLL, RUA_V(t8)>),
                             g, b, 0, s, D, S, tmap, targ, dst, src, row_bytes, P.lpr, P.lp_log2, P.cpr, fp, pad_row, P.per_xcd);
        };
        if (P.rpt > 1) return go(int_c<16>{}, std::false_type{}, int_c<NARROW_RPT>{}, int_c<MOVE_TILE>{}, std::false_type{});
        with_bool(P.scatter, [&](auto sc) {
          if (P.tail8) return with_tile_rows<false>(P.tile_rows, [&](auto tr) { go(int_c<16>{}, sc, int_c<1>{}, tr, std::true_type{}); });
          with_vec(P.vec, [&](auto v) { with_tile_rows<RUA_V(v) == 16>(P.tile_rows, [&](auto tr) { go(v, sc, int_c<1>{}, tr, std::false_type{}); }); });
        });
      }); break;
  }
  return (int)hipGetLastError();
}

// ONE record per plan: the kernel family, its template arguments as launch_move_rows instantiates them, the geometry
// and the run-time arguments that are the plan's.  The trace and rua_debug_move_plan both print through it.
static void format_move_plan(const MoveRowsPlan& P, char* rec, size_t cap) {
  const long long px = P.per_xcd, lpr = P.lpr;
  rec[0] = 0;
  switch (P.form) {
    case MOVE_TILES_LDS:
      snprintf(rec, cap, "pack_tile_lds_kernel VEC=%d TO_PACK=%d TTL=%d TRL=%d grid=%u per_xcd=%lld lds=%d lpr=%lld R=%d phase=%lld",
               P.vec, (int)P.to_pack, P.ttl, P.trl, P.grid, px, P.lds, lpr, P.R, (long long)P.phase); break;
    case MOVE_TILES_VEC:
      snprintf(rec, cap, "pack_tile_vec_kernel RB=%d TO_PACK=%d TTL=%d TRL=%d grid=%u per_xcd=%lld", P.vec, (int)P.to_pack, P.ttl, P.trl, P.grid, px); break;
    case MOVE_ROLL_STEPS: snprintf(rec, cap, "pack_roll_steps_kernel NT=%d grid=%u per_xcd=%lld trl=%d", (int)P.nt, P.grid, px, P.trl); break;
    case MOVE_SEQ_COPY: snprintf(rec, cap, "seq_copy_kernel NT=%d grid=%u spw=%d", (int)P.nt, P.grid, P.spw); break;
    case MOVE_NARROW:
      snprintf(rec, cap, "move_rows_narrow_kernel VEC=%d SCATTER=%d NT=%d CH=%d grid=%u per_xcd=%lld", P.vec, (int)P.scatter, (int)P.nt, NARROW_CH, P.grid, px); break;
    case MOVE_ROLL_TILES: snprintf(rec, cap, "pack_roll_tile_kernel VEC=16 TTL=%d grid=%u per_xcd=%lld lpr=%lld", P.ttl, P.grid, px, lpr); break;
    case MOVE_SPAN: snprintf(rec, cap, "move_rows_span_kernel NT=%d grid=%u per_xcd=%lld tile_rows=%d", (int)P.nt, P.grid, px, P.tile_rows); break;
    case MOVE_ROWS:
      snprintf(rec, cap, "move_rows_kernel VEC=%d SCATTER=%d NT=%d RPT=%d TROWS=%d TAIL8=%d grid=%u per_xcd=%lld lpr=%lld lp_log2=%d cpr=%d",
               P.vec, (int)P.scatter, (int)P.nt, P.rpt, P.tile_rows, (int)P.tail8, P.grid, px, lpr, P.lp_log2, P.cpr); break;
  }
}

// ---------------------------------------------------------------------------------------------
// Backward of a row scatter rows_of(src)[list] = value  (rua_setitem_backward, include/rua.h): gather-and-zero.
// A wave takes 64 consecutive list entries; each lane resolves ONE of them into a storage row of `src` with the mover's own
// resolve_wave_rows<true> (a LIST layout takes none of its cooperative searches: every lane reads its own pair and maps it —
// exactly the rows the scatter wrote, -1 for an entry that names no token); then the wave walks the 64 rows, UNR row groups in
// flight, the rows handed from lane to lane by shuffles (no LDS, no barrier).  Per entry j with row r:
//   grad_value[j] = grad[r] (zeros when r < 0)      and      grad_raw[r] = 0.
// `grad` is only read and `grad_raw` only written, so repeated rows are race-free (two lanes may store the same zeros)
// and the result does not depend on the order of the waves.  The stores to grad_value are contiguous per wave (64 rows).
constexpr int SETITEM_BWD_UNROLL = 4;

template <int VEC, bool NT, bool TAIL8>
__global__ __launch_bounds__(RUA_BLOCK) void setitem_backward_kernel(rua_layout D, rua_layout S,
                                                                     const char* __restrict__ grad,
                                                                     char* __restrict__ gval, char* __restrict__ graw,
                                                                     int64_t row_bytes, int64_t lpr, int lp_log2, int cpr) {
  using V = typename vec_of<VEC>::type;
  constexpr int UNR = SETITEM_BWD_UNROLL;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int64_t wave_id = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t jw0 = wave_id * RUA_WAVE;
  const int64_t left = D.n_rows - jw0;
  if (left <= 0) return;                                             // wave-uniform
  const int nw = left < RUA_WAVE ? (int)left : RUA_WAVE;
  const int64_t mine = resolve_wave_rows<true>(D, S, RUA_T_SHIFT, 0, -1, jw0, nw, lane, false);

  const int rpw = RUA_WAVE >> lp_log2;           // rows per wave instruction
  const int rsub = lane >> lp_log2;              // which of those rows this lane serves
  const int64_t col0 = lane & ((1 << lp_log2) - 1);
  const V zero = fill_of<VEC>(make_uint4(0, 0, 0, 0));
  for (int g0 = 0; g0 * rpw < nw; g0 += UNR) {                       // wave-uniform trip counts: every lane shuffles
    int64_t row[UNR];
    int ent[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int e = (g0 + u) * rpw + rsub;
      const int64_t r = __shfl(mine, e & (RUA_WAVE - 1), RUA_WAVE);
      ent[u] = e < nw ? e : -1;
      row[u] = e < nw ? r : -1;
    }
    for (int c = 0; c < cpr; ++c) {
      const int64_t col = col0 + (int64_t)c * RUA_WAVE;
      if (col >= lpr) continue;
      const bool last8 = TAIL8 && col == lpr - 1;                    // the row's last, 8-byte piece
      V val[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        val[u] = zero;
        if (ent[u] >= 0 && row[u] >= 0 && gval) {
          const char* p = grad + row[u] * row_bytes + col * VEC;
          if constexpr (TAIL8) {
            if (last8) {
              const u32x2 h = ld_row<u32x2, NT>(p);
              const u32x4 v2 = {h.x, h.y, 0u, 0u};
              val[u] = v2;
            } else {
              val[u] = ld_row_a8<NT>(p);
            }
          } else {
            val[u] = ld_row<V, NT>(p);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (ent[u] < 0) continue;
        if (gval) {
          char* p = gval + (jw0 + ent[u]) * row_bytes + col * VEC;
          if constexpr (TAIL8) {
            if (last8) { u32x2 h = {val[u].x, val[u].y}; st_row<u32x2, NT>(p, h); }
            else st_row_a8<NT>(p, val[u]);
          } else {
            st_row<V, NT>(p, val[u]);
          }
        }
        if (graw && row[u] >= 0) {
          char* p = graw + row[u] * row_bytes + col * VEC;
          if constexpr (TAIL8) {
            if (last8) { u32x2 h = {0u, 0u}; st_row<u32x2, NT>(p, h); }
            else st_row_a8<NT>(p, zero);
          } else {
            st_row<V, NT>(p, zero);
          }
        }
      }
    }
  }
}

static int launch_setitem_backward(const SetitemBackwardPlan& P, hipStream_t s, const rua_layout& D, const rua_layout& S,
                                   const char* grad, char* gval, char* graw, int64_t row_bytes) {
  if (tracing()) {
    char rec[160];
    snprintf(rec, sizeof rec, "setitem_backward_kernel VEC=%d NT=%d TAIL8=%d value=%d raw=%d", P.vec, (int)P.nt, (int)P.tail8, gval != nullptr, graw != nullptr);
    trace_add(rec);
  }
  const dim3 g(P.grid), b(RUA_BLOCK);
  with_bool(P.nt, [&](auto nt) {
    auto go = [&](auto v, auto t8) {
      hipLaunchKernelGGL((setitem_backward_kernel<RUA_V(v), RUA_V(nt), RUA_V(t8)>), g, b, 0, s, D, S, grad, gval, graw, row_bytes,
                         P.lpr, P.lp_log2, P.cpr);
    };
    if (P.tail8) return go(int_c<16>{}, std::true_type{});
    with_vec(P.vec, [&](auto v) { go(v, std::false_type{}); });
  });
  return (int)hipGetLastError();
}

// `nbytes` from src to dst through the row mover's own streaming geometry: the bytes seen as ONE sequence of 1-KiB rows
// (what C.roll(0) launches at the north-star shape: 16-row tiles in destination order, an XCD span on big launches),
// and the last, shorter piece as a row of its own.
static int stream_copy(void* dst, const void* src, int64_t nbytes, void* stream) {
  auto flat = [](int64_t rows) {
    rua_layout L = {};
    L.kind = RUA_LEFT; L.n_rows = rows; L.B = 1; L.T_phys = rows; L.T_log = rows; L.len_add = rows;
    return L;
  };
  const int64_t rows = nbytes / COPY_ROW_BYTES, tail = nbytes - rows * COPY_ROW_BYTES;
  if (rows > 0) {
    const rua_layout L = flat(rows);
    const int e = rua_move_rows(&L, &L, RUA_T_SHIFT, 0, dst, src, COPY_ROW_BYTES, nullptr, -1, 0, stream);
    if (e) return e;
  }
  if (tail > 0) {
    const rua_layout L = flat(1);
    return rua_move_rows(&L, &L, RUA_T_SHIFT, 0, (char*)dst + rows * COPY_ROW_BYTES, (const char*)src + rows * COPY_ROW_BYTES, tail,
                         nullptr, -1, 0, stream);
  }
  return 0;
}

}  // namespace rua

using namespace rua;

// plan, trace if on, launch
extern "C" int rua_move_rows(const rua_layout* dst, const rua_layout* src, int32_t tmap, int64_t tmap_arg, void* dst_data,
                             const void* src_data, int64_t row_bytes, const void* fill16, int64_t pad_row, int32_t flags,
                             void* stream) {
  const MoveRowsPlan P = plan_move_rows(dst, src, tmap, tmap_arg, (uintptr_t)dst_data, (uintptr_t)src_data, row_bytes, pad_row, flags);
  if (P.err || P.form == MOVE_NONE) return P.err;
  if (tracing()) { char rec[256]; format_move_plan(P, rec, sizeof rec); trace_add(rec); }
  return launch_move_rows(P, (hipStream_t)stream, *dst, *src, tmap, tmap_arg, (char*)dst_data, (const char*)src_data, row_bytes,
                          fill16, pad_row);
}

// the same validation, plan and record, and no launch: the payload ADDRESSES stand in for the pointers
extern "C" int64_t rua_debug_move_plan(const rua_layout* dst, const rua_layout* src, int32_t tmap, int64_t tmap_arg,
                                       uint64_t dst_addr, uint64_t src_addr, int64_t row_bytes, int64_t pad_row, int32_t flags,
                                       char* buf, int64_t cap) {
  const MoveRowsPlan P = plan_move_rows(dst, src, tmap, tmap_arg, (uintptr_t)dst_addr, (uintptr_t)src_addr, row_bytes, pad_row, flags);
  if (P.err) return P.err;
  char rec[256];
  format_move_plan(P, rec, sizeof rec);
  const int64_t n = (int64_t)strlen(rec);
  if (!buf || n > cap) return RUA_ERANGE;
  memcpy(buf, rec, (size_t)n);
  return n;
}

extern "C" int rua_setitem_backward(const rua_layout* list, const rua_layout* src, const void* grad, void* grad_value,
                                    void* grad_raw, int64_t row_bytes, int32_t flags, void* stream) {
  int e;
  if (!list || list->kind != RUA_LIST) return RUA_EINVAL;
  if ((e = check_layout(list, true)) != 0 || (e = check_layout(src, false)) != 0) return e;
  if (row_bytes < 0 || (flags & ~(RUA_MOVE_NT_ON | RUA_MOVE_NT_OFF)) != 0) return RUA_EINVAL;
  if (grad_raw && grad_raw == grad) return RUA_EINVAL;
  if (!grad && list->n_rows > 0) return RUA_EINVAL;
  if (row_bytes == 0 || (!grad_value && !grad_raw)) return 0;
  if (grad_raw && src->n_rows > 0) {
    // every row nobody names is a copy of the same row of `grad`: the streaming copy first, the named rows are zeroed behind it
    if (!grad) return RUA_EINVAL;
    if ((double)src->n_rows * (double)row_bytes >= 9.0e18) return RUA_ERANGE;
    if (tracing()) trace_add("setitem_backward_copy");
    if ((e = stream_copy(grad_raw, grad, src->n_rows * row_bytes, stream)) != 0) return e;
  }
  if (list->n_rows == 0) return 0;
  // the mover's rules: the lane width from the row size and all three base addresses, streaming by the larger output
  const int64_t dst_rows = grad_raw && src->n_rows > list->n_rows ? src->n_rows : list->n_rows;
  const SetitemBackwardPlan P = plan_setitem_backward(list->n_rows, dst_rows, row_bytes,
                                                      (uintptr_t)grad | (uintptr_t)grad_value | (uintptr_t)grad_raw, flags);
  if (P.err) return P.err;
  return launch_setitem_backward(P, (hipStream_t)stream, *list, *src, (const char*)grad, (char*)grad_value, (char*)grad_raw,
                                 row_bytes);
}
