// rua_scan.hip — per-sequence inclusive cumsum over the tokens of a C / L / P / R container (rua_segment_cumsum;
// include/rua.h).  An extension: the reference has no prefix operator; its users pad (`left()`), call torch.cumsum along
// dim 1 and cast back — three passes over the payload plus the padding, and nothing at all for a PackedSequence.
//
// ONE association order per (sequence, column, direction), whatever the layout, the kernel form, the alignment or the
// launch geometry — that is what makes the operator commute with the casts bit for bit (z.cumsum().cat() ==
// z.cat().cumsum()).  With u the position along the scan (u = t forward, u = len - 1 - t for `reverse`: the SAME order
// on the mirrored token index, so z.rev().cumsum().rev() == z.cumsum(reverse=True)) and x_u the token there:
//   - GROUPS of SC_GROUP = 8 consecutive positions: the inclusive prefixes inside a group come from three doubling
//     steps, p_j <- p_(j-d) + p_j for j >= d, d = 1, 2, 4 (a position below d keeps its value: no addition);
//   - TILES of SC_SLOTS = 32 positions = 4 groups with totals g0 .. g3 (the prefix at a group's last position): a token
//     of group 1 is preceded by g0, of group 2 by g0 + g1, of group 3 by (g0 + g1) + g2; the tile's total is
//     ((g0 + g1) + g2) + g3;
//   - BLOCKS of SC_BLOCK_TOK = 2 048 positions = 64 tiles: the carry of a block is the sum of the totals of its tiles so
//     far, added one tile after the other, starting afresh in every block;
//   - the base of a block is the sum of the totals of the blocks before it, added one block after the other;
//   - out_u = ((base + carry) + groups before) + prefix inside the group, rounded once to the payload dtype.
// A term that does not exist (first block, first tile of a block, first group of a tile; positions past the end of the
// sequence) is the additive IDENTITY, which for IEEE floats is -0.0, not +0.0: x + (-0.0) is x for every x, -0.0 and
// +0.0 included, so no form can differ from another in the sign of a zero by adding a carry the other one skips.
// The lanes form maps a position of a tile to a lane (32 lanes per sequence), the rows form to 8 consecutive threads of
// a workgroup (one 16-byte vector each; a group is 8 slots of one wave, the four groups are the four waves).  The cut
// form hands the blocks of a long sequence to different workgroups: phase 1 leaves every block's total in a small
// workspace, phase 2 adds them up in block order and scans the block with that base (the payload is read twice).
//
// bf16 / f16 accumulate in fp32 and every output is rounded once (CPU torch: x.cumsum(0) ==
// x.float().cumsum(0).to(x.dtype)); int64 wraps.  Padding rows of a LEFT / RIGHT result are written as zeros in the same
// pass and are never read.  The carry travels along the sequence: one read and one write of the payload, no slab.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int SC_GROUP = 8;                // positions scanned by doubling steps
constexpr int SC_SLOTS = 32;               // positions of a tile = 4 groups
constexpr int SC_BLOCK_TOK = SEG_BLOCK_TOK; // positions of a block = 64 tiles
constexpr int SC_TILES = SC_BLOCK_TOK / SC_SLOTS;
constexpr int SC_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int SC_ROWS_UNR = 4;             // rows form: tiles in flight per workgroup (one barrier for the four)
constexpr int SC_LANES_UNR = 4;            // lanes form: tiles in flight per half wave
static_assert(SC_SLOTS == 4 * SC_GROUP && SC_SLOTS * SC_LPR == RUA_BLOCK && SC_GROUP * SC_LPR == RUA_WAVE,
              "a group is a wave of the rows form, a tile is its workgroup");

// ---------------------------------------------------------------- element types
template <typename B> struct sc_float : B {
  static __device__ __forceinline__ typename B::acc ident() { return (typename B::acc)(-0.0); }
};
struct sc_i64 {                            // unsigned accumulation: the sum wraps
  using raw = int64_t; using acc = unsigned long long;
  static __device__ __forceinline__ acc up(raw v) { return (acc)v; }
  static __device__ __forceinline__ raw down(acc v) { return (raw)v; }
  static __device__ __forceinline__ acc ident() { return 0; }
  static const char* name() { return "i64"; }
};

// ---------------------------------------------------------------- the order, in one place for every form
// what precedes a token of group `w` of a tile, given the tile's four group totals; `car` moves on by the tile's total
template <typename E>
__device__ __forceinline__ typename E::acc sc_before(typename E::acc base, typename E::acc& car, typename E::acc g0,
                                                     typename E::acc g1, typename E::acc g2, typename E::acc g3, int w) {
  using A = typename E::acc;
  const A s1 = g0 + g1, s2 = s1 + g2, tt = s2 + g3;
  const A groups = w == 0 ? E::ident() : w == 1 ? g0 : w == 2 ? s1 : s2;
  const A pre = (base + car) + groups;
  car = car + tt;
  return pre;
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// A wave takes two sequences, 32 lanes each; lane r of a half is position r of a tile: consecutive lanes take
// consecutive tokens (one contiguous run of whole lines for CAT), the doubling steps and the group totals go across
// lanes by shuffles, base and carry stay in registers from tile to tile.
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_cumsum_lanes_kernel(rua_layout L, const char* xin, char* out, int H,
                                                                     int W, int rev) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = SC_LANES_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (SC_SLOTS - 1), gq = q & (SC_GROUP - 1), w = q / SC_GROUP;
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);

  struct alignas(16) Row { raw e[VE]; };
  A base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = E::ident();

  for (int64_t u0 = 0; u0 < maxlen; u0 += (int64_t)SC_SLOTS * UNR) {
    Row x[UNR];
    int64_t rows[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * SC_SLOTS + q;
      rows[k] = -1;
      if (u < len) {
        const int64_t row = token_to_row(L, b, rev ? len - 1 - u : u, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ld_row_w(xin + row * nb, nb, W, &x[k]);
        }
      }
    }
    A v[UNR][VE];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
#pragma unroll
      for (int e = 0; e < VE; ++e) v[k][e] = (rows[k] >= 0 && e < H) ? E::up(x[k].e[e]) : E::ident();
    }
#pragma unroll
    for (int d = 1; d < SC_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          const A from = __shfl_up(v[k][e], d, SC_SLOTS);
          if (gq >= d) v[k][e] = from + v[k][e];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * SC_SLOTS;
      if (tile0 >= maxlen) break;                             // wave-uniform
      Row o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (e >= H) continue;
        const A g0 = __shfl(v[k][e], SC_GROUP - 1, SC_SLOTS), g1 = __shfl(v[k][e], 2 * SC_GROUP - 1, SC_SLOTS);
        const A g2 = __shfl(v[k][e], 3 * SC_GROUP - 1, SC_SLOTS), g3 = __shfl(v[k][e], 4 * SC_GROUP - 1, SC_SLOTS);
        o.e[e] = E::down(sc_before<E>(base[e], car[e], g0, g1, g2, g3, w) + v[k][e]);
      }
      if (rows[k] >= 0) st_row_w(out + rows[k] * nb, nb, W, &o);
      if ((tile0 / SC_SLOTS + 1) % SC_TILES == 0) {           // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = base[e] + car[e]; car[e] = E::ident(); }
      }
    }
  }
  if (have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
    Row z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < L.T_phys; j += SC_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st_row_w(out + row * nb, nb, W, &z);
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup takes (sequence x 128-byte column chunk): thread (q, l) = (tid / 8, tid % 8) is position q of a tile and
// owns the l-th 16-byte vector of the chunk.  A group is the 8 slots of one wave (doubling steps by shuffles over 8, 16
// and 32 lanes); the four group totals of a tile cross the waves through LDS — four tiles per barrier, two buffers in
// turn, so one barrier per 128 rows.  Base and carry are kept by every thread (the same values in all of them).
// mode SEG_PARTIAL / SEG_FINISH: the CUT form — a workgroup per (sequence, block of 2 048 positions, chunk) leaves its
// block's total in `ws`, and a second launch adds the totals of the blocks before its own and scans the block.
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.
template <typename E, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_cumsum_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                    typename E::raw* out, int64_t H, int n_chunks,
                                                                    int mode, int maxblk, typename E::acc* ws, int rev) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = SC_LPR * VE;
  constexpr int UNR = SC_ROWS_UNR;
  __shared__ A xch[2][UNR][RUA_WAVES_PER_BLOCK][SC_LPR][VE];
  struct alignas(16) Vec { raw e[VE]; };

  const int tid = threadIdx.x;
  const int l = tid & (SC_LPR - 1), q = tid >> 3, w = tid >> 6, gq = q & (SC_GROUP - 1);
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode != SEG_FULL) { blk = (int)(b % maxblk); b /= maxblk; }
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: a CAT layout whose T_log understates a length
  // must not walk past the maxblk blocks that exist (rua.h: T_log has to be a true bound)
  const int64_t have_blk = (len + SC_BLOCK_TOK - 1) / SC_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode != SEG_FULL && blk > 0 && blk >= nblk) return;     // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  int64_t ub = 0, ue = len;                                  // positions along the scan
  if (mode != SEG_FULL) {
    ub = (int64_t)blk * SC_BLOCK_TOK;
    ue = len < ub + SC_BLOCK_TOK ? len : ub + SC_BLOCK_TOK;
    if (ub > ue) ub = ue;
  }

  auto ld = [&](int64_t row, Vec& v) {
    const raw* p = xin + row * H + col0;
    if constexpr (AL) {
      *(uint4*)&v = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = e < nval ? p[e] : (raw)0;
    }
  };
  auto st = [&](int64_t row, const Vec& v) {
    raw* p = out + row * H + col0;
    if constexpr (AL) {
      *(uint4*)p = *(const uint4*)&v;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (e < nval) p[e] = v.e[e];
    }
  };

  A base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = E::ident();
  if (mode == SEG_FINISH) {
    for (int64_t k = 0; k < blk; ++k) {
      const A* p = ws + ((((b * maxblk + k) * n_chunks + c) * SC_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) base[e] = base[e] + p[e];
    }
  }

  int buf = 0;
  for (int64_t u0 = ub; u0 < ue; u0 += (int64_t)SC_SLOTS * UNR, buf ^= 1) {
    Vec x[UNR];
    int64_t rows[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * SC_SLOTS + q;
      rows[k] = -1;
      if (active && u < ue) {
        const int64_t row = token_to_row(L, b, rev ? len - 1 - u : u, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ld(row, x[k]);
        }
      }
    }
    A v[UNR][VE];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
#pragma unroll
      for (int e = 0; e < VE; ++e) v[k][e] = rows[k] >= 0 ? E::up(x[k].e[e]) : E::ident();
    }
    // positions 0 .. 7 of a group sit 8 lanes apart
#pragma unroll
    for (int d = 1; d < SC_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const A from = __shfl_up(v[k][e], d * SC_LPR, RUA_WAVE);
          if (gq >= d) v[k][e] = from + v[k][e];
        }
      }
    }
    if (gq == SC_GROUP - 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) xch[buf][k][w][l][e] = v[k][e];
      }
    }
    __syncthreads();       // (the other buffer is written next: whoever still reads this one has not passed the next barrier)
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * SC_SLOTS;
      if (tile0 >= ue) break;                                 // workgroup-uniform
      Vec o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A pre = sc_before<E>(base[e], car[e], xch[buf][k][0][l][e], xch[buf][k][1][l][e], xch[buf][k][2][l][e],
                                   xch[buf][k][3][l][e], w);
        o.e[e] = E::down(pre + v[k][e]);
      }
      if (mode != SEG_PARTIAL && rows[k] >= 0) st(rows[k], o);
      if (mode == SEG_FULL && (tile0 / SC_SLOTS + 1) % SC_TILES == 0) {      // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = base[e] + car[e]; car[e] = E::ident(); }
      }
    }
  }
  if (mode == SEG_PARTIAL) {
    if (tid < SC_LPR) {
      A* p = ws + ((((b * maxblk + blk) * n_chunks + c) * SC_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) p[e] = car[e];
    }
    return;
  }
  if (active && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
    Vec z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < L.T_phys; j += SC_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st(row, z);
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps a block's total per (padded) column: one accumulator
static seg_plan sc_make_plan(const rua_layout& L, int64_t H, int32_t dtype) {
  const int es = seg_esize(dtype, true);
  return seg_make_plan(L, H, es, es == 8 ? 8 : 4);
}

template <typename E>
static int sc_launch(const rua_layout& L, const void* x, void* out, int64_t H, int32_t dtype, int rev, void* ws,
                     hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t bases = (uint64_t)(uintptr_t)x | (uint64_t)(uintptr_t)out;
  if (bases % sizeof(raw)) return RUA_EALIGN;                 // (elements themselves are always aligned)

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    const uint64_t own = (uint64_t)row_bytes | 16u;             // AL: the bases did not narrow the row's own access width
    seg_trace("seg_cumsum_lanes_kernel T=%s W=%d H=%d AL=%d rev=%d kind=%d", E::name(), ln.W, (int)H,
              (int)(ln.W == (int)(own & (~own + 1))), rev, L.kind);
    hipLaunchKernelGGL((seg_cumsum_lanes_kernel<E>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, L, (const char*)x,
                       (char*)out, (int)H, ln.W, rev);
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(sc_make_plan(L, H, dtype), L, row_bytes, bases, ws != nullptr);
  const seg_plan& p = r.p;
  if (!r.grid) return RUA_ERANGE;
  return seg_launch_rows(
      r,
      [&](int mode) {
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_cumsum_rows_kernel<E, decltype(AL)::value>), dim3((unsigned)r.grid), dim3(RUA_BLOCK), 0,
                             s, L, (const raw*)x, (raw*)out, H, p.n_chunks, mode, r.cut ? p.maxblk : 1, (A*)ws, rev);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("seg_cumsum_rows_kernel T=%s AL=%d rev=%d kind=%d cut=1 phase=%s blocks=%d chunks=%d", E::name(),
                    (int)r.al, rev, L.kind, phase, p.maxblk, p.n_chunks);
        else
          seg_trace("seg_cumsum_rows_kernel T=%s AL=%d rev=%d kind=%d cut=0 chunks=%d", E::name(), (int)r.al, rev, L.kind,
                    p.n_chunks);
      });
}

static int sc_dispatch(const rua_layout* lay, const void* x, void* out, int64_t H, int32_t dtype, int32_t reverse,
                       void* ws, void* stream) {
  const int es = seg_esize(dtype, true);
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!x || !out) return RUA_EINVAL;
  if (seg_too_large(lay, H, es)) return RUA_ERANGE;
#define RUA_SC(E) sc_launch<E>(*lay, x, out, H, dtype, reverse ? 1 : 0, ws, (hipStream_t)stream)
#define RUA_SC_FLOAT(B) RUA_SC(sc_float<B>)
  if (dtype == RUA_I64) return RUA_SC(sc_i64);
  RUA_DISPATCH_FLOAT(dtype, RUA_SC_FLOAT);
#undef RUA_SC_FLOAT
#undef RUA_SC
}

}  // namespace rua

extern "C" int64_t rua_cumsum_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::sc_make_plan(*lay, H, dtype).ws_bytes;
}

extern "C" int rua_segment_cumsum(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype,
                                  int32_t reverse, void* ws, void* stream) {
  return rua::sc_dispatch(lay, data, out, H, dtype, reverse, ws, stream);
}
