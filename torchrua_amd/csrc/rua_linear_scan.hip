// rua_linear_scan.hip — per-sequence first-order linear recurrence h_u = a_u * h_(u-1) + x_u over the tokens of a
// C / L / P / R container (rua_segment_linear_scan, rua_segment_linear_scan_backward; include/rua.h).  An extension, like
// the cumsum of rua_scan.hip: the reference's users pad (`left()`), loop over the time steps with ATen elementwise
// kernels and cast back — T launches and traffic over the padding, and nothing at all for a PackedSequence.
//
// The operator is associative on pairs (A, B) = (product of gates, value): an EARLIER (A1, B1) and a LATER (A2, B2)
// combine as (A2 * A1, A2 * B1 + B2).  Position u of a sequence enters as (a_u, x_u), position 0 as (1, x_0): its gate
// is never used (forward: the gate of the first token; `reverse`: of the last).  The pairs are combined in the ONE
// association order of rua_scan.hip, unchanged — groups of 8 positions by three doubling steps, tiles of 4 groups,
// blocks of 64 tiles whose carry starts afresh, the base of a block from the totals of the blocks before it, and
//   out_u = B of (((base . carry) . groups before) . prefix inside the group),
// rounded once to the payload dtype — for every layout, kernel form, alignment and launch geometry, so the operator
// commutes with the casts bit for bit, `reverse` is the mirrored forward scan, cut == uncut, aligned == unaligned, and a
// gate that is exactly 1 everywhere gives rua_segment_cumsum's bits (1 * B1 + B2 is B1 + B2).  A term that does not
// exist (first block, first tile, first group; positions past the end) is the pair (1, -0.0): as the LATER operand it
// changes nothing at all, as the EARLIER one it leaves A2 * (-0.0) + B2, which is B2 for every finite A2 (but for the
// sign of a zero B2 under a negative A2).  Multiplications and additions are never contracted.
// LIMIT: a blocked scan forms partial gate products.  The result is finite only where the product of the gates over
// every aligned group, tile and block (and over the blocks before a block) is representable: a sequential evaluation
// survives a gate product that overflows and is later multiplied by 0, this one turns it into inf * 0 = NaN.
//
// bf16 / f16 accumulate in fp32, gates included, and every output is rounded once.  The gate is a tensor of the
// payload's storage shape or ONE scalar passed by value and held in the accumulator type (no gate tensor is read).
// Padding rows of a LEFT / RIGHT result are zeros, written in the same pass and never read.
//
// The backward is the same scan run the other way with the gate taken from the PREVIOUS scan position (which drops
// exactly the gate the forward ignored): dx_u' = g_u' + a_(u'-1) * dx_(u'-1), and da_u' = dx_u' * h_(u'+1) (0 where the
// next position does not exist: the ignored gate).  The shifted gate and h are loaded from the neighbouring token's row:
// the same lines the neighbouring threads load, so every array still crosses the memory bus once.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <initializer_list>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

// the geometry of rua_scan.hip, repeated (that file's bits are pinned by its own tests and it stays untouched): a gate
// of 1 reproduces the cumsum bit for bit only while these agree with SC_* there
constexpr int LS_GROUP = 8;                // positions scanned by doubling steps
constexpr int LS_SLOTS = 32;               // positions of a tile = 4 groups
constexpr int LS_BLOCK_TOK = SEG_BLOCK_TOK; // positions of a block = 64 tiles
constexpr int LS_TILES = LS_BLOCK_TOK / LS_SLOTS;
constexpr int LS_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int LS_ROWS_UNR = 2;             // rows form: tiles in flight per workgroup (two accumulators per element)
constexpr int LS_LANES_UNR = 2;            // lanes form: tiles in flight per half wave
static_assert(LS_GROUP == 8 && LS_SLOTS == 32 && LS_BLOCK_TOK == 2048 && LS_TILES == 64,
              "the association order of rua_scan.hip: groups of 8, tiles of 32, blocks of 2 048");
static_assert(LS_SLOTS == 4 * LS_GROUP && LS_SLOTS * LS_LPR == RUA_BLOCK && LS_GROUP * LS_LPR == RUA_WAVE,
              "a group is a wave of the rows form, a tile is its workgroup");

// ---------------------------------------------------------------- the pair and the order, in one place for every form
template <typename A> struct ls_pair { A a, b; };

template <typename A> __device__ __forceinline__ ls_pair<A> ls_ident() { return {(A)1, (A)(-0.0)}; }

// an earlier pair, then a later one
template <typename A> __device__ __forceinline__ ls_pair<A> ls_comb(ls_pair<A> p, ls_pair<A> q) {
  return {q.a * p.a, q.a * p.b + q.b};
}

// A value about to be rounded to the payload dtype, made opaque to the optimiser: for f16 the backend otherwise folds
// the fp32 multiplication (or addition) and the conversion into ONE mixed-precision instruction that rounds once — in
// some instantiations and not in others, so two forms of the same scan would differ in the last bit of a double rounding.
template <typename A> __device__ __forceinline__ A ls_pin(A v) {
  asm volatile("" : "+v"(v));
  return v;
}

// what precedes a token of group `w` of a tile, given the tile's four group totals; `car` moves on by the tile's total
template <typename A>
__device__ __forceinline__ ls_pair<A> ls_before(ls_pair<A> base, ls_pair<A>& car, ls_pair<A> g0, ls_pair<A> g1,
                                                ls_pair<A> g2, ls_pair<A> g3, int w) {
  const ls_pair<A> s1 = ls_comb(g0, g1), s2 = ls_comb(s1, g2), tt = ls_comb(s2, g3);
  const ls_pair<A> groups = w == 0 ? ls_ident<A>() : w == 1 ? g0 : w == 2 ? s1 : s2;
  const ls_pair<A> pre = ls_comb(ls_comb(base, car), groups);
  car = ls_comb(car, tt);
  return pre;
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// The geometry of seg_cumsum_lanes_kernel: a wave takes two sequences, 32 lanes each; lane r of a half is position r of
// a tile.  BWD: the gate comes from the previous scan position's row, and (gout != NULL) h from the next one's.
template <typename E, bool BWD>
__global__ __launch_bounds__(RUA_BLOCK) void seg_linear_scan_lanes_kernel(rua_layout L, const char* xin,
                                                                          const char* gate, double gate_scalar,
                                                                          const char* hin, char* out, char* gout, int H,
                                                                          int W, int rev) {
  using raw = typename E::raw;
  using A = typename E::acc;
  using PR = ls_pair<A>;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = LS_LANES_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (LS_SLOTS - 1), gq = q & (LS_GROUP - 1), w = q / LS_GROUP;
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);
  const A gs = (A)gate_scalar;

  struct alignas(16) Row { raw e[VE]; };
  PR base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = ls_ident<A>();

  for (int64_t u0 = 0; u0 < maxlen; u0 += (int64_t)LS_SLOTS * UNR) {
    Row x[UNR], ga[UNR], hh[UNR];
    int64_t rows[UNR];
    bool hasg[UNR], hash[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * LS_SLOTS + q;
      rows[k] = -1;
      hasg[k] = hash[k] = false;
      if (u < len) {
        const int64_t row = token_to_row(L, b, rev ? len - 1 - u : u, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ld_row_w(xin + row * nb, nb, W, &x[k]);
          if (u > 0 && gate) {
            const int64_t ug = BWD ? u - 1 : u;
            const int64_t grow = BWD ? token_to_row(L, b, rev ? len - 1 - ug : ug, len) : row;
            if (grow >= 0 && grow < L.n_rows) { hasg[k] = true; ld_row_w(gate + grow * nb, nb, W, &ga[k]); }
          }
          if (BWD && gout && u + 1 < len) {
            const int64_t hrow = token_to_row(L, b, rev ? len - 2 - u : u + 1, len);
            if (hrow >= 0 && hrow < L.n_rows) { hash[k] = true; ld_row_w(hin + hrow * nb, nb, W, &hh[k]); }
          }
        }
      }
    }
    PR v[UNR][VE];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * LS_SLOTS + q;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        v[k][e] = ls_ident<A>();
        if (rows[k] >= 0 && e < H) {
          v[k][e].b = E::up(x[k].e[e]);
          if (u > 0) v[k][e].a = gate ? (hasg[k] ? E::up(ga[k].e[e]) : (A)1) : gs;
        }
      }
    }
#pragma unroll
    for (int d = 1; d < LS_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          PR from;
          from.a = __shfl_up(v[k][e].a, d, LS_SLOTS);
          from.b = __shfl_up(v[k][e].b, d, LS_SLOTS);
          if (gq >= d) v[k][e] = ls_comb(from, v[k][e]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * LS_SLOTS;
      if (tile0 >= maxlen) break;                             // wave-uniform
      Row o, og;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        o.e[e] = (raw)0;
        og.e[e] = (raw)0;
        if (e >= H) continue;
        PR g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          g[i].a = __shfl(v[k][e].a, (i + 1) * LS_GROUP - 1, LS_SLOTS);
          g[i].b = __shfl(v[k][e].b, (i + 1) * LS_GROUP - 1, LS_SLOTS);
        }
        const PR pre = ls_before<A>(base[e], car[e], g[0], g[1], g[2], g[3], w);
        const A r = ls_pin(v[k][e].a * pre.b + v[k][e].b);
        o.e[e] = E::down(r);
        if (BWD && hash[k]) og.e[e] = E::down(ls_pin(r * E::up(hh[k].e[e])));
      }
      if (rows[k] >= 0) {
        st_row_w(out + rows[k] * nb, nb, W, &o);
        if (BWD && gout) st_row_w(gout + rows[k] * nb, nb, W, &og);
      }
      if ((tile0 / LS_SLOTS + 1) % LS_TILES == 0) {           // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = ls_comb(base[e], car[e]); car[e] = ls_ident<A>(); }
      }
    }
  }
  if (have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
    Row z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < L.T_phys; j += LS_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) {
        st_row_w(out + row * nb, nb, W, &z);
        if (BWD && gout) st_row_w(gout + row * nb, nb, W, &z);
      }
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// The geometry of seg_cumsum_rows_kernel: a workgroup per (sequence x 128-byte column chunk), thread (q, l) is position
// q of a tile and owns the l-th 16-byte vector of the chunk; the four group totals of a tile (pairs) cross the waves
// through LDS, two buffers in turn.  mode SEG_PARTIAL / SEG_FINISH: the cut form, a pair per block and column in `ws`.
template <typename E, bool AL, bool BWD>
__global__ __launch_bounds__(RUA_BLOCK) void seg_linear_scan_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                         const typename E::raw* gate, double gate_scalar,
                                                                         const typename E::raw* hin,
                                                                         typename E::raw* out, typename E::raw* gout,
                                                                         int64_t H, int n_chunks, int mode, int maxblk,
                                                                         ls_pair<typename E::acc>* ws, int rev) {
  using raw = typename E::raw;
  using A = typename E::acc;
  using PR = ls_pair<A>;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = LS_LPR * VE;
  constexpr int UNR = LS_ROWS_UNR;
  __shared__ PR xch[2][UNR][RUA_WAVES_PER_BLOCK][LS_LPR][VE];
  struct alignas(16) Vec { raw e[VE]; };

  const int tid = threadIdx.x;
  const int l = tid & (LS_LPR - 1), q = tid >> 3, w = tid >> 6, gq = q & (LS_GROUP - 1);
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode != SEG_FULL) { blk = (int)(b % maxblk); b /= maxblk; }
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: never walk past the maxblk blocks that exist
  const int64_t have_blk = (len + LS_BLOCK_TOK - 1) / LS_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode != SEG_FULL && blk > 0 && blk >= nblk) return;     // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  const bool want_h = BWD && gout != nullptr && mode != SEG_PARTIAL;
  const A gs = (A)gate_scalar;
  int64_t ub = 0, ue = len;                                  // positions along the scan
  if (mode != SEG_FULL) {
    ub = (int64_t)blk * LS_BLOCK_TOK;
    ue = len < ub + LS_BLOCK_TOK ? len : ub + LS_BLOCK_TOK;
    if (ub > ue) ub = ue;
  }

  auto ld = [&](const raw* src, int64_t row, Vec& v) {
    const raw* p = src + row * H + col0;
    if constexpr (AL) {
      *(uint4*)&v = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = e < nval ? p[e] : (raw)0;
    }
  };
  auto st = [&](raw* dst, int64_t row, const Vec& v) {
    raw* p = dst + row * H + col0;
    if constexpr (AL) {
      *(uint4*)p = *(const uint4*)&v;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (e < nval) p[e] = v.e[e];
    }
  };

  PR base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = ls_ident<A>();
  if (mode == SEG_FINISH) {
    for (int64_t k = 0; k < blk; ++k) {
      const PR* p = ws + ((((b * maxblk + k) * n_chunks + c) * LS_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) base[e] = ls_comb(base[e], p[e]);
    }
  }

  int buf = 0;
  for (int64_t u0 = ub; u0 < ue; u0 += (int64_t)LS_SLOTS * UNR, buf ^= 1) {
    Vec x[UNR], ga[UNR], hh[UNR];
    int64_t rows[UNR];
    bool hasg[UNR], hash[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * LS_SLOTS + q;
      rows[k] = -1;
      hasg[k] = hash[k] = false;
      if (active && u < ue) {
        const int64_t row = token_to_row(L, b, rev ? len - 1 - u : u, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ld(xin, row, x[k]);
          if (u > 0 && gate) {
            const int64_t ug = BWD ? u - 1 : u;
            const int64_t grow = BWD ? token_to_row(L, b, rev ? len - 1 - ug : ug, len) : row;
            if (grow >= 0 && grow < L.n_rows) { hasg[k] = true; ld(gate, grow, ga[k]); }
          }
          if (want_h && u + 1 < len) {
            const int64_t hrow = token_to_row(L, b, rev ? len - 2 - u : u + 1, len);
            if (hrow >= 0 && hrow < L.n_rows) { hash[k] = true; ld(hin, hrow, hh[k]); }
          }
        }
      }
    }
    PR v[UNR][VE];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * LS_SLOTS + q;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        v[k][e] = ls_ident<A>();
        if (rows[k] >= 0) {
          v[k][e].b = E::up(x[k].e[e]);
          if (u > 0) v[k][e].a = gate ? (hasg[k] ? E::up(ga[k].e[e]) : (A)1) : gs;
        }
      }
    }
    // positions 0 .. 7 of a group sit 8 lanes apart
#pragma unroll
    for (int d = 1; d < LS_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          PR from;
          from.a = __shfl_up(v[k][e].a, d * LS_LPR, RUA_WAVE);
          from.b = __shfl_up(v[k][e].b, d * LS_LPR, RUA_WAVE);
          if (gq >= d) v[k][e] = ls_comb(from, v[k][e]);
        }
      }
    }
    if (gq == LS_GROUP - 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) xch[buf][k][w][l][e] = v[k][e];
      }
    }
    __syncthreads();       // (the other buffer is written next: whoever still reads this one has not passed the next barrier)
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * LS_SLOTS;
      if (tile0 >= ue) break;                                 // workgroup-uniform
      Vec o, og;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const PR pre = ls_before<A>(base[e], car[e], xch[buf][k][0][l][e], xch[buf][k][1][l][e], xch[buf][k][2][l][e],
                                    xch[buf][k][3][l][e], w);
        const A r = ls_pin(v[k][e].a * pre.b + v[k][e].b);
        o.e[e] = E::down(r);
        og.e[e] = (BWD && hash[k]) ? E::down(ls_pin(r * E::up(hh[k].e[e]))) : (raw)0;
      }
      if (mode != SEG_PARTIAL && rows[k] >= 0) {
        st(out, rows[k], o);
        if (want_h) st(gout, rows[k], og);
      }
      if (mode == SEG_FULL && (tile0 / LS_SLOTS + 1) % LS_TILES == 0) {      // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = ls_comb(base[e], car[e]); car[e] = ls_ident<A>(); }
      }
    }
  }
  if (mode == SEG_PARTIAL) {
    if (tid < LS_LPR) {
      PR* p = ws + ((((b * maxblk + blk) * n_chunks + c) * LS_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) p[e] = car[e];
    }
    return;
  }
  if (active && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
    Vec z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < L.T_phys; j += LS_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) {
        st(out, row, z);
        if (want_h) st(gout, row, z);
      }
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps one PAIR of accumulators per block and (padded) column
static seg_plan ls_make_plan(const rua_layout& L, int64_t H, int32_t dtype) {
  const int es = seg_esize(dtype, false);
  return seg_make_plan(L, H, es, 2 * (es == 8 ? 8 : 4));
}

template <typename E, bool BWD>
static int ls_launch(const rua_layout& L, const void* x, const void* gate, double gs, const void* h, void* out,
                     void* gout, int64_t H, int32_t dtype, int rev, void* ws, hipStream_t s) {
  using raw = typename E::raw;
  using PR = ls_pair<typename E::acc>;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t bases = (uint64_t)(uintptr_t)x | (uint64_t)(uintptr_t)out | (uint64_t)(uintptr_t)gate |
                         (uint64_t)(uintptr_t)(gout ? h : nullptr) | (uint64_t)(uintptr_t)gout;
  if (bases % sizeof(raw)) return RUA_EALIGN;                 // (elements themselves are always aligned)
  const char* gname = gate ? "tensor" : "scalar";

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    const uint64_t own = (uint64_t)row_bytes | 16u;             // AL: the bases did not narrow the row's own access width
    seg_trace("seg_linear_scan_lanes_kernel T=%s W=%d H=%d AL=%d rev=%d kind=%d gate=%s bwd=%d cut=0", E::name(), ln.W,
              (int)H, (int)(ln.W == (int)(own & (~own + 1))), rev, L.kind, gname, (int)BWD);
    hipLaunchKernelGGL((seg_linear_scan_lanes_kernel<E, BWD>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, L,
                       (const char*)x, (const char*)gate, gs, (const char*)h, (char*)out, (char*)gout, (int)H, ln.W, rev);
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(ls_make_plan(L, H, dtype), L, row_bytes, bases, ws != nullptr);
  const seg_plan& p = r.p;
  if (!r.grid) return RUA_ERANGE;
  return seg_launch_rows(
      r,
      [&](int mode) {
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_linear_scan_rows_kernel<E, decltype(AL)::value, BWD>), dim3((unsigned)r.grid),
                             dim3(RUA_BLOCK), 0, s, L, (const raw*)x, (const raw*)gate, gs, (const raw*)h, (raw*)out,
                             (raw*)gout, H, p.n_chunks, mode, r.cut ? p.maxblk : 1, (PR*)ws, rev);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("seg_linear_scan_rows_kernel T=%s AL=%d rev=%d kind=%d gate=%s bwd=%d cut=1 phase=%s blocks=%d chunks=%d",
                    E::name(), (int)r.al, rev, L.kind, gname, (int)BWD, phase, p.maxblk, p.n_chunks);
        else
          seg_trace("seg_linear_scan_rows_kernel T=%s AL=%d rev=%d kind=%d gate=%s bwd=%d cut=0 chunks=%d", E::name(),
                    (int)r.al, rev, L.kind, gname, (int)BWD, p.n_chunks);
      });
}

template <bool BWD>
static int ls_dispatch(const rua_layout* lay, const void* x, const void* gate, double gs, const void* h, void* out,
                       void* gout, int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream) {
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!x || !out) return RUA_EINVAL;
  if (out == gate || (BWD && h && out == h)) return RUA_EINVAL;
  if (BWD && gout && (!h || !gate || gout == x || gout == gate || gout == h || gout == out)) return RUA_EINVAL;
  if (seg_too_large(lay, H, es)) return RUA_ERANGE;
  // the backward runs the scan the other way
  const int rev = (reverse ? 1 : 0) ^ (BWD ? 1 : 0);
#define RUA_LS(E) ls_launch<E, BWD>(*lay, x, gate, gs, h, out, gout, H, dtype, rev, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_LS);
#undef RUA_LS
}

}  // namespace rua

extern "C" int64_t rua_linear_scan_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::ls_make_plan(*lay, H, dtype).ws_bytes;
}

extern "C" int rua_segment_linear_scan(const rua_layout* lay, const void* data, const void* gate, double gate_scalar,
                                       void* out, int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream) {
  return rua::ls_dispatch<false>(lay, data, gate, gate_scalar, nullptr, out, nullptr, H, dtype, reverse, ws, stream);
}

extern "C" int rua_segment_linear_scan_backward(const rua_layout* lay, const void* grad_out, const void* gate,
                                                double gate_scalar, const void* h, void* grad_x, void* grad_gate,
                                                int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream) {
  return rua::ls_dispatch<true>(lay, grad_out, gate, gate_scalar, h, grad_x, grad_gate, H, dtype, reverse, ws, stream);
}
