// rua_cumext.hip — the rest of the per-sequence `cum*` family over the tokens of a C / L / P / R container: running
// max / min with indices (rua_segment_cumextreme), its backward (rua_segment_cumextreme_backward), logcumsumexp
// (rua_segment_logcumsumexp) and its backward (rua_segment_logcumsumexp_backward); include/rua.h.  Extensions, like the
// cumsum of rua_scan.hip: the reference's users pad (`left(fill_value=-inf)`), call torch.cummax / torch.logcumsumexp
// along dim 1 and cast back — running values in the padding rows, wrong for an R, nothing for a PackedSequence.
//
// ONE skeleton for the four, the one of rua_scan.hip (groups of 8 positions by three doubling steps -> tiles of 32 = 4
// groups -> blocks of 2 048 = 64 tiles, carried tile after tile -> block bases added in block order; u = t forward,
// u = len - 1 - t for `reverse`), written ONCE over a monoid `Op`: a state of two fields per (sequence, column), an
// identity that comb() absorbs EXACTLY (it returns the other operand: a form that combines with a carry that does not
// exist gives the bits of a form that skips it), comb(earlier, later), a load that makes the state of one token and a
// store that finishes the inclusive state at a token.
//   cx_ext       (value, position): the LAST element of the highest rank, NaN above every number, -0.0 == +0.0 — torch's
//                cummax rule (later wins among equals; once a NaN is met the value stays NaN and the index moves on to
//                every later NaN).  comb() picks one of its operands: associative and idempotent, so every association
//                order gives the same bits.  Identity: "no element" (position -1), never a -inf that could beat a real one.
//   cx_ext_bwd   (sum, run id): the adjoint of "gather by indices".  Along the scan `indices` is constant on a run and
//                the run's head s has indices[s] == s, so grad_in[s] = [indices[s] == s] * sum of grad over the run of
//                s: a segmented sum keyed by the run id, scanned AGAINST the forward's direction.  Identity: id -1.
//   cx_lse       (m, s) with value m + log s, the softmax kernels' convention (rua_softmax.hip `combine`): s <- s_a *
//                exp(m_a - M) + s_b * exp(m_b - M), M = max(m_a, m_b), where the factor of the operand that holds M is
//                exactly 1 (no exp: +inf - +inf never forms).  A token is (x, 1); -inf is the identity (-inf, 0); a NaN
//                is (-inf, NaN), which poisons every later sum and is never mistaken for the identity.
//   cx_lse_bwd   the SAME fold with exponents -y_t and signed weights grad_t, run against the forward's direction, and
//                another finish: grad_in[s] = s_state * exp(m_state + x_s); exactly 0 where x_s = -inf.
// The three kernel forms are the cumsum's: lanes (rows of one vector, two sequences per wave), rows (a workgroup per
// sequence x 128-byte chunk, aligned or elementwise) and the cut form (partial + finish through a workspace that keeps
// one state per block and padded column).  Padding rows of a LEFT / RIGHT result are zeros in every output and are
// never read.  bf16 / f16 accumulate in fp32, every output is rounded once.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int CX_GROUP = 8;                // positions scanned by doubling steps
constexpr int CX_SLOTS = 32;               // positions of a tile = 4 groups
constexpr int CX_BLOCK_TOK = SEG_BLOCK_TOK; // positions of a block = 64 tiles
constexpr int CX_TILES = CX_BLOCK_TOK / CX_SLOTS;
constexpr int CX_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int CX_UNR = 2;                  // tiles in flight (a state is two fields: half the cumsum's four)
static_assert(CX_SLOTS == 4 * CX_GROUP && CX_SLOTS * CX_LPR == RUA_BLOCK && CX_GROUP * CX_LPR == RUA_WAVE,
              "a group is a wave of the rows form, a tile is its workgroup");

struct cx_i64 {
  using raw = int64_t; using acc = int64_t;
  static __device__ __forceinline__ acc up(raw v) { return v; }
  static __device__ __forceinline__ raw down(acc v) { return v; }
  static const char* name() { return "i64"; }
};

// the tensors of a launch, all of the payload's storage shape: element (row, column) sits at row * H + column in each
struct cx_args { const void* in0; const void* in1; const void* in2; void* out0; void* out1; int flag; };

template <typename A, typename B> struct cx_pair { A a; B b; };
struct cx_none {};

template <typename A, typename B>
__device__ __forceinline__ cx_pair<A, B> cx_shfl_up(const cx_pair<A, B>& v, int d, int width) {
  return {__shfl_up(v.a, d, width), __shfl_up(v.b, d, width)};
}
template <typename A, typename B>
__device__ __forceinline__ cx_pair<A, B> cx_shfl(const cx_pair<A, B>& v, int src, int width) {
  return {__shfl(v.a, src, width), __shfl(v.b, src, width)};
}

// VE elements at `off` of a tensor of T.  AL: whole aligned 16-byte vectors (nval == VE); else the first nval, one by one
template <bool AL, typename T, int VE> __device__ __forceinline__ void cx_ld(const void* base, int64_t off, int nval, T (&v)[VE]) {
  const T* p = (const T*)base + off;
  if constexpr (AL) {
    struct alignas(16) V { T e[VE]; };
    const V t = *(const V*)p;
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = t.e[e];
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = e < nval ? p[e] : (T)0;
  }
}
template <bool AL, typename T, int VE> __device__ __forceinline__ void cx_st(void* base, int64_t off, int nval, const T (&v)[VE]) {
  T* p = (T*)base + off;
  if constexpr (AL) {
    struct alignas(16) V { T e[VE]; };
    V t;
#pragma unroll
    for (int e = 0; e < VE; ++e) t.e[e] = v[e];
    *(V*)p = t;
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) if (e < nval) p[e] = v[e];
  }
}
template <bool AL, typename T, int VE> __device__ __forceinline__ void cx_zero(void* base, int64_t off, int nval) {
  T z[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) z[e] = (T)0;
  cx_st<AL, T, VE>(base, off, nval, z);
}

// ---------------------------------------------------------------- the monoids
// running max (flag = RUA_MAX) / min: in0 data; out0 values (may be null), out1 indices (int64, may be null)
template <typename E> struct cx_ext {
  using raw = typename E::raw; using A = typename E::acc;
  using S = cx_pair<A, int64_t>; using X = cx_none;
  static constexpr int VE = 16 / (int)sizeof(raw);
  static const char* name() { return E::name(); }
  static __device__ __forceinline__ S ident() { return {(A)0, (int64_t)-1}; }
  static __device__ __forceinline__ S comb(const S& a, const S& b, int flag) {
    if (b.b < 0) return a;
    if (a.b < 0) return b;
    const bool bn = b.a != b.a, an = a.a != a.a;
    const bool later = bn || (!an && (flag == RUA_MAX ? b.a >= a.a : b.a <= a.a));
    return later ? b : a;
  }
  template <bool AL> static __device__ __forceinline__ void load(const cx_args& g, int64_t off, int nval, int64_t t,
                                                                  S (&s)[VE], X (&)[VE]) {
    raw v[VE];
    cx_ld<AL, raw, VE>(g.in0, off, nval, v);
#pragma unroll
    for (int e = 0; e < VE; ++e) s[e] = e < nval ? S{E::up(v[e]), t} : ident();
  }
  template <bool AL> static __device__ __forceinline__ void store(const cx_args& g, int64_t off, int nval, int64_t,
                                                                   const S (&s)[VE], const X (&)[VE]) {
    if (g.out0) {
      raw o[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) o[e] = E::down(s[e].a);
      cx_st<AL, raw, VE>(g.out0, off, nval, o);
    }
    if (g.out1) {
      int64_t o[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) o[e] = s[e].b;
      cx_st<AL, int64_t, VE>(g.out1, off, nval, o);
    }
  }
  template <bool AL> static __device__ __forceinline__ void zero(const cx_args& g, int64_t off, int nval) {
    if (g.out0) cx_zero<AL, raw, VE>(g.out0, off, nval);
    if (g.out1) cx_zero<AL, int64_t, VE>(g.out1, off, nval);
  }
};

// the run sums: in0 grad, in1 indices (int64); out0 grad_in
template <typename E> struct cx_ext_bwd {
  using raw = typename E::raw; using A = typename E::acc;
  using S = cx_pair<A, int64_t>; using X = cx_none;
  static constexpr int VE = 16 / (int)sizeof(raw);
  static const char* name() { return E::name(); }
  static __device__ __forceinline__ S ident() { return {(A)0, (int64_t)-1}; }
  // the sum of the trailing elements that share the last run id, and that id
  static __device__ __forceinline__ S comb(const S& a, const S& b, int) {
    if (b.b < 0) return a;
    if (a.b < 0) return b;
    return a.b == b.b ? S{a.a + b.a, b.b} : b;
  }
  template <bool AL> static __device__ __forceinline__ void load(const cx_args& g, int64_t off, int nval, int64_t,
                                                                  S (&s)[VE], X (&)[VE]) {
    raw v[VE];
    int64_t id[VE];
    cx_ld<AL, raw, VE>(g.in0, off, nval, v);
    cx_ld<AL, int64_t, VE>(g.in1, off, nval, id);
#pragma unroll
    for (int e = 0; e < VE; ++e) s[e] = e < nval ? S{E::up(v[e]), id[e]} : ident();
  }
  template <bool AL> static __device__ __forceinline__ void store(const cx_args& g, int64_t off, int nval, int64_t t,
                                                                   const S (&s)[VE], const X (&)[VE]) {
    raw o[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) o[e] = s[e].b == t ? E::down(s[e].a) : (raw)0;
    cx_st<AL, raw, VE>(g.out0, off, nval, o);
  }
  template <bool AL> static __device__ __forceinline__ void zero(const cx_args& g, int64_t off, int nval) {
    cx_zero<AL, raw, VE>(g.out0, off, nval);
  }
};

// the weighted log-space fold, written once; BWD picks the load and the finish
//   forward:  in0 x; out0 y = m + log s
//   backward: in0 grad, in1 x, in2 y; out0 grad_in = s * exp(m + x)
template <typename E, bool BWD> struct cx_lse {
  using raw = typename E::raw; using A = typename E::acc;
  using S = cx_pair<A, A>;
  using X = typename std::conditional<BWD, A, cx_none>::type;
  static constexpr int VE = 16 / (int)sizeof(raw);
  static const char* name() { return E::name(); }
  static __device__ __forceinline__ S ident() { return {-seg_inf<A>(), (A)0}; }
  static __device__ __forceinline__ S comb(const S& a, const S& b, int) {
    const A ninf = -seg_inf<A>();
    if (b.a == ninf && b.b == (A)0) return a;
    if (a.a == ninf && a.b == (A)0) return b;
    const A M = a.a > b.a ? a.a : b.a;
    const A ea = a.a == M ? (A)1 : seg_exp(a.a - M), eb = b.a == M ? (A)1 : seg_exp(b.a - M);
    const A ta = a.b * ea, tb = b.b * eb;
    return {M, ta + tb};
  }
  template <bool AL> static __device__ __forceinline__ void load(const cx_args& g, int64_t off, int nval, int64_t,
                                                                  S (&s)[VE], X (&x)[VE]) {
    raw v[VE];
    cx_ld<AL, raw, VE>(g.in0, off, nval, v);
    if constexpr (BWD) {
      raw vx[VE], vy[VE];
      cx_ld<AL, raw, VE>(g.in1, off, nval, vx);
      cx_ld<AL, raw, VE>(g.in2, off, nval, vy);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A y = E::up(vy[e]);
        x[e] = E::up(vx[e]);
        s[e] = e < nval ? (y != y ? S{-seg_inf<A>(), seg_nan<A>()} : S{-y, E::up(v[e])}) : ident();
      }
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A xv = E::up(v[e]);
        s[e] = e < nval ? (xv != xv ? S{-seg_inf<A>(), seg_nan<A>()} : xv == -seg_inf<A>() ? ident() : S{xv, (A)1}) : ident();
      }
    }
  }
  template <bool AL> static __device__ __forceinline__ void store(const cx_args& g, int64_t off, int nval, int64_t,
                                                                   const S (&s)[VE], const X (&x)[VE]) {
    raw o[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if constexpr (BWD) o[e] = E::down(x[e] == -seg_inf<A>() ? (A)0 : s[e].b * seg_exp(s[e].a + x[e]));
      else o[e] = E::down(s[e].a + seg_log(s[e].b));
    }
    cx_st<AL, raw, VE>(g.out0, off, nval, o);
  }
  template <bool AL> static __device__ __forceinline__ void zero(const cx_args& g, int64_t off, int nval) {
    cx_zero<AL, raw, VE>(g.out0, off, nval);
  }
};

// ---------------------------------------------------------------- the order, in one place for every form
// what precedes a token of group `w` of a tile, given the tile's four group totals; `car` moves on by the tile's total
template <typename Op>
__device__ __forceinline__ typename Op::S cx_before(const typename Op::S& base, typename Op::S& car,
                                                    const typename Op::S& g0, const typename Op::S& g1,
                                                    const typename Op::S& g2, const typename Op::S& g3, int w, int flag) {
  using S = typename Op::S;
  const S s1 = Op::comb(g0, g1, flag), s2 = Op::comb(s1, g2, flag), tt = Op::comb(s2, g3, flag);
  const S groups = w == 0 ? Op::ident() : w == 1 ? g0 : w == 2 ? s1 : s2;
  const S pre = Op::comb(Op::comb(base, car, flag), groups, flag);
  car = Op::comb(car, tt, flag);
  return pre;
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// The geometry of seg_cumsum_lanes_kernel: a wave takes two sequences, 32 lanes each; lane r of a half is position r of
// a tile; doubling steps and group totals by shuffles; base and carry in registers from tile to tile.
template <typename Op, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_cumext_lanes_kernel(rua_layout L, cx_args g, int H, int rev) {
  using S = typename Op::S;
  using X = typename Op::X;
  constexpr int VE = Op::VE;
  constexpr int UNR = CX_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (CX_SLOTS - 1), gq = q & (CX_GROUP - 1), w = q / CX_GROUP;
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int flag = g.flag;

  S base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = Op::ident();

  for (int64_t u0 = 0; u0 < maxlen; u0 += (int64_t)CX_SLOTS * UNR) {
    S v[UNR][VE];
    X x[UNR][VE];
    int64_t rows[UNR], ts[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * CX_SLOTS + q;
      rows[k] = -1;
      ts[k] = 0;
#pragma unroll
      for (int e = 0; e < VE; ++e) v[k][e] = Op::ident();
      if (u < len) {
        const int64_t t = rev ? len - 1 - u : u;
        const int64_t row = token_to_row(L, b, t, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ts[k] = t;
          Op::template load<AL>(g, row * H, H, t, v[k], x[k]);
        }
      }
    }
#pragma unroll
    for (int d = 1; d < CX_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          const S from = cx_shfl_up(v[k][e], d, CX_SLOTS);
          if (gq >= d) v[k][e] = Op::comb(from, v[k][e], flag);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * CX_SLOTS;
      if (tile0 >= maxlen) break;                             // wave-uniform
      S o[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        o[e] = Op::ident();
        if (e >= H) continue;
        const S g0 = cx_shfl(v[k][e], CX_GROUP - 1, CX_SLOTS), g1 = cx_shfl(v[k][e], 2 * CX_GROUP - 1, CX_SLOTS);
        const S g2 = cx_shfl(v[k][e], 3 * CX_GROUP - 1, CX_SLOTS), g3 = cx_shfl(v[k][e], 4 * CX_GROUP - 1, CX_SLOTS);
        o[e] = Op::comb(cx_before<Op>(base[e], car[e], g0, g1, g2, g3, w, flag), v[k][e], flag);
      }
      if (rows[k] >= 0) Op::template store<AL>(g, rows[k] * H, H, ts[k], o, x[k]);
      if ((tile0 / CX_SLOTS + 1) % CX_TILES == 0) {           // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = Op::comb(base[e], car[e], flag); car[e] = Op::ident(); }
      }
    }
  }
  if (have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
    for (int64_t j = q; j < L.T_phys; j += CX_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) Op::template zero<AL>(g, row * H, H);
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// The geometry of seg_cumsum_rows_kernel: a workgroup per (sequence x 128-byte column chunk of the PAYLOAD), thread
// (q, l) = (tid / 8, tid % 8) is position q of a tile and owns the l-th vector of VE elements of the chunk.  A group is
// the 8 slots of one wave; the four group totals of a tile cross the waves through LDS — two tiles per barrier, two
// buffers in turn.  mode SEG_PARTIAL / SEG_FINISH: the cut form, a block's total state in `ws`.
template <typename Op, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_cumext_rows_kernel(rua_layout L, cx_args g, int64_t H, int n_chunks,
                                                                   int mode, int maxblk, typename Op::S* ws, int rev) {
  using S = typename Op::S;
  using X = typename Op::X;
  constexpr int VE = Op::VE;
  constexpr int CW = CX_LPR * VE;
  constexpr int UNR = CX_UNR;
  __shared__ S xch[2][UNR][RUA_WAVES_PER_BLOCK][CX_LPR][VE];

  const int tid = threadIdx.x;
  const int l = tid & (CX_LPR - 1), q = tid >> 3, w = tid >> 6, gq = q & (CX_GROUP - 1);
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode != SEG_FULL) { blk = (int)(b % maxblk); b /= maxblk; }
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: a CAT layout whose T_log understates a length
  // must not walk past the maxblk blocks that exist (rua.h: T_log has to be a true bound)
  const int64_t have_blk = (len + CX_BLOCK_TOK - 1) / CX_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode != SEG_FULL && blk > 0 && blk >= nblk) return;     // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  const int flag = g.flag;
  int64_t ub = 0, ue = len;                                  // positions along the scan
  if (mode != SEG_FULL) {
    ub = (int64_t)blk * CX_BLOCK_TOK;
    ue = len < ub + CX_BLOCK_TOK ? len : ub + CX_BLOCK_TOK;
    if (ub > ue) ub = ue;
  }

  S base[VE], car[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) base[e] = car[e] = Op::ident();
  if (mode == SEG_FINISH) {
    for (int64_t k = 0; k < blk; ++k) {
      const S* p = ws + ((((b * maxblk + k) * n_chunks + c) * CX_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) base[e] = Op::comb(base[e], p[e], flag);
    }
  }

  int buf = 0;
  for (int64_t u0 = ub; u0 < ue; u0 += (int64_t)CX_SLOTS * UNR, buf ^= 1) {
    S v[UNR][VE];
    X x[UNR][VE];
    int64_t rows[UNR], ts[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t u = u0 + (int64_t)k * CX_SLOTS + q;
      rows[k] = -1;
      ts[k] = 0;
#pragma unroll
      for (int e = 0; e < VE; ++e) v[k][e] = Op::ident();
      if (active && u < ue) {
        const int64_t t = rev ? len - 1 - u : u;
        const int64_t row = token_to_row(L, b, t, len);
        if (row >= 0 && row < L.n_rows) {
          rows[k] = row;
          ts[k] = t;
          Op::template load<AL>(g, row * H + col0, nval, t, v[k], x[k]);
        }
      }
    }
    // positions 0 .. 7 of a group sit 8 lanes apart
#pragma unroll
    for (int d = 1; d < CX_GROUP; d <<= 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const S from = cx_shfl_up(v[k][e], d * CX_LPR, RUA_WAVE);
          if (gq >= d) v[k][e] = Op::comb(from, v[k][e], flag);
        }
      }
    }
    if (gq == CX_GROUP - 1) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) xch[buf][k][w][l][e] = v[k][e];
      }
    }
    __syncthreads();       // (the other buffer is written next: whoever still reads this one has not passed the next barrier)
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int64_t tile0 = u0 + (int64_t)k * CX_SLOTS;
      if (tile0 >= ue) break;                                 // workgroup-uniform
      S o[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const S pre = cx_before<Op>(base[e], car[e], xch[buf][k][0][l][e], xch[buf][k][1][l][e], xch[buf][k][2][l][e],
                                    xch[buf][k][3][l][e], w, flag);
        o[e] = Op::comb(pre, v[k][e], flag);
      }
      if (mode != SEG_PARTIAL && rows[k] >= 0) Op::template store<AL>(g, rows[k] * H + col0, nval, ts[k], o, x[k]);
      if (mode == SEG_FULL && (tile0 / CX_SLOTS + 1) % CX_TILES == 0) {      // the block ends: its total joins the base
#pragma unroll
        for (int e = 0; e < VE; ++e) { base[e] = Op::comb(base[e], car[e], flag); car[e] = Op::ident(); }
      }
    }
  }
  if (mode == SEG_PARTIAL) {
    if (tid < CX_LPR) {
      S* p = ws + ((((b * maxblk + blk) * n_chunks + c) * CX_LPR + l) * VE);
#pragma unroll
      for (int e = 0; e < VE; ++e) p[e] = car[e];
    }
    return;
  }
  if (active && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
    for (int64_t j = q; j < L.T_phys; j += CX_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) Op::template zero<AL>(g, row * H + col0, nval);
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps one state per block and (padded) column: (value, position) and (sum, run id) are 16 bytes with the
// padding of the pair, (m, s) is two accumulators
static int cx_ws_per_column(int32_t dtype, bool lse) {
  return lse ? (seg_esize(dtype, false) == 8 ? 16 : 8) : 16;
}
static seg_plan cx_make_plan(const rua_layout& L, int64_t H, int32_t dtype, bool lse) {
  const int es = seg_esize(dtype, !lse);
  return seg_make_plan(L, H, es, cx_ws_per_column(dtype, lse));
}

// `bases`: every address of the launch ORed together (the int64 tensors too); `scan_rev`: the direction of THIS scan
template <typename Op>
static int cx_launch(const char* kname, const rua_layout& L, const cx_args& g, uint64_t bases, const seg_plan& plan,
                     int64_t H, int scan_rev, void* ws, hipStream_t s) {
  using raw = typename Op::raw;
  using S = typename Op::S;
  static_assert(sizeof(S) == 16 || sizeof(S) == 8, "cx_ws_per_column");
  const int64_t row_bytes = H * (int64_t)sizeof(raw);

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    const bool al = ln.W == 16;
    seg_trace("%s_lanes_kernel T=%s W=%d H=%d AL=%d rev=%d kind=%d op=%d", kname, Op::name(), ln.W, (int)H, (int)al,
              scan_rev, L.kind, g.flag);
    seg_with_al(al, [&](auto AL) {
      hipLaunchKernelGGL((seg_cumext_lanes_kernel<Op, decltype(AL)::value>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0,
                         s, L, g, (int)H, scan_rev);
    });
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(plan, L, row_bytes, bases, ws != nullptr);
  const seg_plan& p = r.p;
  if (!r.grid) return RUA_ERANGE;
  return seg_launch_rows(
      r,
      [&](int mode) {
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_cumext_rows_kernel<Op, decltype(AL)::value>), dim3((unsigned)r.grid), dim3(RUA_BLOCK), 0,
                             s, L, g, H, p.n_chunks, mode, r.cut ? p.maxblk : 1, (S*)ws, scan_rev);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("%s_rows_kernel T=%s AL=%d rev=%d kind=%d op=%d cut=1 phase=%s blocks=%d chunks=%d", kname, Op::name(),
                    (int)r.al, scan_rev, L.kind, g.flag, phase, p.maxblk, p.n_chunks);
        else
          seg_trace("%s_rows_kernel T=%s AL=%d rev=%d kind=%d op=%d cut=0 chunks=%d", kname, Op::name(), (int)r.al,
                    scan_rev, L.kind, g.flag, p.n_chunks);
      });
}

static uint64_t cx_or(const void* p) { return (uint64_t)(uintptr_t)p; }

// what the four entry points check after seg_check_entry, in this order: nothing to do (0), then the caller's null
// test, the payload size, the element alignment of the payload tensors (`pay`) and of the int64 tensors (`idx`)
static int cx_checks(const rua_layout* lay, int64_t H, bool any_null, uint64_t pay, uint64_t idx, int es, int& done) {
  done = 1;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (any_null) return RUA_EINVAL;
  if (seg_too_large(lay, H, 8)) return RUA_ERANGE;
  if (pay % es || idx % 8) return RUA_EALIGN;
  done = 0;
  return 0;
}

static int cx_extreme(const rua_layout* lay, const void* x, void* values, void* indices, int64_t H, int32_t dtype,
                      int32_t op, int32_t reverse, void* ws, void* stream) {
  const int es = seg_esize(dtype, true);
  int e, done;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (op != RUA_MAX && op != RUA_MIN) return RUA_EINVAL;
  const bool bad = !x || (!values && !indices) || (values && values == indices);
  e = cx_checks(lay, H, bad, cx_or(x) | cx_or(values), cx_or(indices), es, done);
  if (done) return e;
  const cx_args g = {x, nullptr, nullptr, values, indices, op};
  const uint64_t bases = cx_or(x) | cx_or(values) | cx_or(indices);
  const seg_plan plan = cx_make_plan(*lay, H, dtype, false);
#define RUA_CX(E) cx_launch<cx_ext<E>>("seg_cumextreme", *lay, g, bases, plan, H, reverse ? 1 : 0, ws, (hipStream_t)stream)
  if (dtype == RUA_I64) return RUA_CX(cx_i64);
  RUA_DISPATCH_FLOAT(dtype, RUA_CX);
#undef RUA_CX
}

static int cx_extreme_bwd(const rua_layout* lay, const void* grad, const void* indices, void* grad_in, int64_t H,
                          int32_t dtype, int32_t reverse, void* ws, void* stream) {
  const int es = seg_esize(dtype, false);
  int e, done;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  e = cx_checks(lay, H, !grad || !indices || !grad_in || grad_in == indices, cx_or(grad) | cx_or(grad_in),
                cx_or(indices), es, done);
  if (done) return e;
  const cx_args g = {grad, indices, nullptr, grad_in, nullptr, 0};
  const uint64_t bases = cx_or(grad) | cx_or(indices) | cx_or(grad_in);
  const seg_plan plan = cx_make_plan(*lay, H, dtype, false);
  // against the forward's direction
#define RUA_CX(E) cx_launch<cx_ext_bwd<E>>("seg_cumextreme_bwd", *lay, g, bases, plan, H, reverse ? 0 : 1, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CX);
#undef RUA_CX
}

static int cx_logcumsumexp(const rua_layout* lay, const void* x, void* out, int64_t H, int32_t dtype, int32_t reverse,
                           void* ws, void* stream) {
  const int es = seg_esize(dtype, false);
  int e, done;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  e = cx_checks(lay, H, !x || !out, cx_or(x) | cx_or(out), 0, es, done);
  if (done) return e;
  const cx_args g = {x, nullptr, nullptr, out, nullptr, 0};
  const seg_plan plan = cx_make_plan(*lay, H, dtype, true);
#define RUA_CX(E) cx_launch<cx_lse<E, false>>("seg_logcumsumexp", *lay, g, cx_or(x) | cx_or(out), plan, H, reverse ? 1 : 0, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CX);
#undef RUA_CX
}

static int cx_logcumsumexp_bwd(const rua_layout* lay, const void* grad, const void* x, const void* y, void* grad_in,
                               int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream) {
  const int es = seg_esize(dtype, false);
  int e, done;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  const uint64_t bases = cx_or(grad) | cx_or(x) | cx_or(y) | cx_or(grad_in);
  e = cx_checks(lay, H, !grad || !x || !y || !grad_in, bases, 0, es, done);
  if (done) return e;
  const cx_args g = {grad, x, y, grad_in, nullptr, 0};
  const seg_plan plan = cx_make_plan(*lay, H, dtype, true);
#define RUA_CX(E) cx_launch<cx_lse<E, true>>("seg_logcumsumexp_bwd", *lay, g, bases, plan, H, reverse ? 0 : 1, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CX);
#undef RUA_CX
}

}  // namespace rua

extern "C" int64_t rua_cumextreme_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::cx_make_plan(*lay, H, dtype, false).ws_bytes;
}

extern "C" int64_t rua_logcumsumexp_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::cx_make_plan(*lay, H, dtype, true).ws_bytes;
}

extern "C" int rua_segment_cumextreme(const rua_layout* lay, const void* data, void* values, void* indices, int64_t H,
                                      int32_t dtype, int32_t op, int32_t reverse, void* ws, void* stream) {
  return rua::cx_extreme(lay, data, values, indices, H, dtype, op, reverse, ws, stream);
}

extern "C" int rua_segment_cumextreme_backward(const rua_layout* lay, const void* grad, const void* indices,
                                               void* grad_in, int64_t H, int32_t dtype, int32_t reverse, void* ws,
                                               void* stream) {
  return rua::cx_extreme_bwd(lay, grad, indices, grad_in, H, dtype, reverse, ws, stream);
}

extern "C" int rua_segment_logcumsumexp(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype,
                                        int32_t reverse, void* ws, void* stream) {
  return rua::cx_logcumsumexp(lay, data, out, H, dtype, reverse, ws, stream);
}

extern "C" int rua_segment_logcumsumexp_backward(const rua_layout* lay, const void* grad, const void* data,
                                                 const void* out, void* grad_in, int64_t H, int32_t dtype,
                                                 int32_t reverse, void* ws, void* stream) {
  return rua::cx_logcumsumexp_bwd(lay, grad, data, out, grad_in, H, dtype, reverse, ws, stream);
}
