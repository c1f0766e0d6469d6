// rua_norm.hip — per-sequence mean / variance and standardize over the tokens of a C / L / P / R container, and their
// backwards (rua_segment_var_mean, rua_segment_standardize and the two *_backward; include/rua.h).  An extension: the
// reference's users spell it as segment_mean + repeat_interleave + sub + square + segment_mean + rsqrt + mul over [N, H]
// temporaries, for a CattedSequence only.
//
//   mean[b,h] = (1/n) sum_t x      M2[b,h] = sum_t (x - mean)^2      var = M2 / (n - c)      y = (x - mean) * rstd
//   rstd = 1 / sqrt(M2 / (n - c) + eps)
//
// ONE fold order per (sequence, column), the softmax's (rua_softmax.hip), whatever the layout, the kernel form, the
// alignment or the launch geometry:
//   - the tokens of a sequence are cut into BLOCKS of NM_BLOCK_TOK = 2 048 consecutive tokens;
//   - inside a block, SLOT r (of NM_SLOTS = 32) folds the tokens t = r (mod 32) in ascending order from the empty state
//     (n, mean, M2) = (0, 0, 0) with Welford's update; the k-th token of a chain multiplies by rk = 1 / k — ONE division
//     per token and thread, shared by the 4 or 8 columns the thread owns, instead of one per element;
//   - the 32 slots are joined by a butterfly over the slot number (xor 1, 2, 4, 8, 16) with Chan's pairwise formula.
//     The formula is NOT symmetric (mean = mean_a + delta * n_b / n keeps a constant column exact), so both partners
//     compute merge(lower slot, upper slot); this file is compiled without fp contraction, so they get the same bits;
//   - the block results are joined in ascending block order, merge(so far, block), from the empty state.
// The backward of standardize sums g and g * y in the same order with `+`.  fp32 accumulation (fp64 for RUA_F64), every
// output element rounded once.  Padding rows of a LEFT / RIGHT result are written as zeros in the same pass and are
// never read.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int NM_SLOTS = 32;               // parallel fold chains per (sequence, column)
constexpr int NM_BLOCK_TOK = SEG_BLOCK_TOK; // tokens per block = 64 per slot
constexpr int NM_LPR = 8;                  // row forms: 16-byte lanes per row chunk (128 bytes)
constexpr int NM_ROWS_UNR = 4;             // row forms: rows in flight per thread
constexpr int NM_LANES_UNR = 8;            // lanes form: tokens a lane keeps in registers (sequences up to 256 tokens)
constexpr int NM_LDS_BUDGET = 64 * 1024;   // per workgroup: two workgroups per CU, no opt-in for large dynamic LDS
enum { NM_STD = 0, NM_VM = 1, NM_BWD = 2 };  // standardize forward, var_mean (its first walk alone), standardize backward

__device__ __forceinline__ float nm_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double nm_sqrt(double v) { return sqrt(v); }

// ---------------------------------------------------------------- the fold
// Welford, rk = 1 / (tokens of the chain so far, this one included).  A NaN poisons (mean, M2); an infinity makes the
// mean infinite and M2 NaN (inf - inf) — both stay in their (sequence, column).  A constant column keeps d == 0: M2 == 0.
template <typename A> __device__ __forceinline__ void nm_fold(A& mean, A& m2, A x, A rk) {
  const A d = x - mean;
  mean = mean + d * rk;
  m2 = m2 + d * (x - mean);
}

// Chan: a <- merge(a, b), a the LOWER side (earlier slots / blocks).  An empty side leaves the other untouched.
template <typename A, int VE>
__device__ __forceinline__ void nm_merge(A& na, A* ma, A* qa, A nb, const A* mb, const A* qb) {
  if (nb == (A)0) return;
  if (na == (A)0) {
    na = nb;
#pragma unroll
    for (int e = 0; e < VE; ++e) { ma[e] = mb[e]; qa[e] = qb[e]; }
    return;
  }
  const A n = na + nb, f1 = nb / n, f2 = na * f1;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    const A d = mb[e] - ma[e];
    ma[e] = ma[e] + d * f1;
    qa[e] = (qa[e] + qb[e]) + (d * d) * f2;
  }
  na = n;
}

// a butterfly step: both partners compute merge(lower, upper) and keep it
template <typename A, int VE>
__device__ __forceinline__ void nm_join(bool lower, A& n, A* m, A* q, A n2, const A* m2, const A* q2) {
  A an = lower ? n : n2, bn = lower ? n2 : n, am[VE], aq[VE], bm[VE], bq[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    am[e] = lower ? m[e] : m2[e];
    aq[e] = lower ? q[e] : q2[e];
    bm[e] = lower ? m2[e] : m[e];
    bq[e] = lower ? q2[e] : q[e];
  }
  nm_merge<A, VE>(an, am, aq, bn, bm, bq);
  n = an;
#pragma unroll
  for (int e = 0; e < VE; ++e) { m[e] = am[e]; q[e] = aq[e]; }
}

// (n, M2) -> var and rstd; n - c <= 0 (an empty sequence included): NaN
template <typename A> __device__ __forceinline__ void nm_stats(A n, A m2, A corr, A eps, A& var, A& rstd) {
  const A dof = n - corr;
  if (dof > (A)0) {
    var = m2 / dof;
    rstd = (A)1 / nm_sqrt(var + eps);
  } else {
    var = seg_nan<A>();
    rstd = seg_nan<A>();
  }
}

// what walk 2 writes.  forward: (p, r) = (mean, rstd), v = x;  backward: (p, r, s) = (sum g / n, rstd, sum g y / (n - c)), v = y
template <int OP, typename A> __device__ __forceinline__ A nm_finish(A v, A g, A p, A r, A s) {
  if constexpr (OP == NM_BWD) return r * ((g - p) - v * s);
  else return (v - p) * r;
}

// the per-(sequence, column) factors of the backward from its two sums
template <typename A> __device__ __forceinline__ void nm_bwd_factors(A n, A corr, A& s1, A& s2) {
  const A dof = n - corr;
  s1 = n > (A)0 ? s1 / n : seg_nan<A>();
  s2 = dof > (A)0 ? s2 / dof : seg_nan<A>();
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// A wave takes two sequences, 32 lanes each; lane r of a half is slot r.  Sequences of up to 256 tokens stay in registers
// between the two walks; longer ones are read again.  o1 / o2: the [B, H] operands — NM_STD: rstd out (acc type, may be
// null); NM_VM: var out, mean out (either may be null; mean in the acc type when mean_acc); NM_BWD: rstd in.
template <typename E, int OP>
__global__ __launch_bounds__(RUA_BLOCK) void seg_norm_lanes_kernel(rua_layout L, const char* xin, const char* gin,
                                                                   char* out, void* o1, void* o2, int H, int W,
                                                                   typename E::acc corr, typename E::acc eps,
                                                                   int mean_acc) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = NM_LANES_UNR;
  constexpr bool BWD = OP == NM_BWD;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (NM_SLOTS - 1);
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);
  const bool keep = maxlen <= (int64_t)NM_SLOTS * UNR;

  struct alignas(16) Row { raw e[VE]; };
  Row vx[UNR], vg[UNR];
  A N = (A)0, P[VE], S[VE];                                  // forward: (n, mean, M2); backward: (sum g, sum g y)
#pragma unroll
  for (int e = 0; e < VE; ++e) { P[e] = (A)0; S[e] = (A)0; }

  for (int64_t t0 = 0; t0 < maxlen; t0 += NM_BLOCK_TOK) {
    A n = (A)0, p[VE], s[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) { p[e] = (A)0; s[e] = (A)0; }
    const int64_t t1 = len < t0 + NM_BLOCK_TOK ? len : t0 + NM_BLOCK_TOK;
    const int64_t t1w = maxlen < t0 + NM_BLOCK_TOK ? maxlen : t0 + NM_BLOCK_TOK;
    for (int64_t tt = t0; tt < t1w; tt += (int64_t)NM_SLOTS * UNR) {
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t t = tt + (int64_t)u * NM_SLOTS + q;
        ok[u] = false;
        if (t < t1) {
          const int64_t row = token_to_row(L, b, t, len);
          if (row >= 0 && row < L.n_rows) {
            ok[u] = true;
            ld_row_w(xin + row * nb, nb, W, &vx[u]);
            if constexpr (BWD) ld_row_w(gin + row * nb, nb, W, &vg[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (!ok[u]) continue;
        n = n + (A)1;
        const A rk = (A)1 / n;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          if constexpr (BWD) {
            const A y = E::up(vx[u].e[e]), g = E::up(vg[u].e[e]);
            p[e] = p[e] + g;
            s[e] = s[e] + g * y;
          } else {
            nm_fold(p[e], s[e], E::up(vx[u].e[e]), rk);
          }
        }
      }
    }
#pragma unroll
    for (int k = 1; k < NM_SLOTS; k <<= 1) {
      A p2[VE], s2[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) { p2[e] = seg_shfl_xor(p[e], k); s2[e] = seg_shfl_xor(s[e], k); }
      if constexpr (BWD) {
#pragma unroll
        for (int e = 0; e < VE; ++e) { p[e] = p[e] + p2[e]; s[e] = s[e] + s2[e]; }
      } else {
        const A n2 = seg_shfl_xor(n, k);
        nm_join<A, VE>((q & k) == 0, n, p, s, n2, p2, s2);
      }
    }
    if constexpr (BWD) {
#pragma unroll
      for (int e = 0; e < VE; ++e) { P[e] = P[e] + p[e]; S[e] = S[e] + s[e]; }
    } else {
      nm_merge<A, VE>(N, P, S, n, p, s);
    }
  }

  A R[VE];                                                   // rstd
#pragma unroll
  for (int e = 0; e < VE; ++e) R[e] = (A)0;
  if constexpr (BWD) {
    const A nn = (A)len;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (e >= H || !have) continue;
      R[e] = ((const A*)o1)[b * H + e];
      nm_bwd_factors(nn, corr, P[e], S[e]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (e >= H || !have) continue;
      A var;
      nm_stats(N, S[e], corr, eps, var, R[e]);
      if (q != 0) continue;
      if constexpr (OP == NM_VM) {
        const A mean = N > (A)0 ? P[e] : seg_nan<A>();
        if (o1) ((raw*)o1)[b * H + e] = E::down(var);
        if (o2) { if (mean_acc) ((A*)o2)[b * H + e] = mean; else ((raw*)o2)[b * H + e] = E::down(mean); }
      } else {
        if (o1) ((A*)o1)[b * H + e] = R[e];
      }
    }
  }
  if constexpr (OP == NM_VM) return;

  // walk 2
  for (int64_t tt = 0; tt < len; tt += (int64_t)NM_SLOTS * UNR) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t t = tt + (int64_t)u * NM_SLOTS + q;
      if (t >= len) continue;
      const int64_t row = token_to_row(L, b, t, len);
      if (row < 0 || row >= L.n_rows) continue;
      if (!keep) {
        ld_row_w(xin + row * nb, nb, W, &vx[u]);
        if constexpr (BWD) ld_row_w(gin + row * nb, nb, W, &vg[u]);
      }
      Row o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A g = BWD ? E::up(vg[u].e[e]) : (A)0;
        o.e[e] = E::down(nm_finish<OP, A>(E::up(vx[u].e[e]), g, P[e], R[e], S[e]));
      }
      st_row_w(out + row * nb, nb, W, &o);
    }
  }
  if (have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
    Row z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = E::down((A)0);
    for (int64_t j = q; j < L.T_phys; j += NM_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st_row_w(out + row * nb, nb, W, &z);
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup takes (sequence x 128-byte column chunk): thread (q, l) = (tid / 8, tid % 8) is slot q and owns the l-th
// 16-byte vector of the chunk.  RESIDENT (len <= cap_rows): walk 1 parks every vector in LDS in the payload dtype — each
// thread reads back exactly what it stored, so the slab needs no barrier — and walk 2 rewrites out of LDS: the payload
// crosses HBM once.  Otherwise STREAMING: walk 2 reads global memory again.  mode SEG_PARTIAL / SEG_FINISH: the CUT form —
// a workgroup per (sequence, block of 2 048 tokens, chunk) leaves its block's (mean, M2) (backward: the two sums) in
// `ws`; a second launch joins them in block order — the block's n follows from the length — and rewrites the rows.
// NM_VM has no walk 2: its finish is a grid of (sequence x chunk) workgroups that write [B, H].
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.
template <typename E, int OP, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_norm_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                  const typename E::raw* gin, typename E::raw* out,
                                                                  void* o1, void* o2, int64_t H, int n_chunks,
                                                                  int cap_rows, int mode, int maxblk, int gridblk,
                                                                  typename E::acc* ws, typename E::acc corr,
                                                                  typename E::acc eps, int mean_acc) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = NM_LPR * VE;
  constexpr int UNR = NM_ROWS_UNR;
  constexpr bool BWD = OP == NM_BWD;
  constexpr int STR = 2 * VE + 1;                          // a thread's state: p[VE], s[VE], n
  constexpr int XCH_BYTES = (RUA_WAVES_PER_BLOCK * NM_LPR * STR * (int)sizeof(A) + 15) / 16 * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  A* xch = (A*)smem;                                       // [wave][l][STR]
  struct alignas(16) Vec { raw e[VE]; };
  Vec* slab = (Vec*)(smem + XCH_BYTES);                    // [row][l] (+ the same again for g in the backward)

  const int tid = threadIdx.x;
  const int l = tid & (NM_LPR - 1), q = tid >> 3;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode != SEG_FULL) { blk = (int)(b % gridblk); b /= gridblk; }   // (gridblk: maxblk, or 1 for var_mean's finish)
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: a CAT layout whose T_log understates a length
  // must not walk past the maxblk blocks that exist (rua.h: T_log has to be a true bound)
  const int64_t have_blk = (len + NM_BLOCK_TOK - 1) / NM_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode != SEG_FULL && blk > 0 && blk >= nblk) return;   // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  int64_t tb = 0, te = len;
  if (mode != SEG_FULL) {
    tb = (int64_t)blk * NM_BLOCK_TOK;
    te = len < tb + NM_BLOCK_TOK ? len : tb + NM_BLOCK_TOK;
    if (tb > te) tb = te;
  }
  const bool resident = mode == SEG_FULL && OP != NM_VM && len <= cap_rows;

  auto ld = [&](const raw* base, int64_t row, Vec& v) {
    const raw* p = base + row * H + col0;
    if constexpr (AL) {
      *(uint4*)&v = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = e < nval ? p[e] : E::down((A)0);
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

  A N = (A)0, P[VE], S[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { P[e] = (A)0; S[e] = (A)0; }

  if (mode == SEG_FINISH) {
    for (int64_t k = 0; k < nblk; ++k) {
      const A* pw = ws + ((((b * maxblk + k) * n_chunks + c) * NM_LPR + l) * VE) * 2;
      A p[VE], s[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) { p[e] = pw[e * 2]; s[e] = pw[e * 2 + 1]; }
      if constexpr (BWD) {
#pragma unroll
        for (int e = 0; e < VE; ++e) { P[e] = P[e] + p[e]; S[e] = S[e] + s[e]; }
      } else {
        const int64_t left = len - k * NM_BLOCK_TOK;
        nm_merge<A, VE>(N, P, S, (A)(left < NM_BLOCK_TOK ? left : NM_BLOCK_TOK), p, s);
      }
    }
  } else {
    for (int64_t t0 = tb; t0 < te; t0 += NM_BLOCK_TOK) {
      A n = (A)0, p[VE], s[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) { p[e] = (A)0; s[e] = (A)0; }
      const int64_t t1 = te < t0 + NM_BLOCK_TOK ? te : t0 + NM_BLOCK_TOK;
      if (active) {
        for (int64_t tt = t0 + q; tt < t1; tt += (int64_t)NM_SLOTS * UNR) {
          Vec vx[UNR], vg[UNR];
          bool ok[UNR];
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int64_t t = tt + (int64_t)u * NM_SLOTS;
            ok[u] = false;
            if (t < t1) {
              const int64_t row = token_to_row(L, b, t, len);
              if (row >= 0 && row < L.n_rows) {
                ok[u] = true;
                ld(xin, row, vx[u]);
                if constexpr (BWD) ld(gin, row, vg[u]);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int64_t t = tt + (int64_t)u * NM_SLOTS;
            if (!ok[u]) continue;
            if (resident) {
              slab[t * NM_LPR + l] = vx[u];
              if constexpr (BWD) slab[((int64_t)cap_rows + t) * NM_LPR + l] = vg[u];
            }
            n = n + (A)1;
            const A rk = (A)1 / n;
#pragma unroll
            for (int e = 0; e < VE; ++e) {
              if constexpr (BWD) {
                const A y = E::up(vx[u].e[e]), g = E::up(vg[u].e[e]);
                p[e] = p[e] + g;
                s[e] = s[e] + g * y;
              } else {
                nm_fold(p[e], s[e], E::up(vx[u].e[e]), rk);
              }
            }
          }
        }
      }
      // slots 0 .. 7 of a wave: xor 8, 16, 32 of the lane number = xor 1, 2, 4 of the slot number
#pragma unroll
      for (int k = NM_LPR; k < RUA_WAVE; k <<= 1) {
        A p2[VE], s2[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) { p2[e] = seg_shfl_xor(p[e], k); s2[e] = seg_shfl_xor(s[e], k); }
        if constexpr (BWD) {
#pragma unroll
          for (int e = 0; e < VE; ++e) { p[e] = p[e] + p2[e]; s[e] = s[e] + s2[e]; }
        } else {
          const A n2 = seg_shfl_xor(n, k);
          nm_join<A, VE>((lane & k) == 0, n, p, s, n2, p2, s2);
        }
      }
      // slot bits 8, 16 = wave bits 1, 2, through LDS: every thread computes merge(merge(W0, W1), merge(W2, W3))
      __syncthreads();
      if (lane < NM_LPR) {
        A* x = xch + (w * NM_LPR + l) * STR;
#pragma unroll
        for (int e = 0; e < VE; ++e) { x[e] = p[e]; x[VE + e] = s[e]; }
        x[2 * VE] = n;
      }
      __syncthreads();
      {
        A vn[RUA_WAVES_PER_BLOCK], vp[RUA_WAVES_PER_BLOCK][VE], vs[RUA_WAVES_PER_BLOCK][VE];
#pragma unroll
        for (int k = 0; k < RUA_WAVES_PER_BLOCK; ++k) {
          const A* x = xch + (k * NM_LPR + l) * STR;
#pragma unroll
          for (int e = 0; e < VE; ++e) { vp[k][e] = x[e]; vs[k][e] = x[VE + e]; }
          vn[k] = x[2 * VE];
        }
        if constexpr (BWD) {
#pragma unroll
          for (int e = 0; e < VE; ++e) {
            p[e] = (vp[0][e] + vp[1][e]) + (vp[2][e] + vp[3][e]);
            s[e] = (vs[0][e] + vs[1][e]) + (vs[2][e] + vs[3][e]);
          }
        } else {
          nm_merge<A, VE>(vn[0], vp[0], vs[0], vn[1], vp[1], vs[1]);
          nm_merge<A, VE>(vn[2], vp[2], vs[2], vn[3], vp[3], vs[3]);
          nm_merge<A, VE>(vn[0], vp[0], vs[0], vn[2], vp[2], vs[2]);
          n = vn[0];
#pragma unroll
          for (int e = 0; e < VE; ++e) { p[e] = vp[0][e]; s[e] = vs[0][e]; }
        }
      }
      if (mode == SEG_PARTIAL) {
        if (tid < NM_LPR) {
          A* pw = ws + ((((b * maxblk + blk) * n_chunks + c) * NM_LPR + l) * VE) * 2;
#pragma unroll
          for (int e = 0; e < VE; ++e) { pw[e * 2] = p[e]; pw[e * 2 + 1] = s[e]; }
        }
      } else {
        if constexpr (BWD) {
#pragma unroll
          for (int e = 0; e < VE; ++e) { P[e] = P[e] + p[e]; S[e] = S[e] + s[e]; }
        } else {
          nm_merge<A, VE>(N, P, S, n, p, s);
        }
      }
    }
    if (mode == SEG_PARTIAL) return;
  }
  if (!active) return;

  A R[VE];
  if constexpr (BWD) {
    const A nn = (A)len;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      R[e] = e < nval ? ((const A*)o1)[b * H + col0 + e] : (A)0;
      nm_bwd_factors(nn, corr, P[e], S[e]);
    }
  } else {
    const bool writer = q == 0 && blk == 0;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      A var;
      nm_stats(N, S[e], corr, eps, var, R[e]);
      if (!writer || e >= nval) continue;
      const int64_t at = b * H + col0 + e;
      if constexpr (OP == NM_VM) {
        const A mean = N > (A)0 ? P[e] : seg_nan<A>();
        if (o1) ((raw*)o1)[at] = E::down(var);
        if (o2) { if (mean_acc) ((A*)o2)[at] = mean; else ((raw*)o2)[at] = E::down(mean); }
      } else {
        if (o1) ((A*)o1)[at] = R[e];
      }
    }
  }
  if constexpr (OP == NM_VM) return;

  // walk 2
  for (int64_t tt = tb + q; tt < te; tt += (int64_t)NM_SLOTS * UNR) {
    Vec vx[UNR], vg[UNR];
    int64_t rows[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t t = tt + (int64_t)u * NM_SLOTS;
      rows[u] = -1;
      if (t >= te) continue;
      const int64_t row = token_to_row(L, b, t, len);
      if (row < 0 || row >= L.n_rows) continue;
      rows[u] = row;
      if (resident) {
        vx[u] = slab[t * NM_LPR + l];
        if constexpr (BWD) vg[u] = slab[((int64_t)cap_rows + t) * NM_LPR + l];
      } else {
        ld(xin, row, vx[u]);
        if constexpr (BWD) ld(gin, row, vg[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (rows[u] < 0) continue;
      Vec o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A g = BWD ? E::up(vg[u].e[e]) : (A)0;
        o.e[e] = E::down(nm_finish<OP, A>(E::up(vx[u].e[e]), g, P[e], R[e], S[e]));
      }
      st(rows[u], o);
    }
  }
  if ((L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
    Vec z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = E::down((A)0);
    for (int64_t j = q; j < L.T_phys; j += NM_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st(row, z);
    }
  }
}

// ---------------------------------------------------------------- backward of var_mean: token-parallel
//   grad_in = grad_var[b,h] * 2 (x - mean[b,h]) / (n - c) + grad_mean[b,h] / n
// One form: workgroup (b, part) strides the sequence's (token, column) pairs from `part`, elementwise — any width, any
// alignment.  Padding rows of a LEFT / RIGHT gradient are written as zeros by the same workgroups.
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_var_mean_backward_kernel(rua_layout L, const typename E::raw* x,
                                                                          const void* mean, int mean_acc,
                                                                          const typename E::raw* gvar,
                                                                          const typename E::raw* gmean,
                                                                          typename E::raw* out, int64_t H, int parts,
                                                                          typename E::acc corr) {
  using A = typename E::acc;
  const int64_t b = blockIdx.x / (unsigned)parts;
  const int part = (int)(blockIdx.x % (unsigned)parts);
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  const A n = (A)len, dof = n - corr;
  const int64_t stride = (int64_t)parts * RUA_BLOCK;
  const int64_t total = len * H;
  for (int64_t i = (int64_t)part * RUA_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t t = div_rows(i, H), h = i - t * H;
    const int64_t row = token_to_row(L, b, t, len);
    if (row < 0 || row >= L.n_rows) continue;
    const int64_t at = b * H + h;
    A v = (A)0;
    if (gvar) {
      const A mu = mean_acc ? ((const A*)mean)[at] : E::up(((const typename E::raw*)mean)[at]);
      v = dof > (A)0 ? E::up(gvar[at]) * ((A)2 * (E::up(x[row * H + h]) - mu)) / dof : seg_nan<A>();
    }
    if (gmean) v = v + E::up(gmean[at]) / n;
    out[row * H + h] = E::down(v);
  }
  if (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) {
    const int64_t padtot = L.T_phys * H;
    for (int64_t i = (int64_t)part * RUA_BLOCK + threadIdx.x; i < padtot; i += stride) {
      const int64_t j = i / H;
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) out[row * H + (i - j * H)] = E::down((A)0);
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps (mean, M2), or the backward's two sums, per block and padded column: two accumulators
static seg_plan nm_make_plan(const rua_layout& L, int64_t H, int32_t dtype) {
  const int es = seg_esize(dtype, false);
  return seg_make_plan(L, H, es, 2 * (es == 8 ? 8 : 4));
}

static const char* nm_opname(int op) { return op == NM_VM ? "var_mean" : "standardize"; }

template <typename E, int OP>
static int nm_launch(const rua_layout& L, const void* x, const void* g, void* out, void* o1, void* o2, int64_t H,
                     int32_t dtype, int64_t correction, double eps_d, int mean_acc, void* ws, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr bool BWD = OP == NM_BWD;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t bases = (uint64_t)(uintptr_t)x | (uint64_t)(uintptr_t)g | (uint64_t)(uintptr_t)out;
  const char* dir = BWD ? "_backward" : "";
  const A corr = (A)correction, eps = (A)eps_d;
  if (bases % sizeof(raw)) return RUA_EALIGN;                 // (elements themselves are always aligned)
  if ((uint64_t)(uintptr_t)o1 % (OP == NM_VM ? sizeof(raw) : sizeof(A)) ||
      (uint64_t)(uintptr_t)o2 % (mean_acc ? sizeof(A) : sizeof(raw)))
    return RUA_EALIGN;

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    seg_trace("seg_norm%s_lanes_kernel T=%s AL=%d W=%d H=%d kind=%d cut=0 op=%s", dir, E::name(), (int)(ln.W == 16), ln.W,
              (int)H, L.kind, nm_opname(OP));
    hipLaunchKernelGGL((seg_norm_lanes_kernel<E, OP>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, L, (const char*)x,
                       (const char*)g, (char*)out, o1, o2, (int)H, ln.W, corr, eps, mean_acc);
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(nm_make_plan(L, H, dtype), L, row_bytes, bases, ws != nullptr);
  const seg_plan& p = r.p;
  constexpr int XCH_BYTES = (RUA_WAVES_PER_BLOCK * NM_LPR * (2 * VE + 1) * (int)sizeof(A) + 15) / 16 * 16;
  // the slab's cap from the LDS budget: what 64 KiB leave after the exchange area, in rows of 128 bytes (two slabs in
  // the backward), rounded down to whole rounds of the 32 slots — 480 rows forward, 224 backward
  constexpr int CAP = (NM_LDS_BUDGET - XCH_BYTES) / (128 * (BWD ? 2 : 1)) / NM_SLOTS * NM_SLOTS;
  const int cap = OP != NM_VM ? seg_slab_cap(L, r.cut, NM_SLOTS, CAP) : 0;     // (var_mean has no second walk)
  const size_t lds = XCH_BYTES + (size_t)cap * 128 * (BWD ? 2 : 1);
  if (!r.grid) return RUA_ERANGE;
  return seg_launch_rows(
      r,
      [&](int mode) {
        // blocks per unit in this launch's grid; var_mean's finish rewrites no rows: one workgroup per unit
        const int gridblk = mode == SEG_FULL || (mode == SEG_FINISH && OP == NM_VM) ? 1 : p.maxblk;
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_norm_rows_kernel<E, OP, decltype(AL)::value>),
                             dim3((unsigned)(L.B * (int64_t)p.n_chunks * gridblk)), dim3(RUA_BLOCK), lds, s, L,
                             (const raw*)x, (const raw*)g, (raw*)out, o1, o2, H, p.n_chunks, cap, mode,
                             r.cut ? p.maxblk : 1, gridblk, (A*)ws, corr, eps, mean_acc);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("seg_norm%s_stream_kernel T=%s AL=%d kind=%d cut=1 phase=%s cap=0 op=%s blocks=%d chunks=%d", dir,
                    E::name(), (int)r.al, L.kind, phase, nm_opname(OP), p.maxblk, p.n_chunks);
        else
          seg_trace("seg_norm%s_%s_kernel T=%s AL=%d kind=%d cut=0 phase=full cap=%d op=%s chunks=%d", dir,
                    cap > 0 ? "resident" : "stream", E::name(), (int)r.al, L.kind, cap, nm_opname(OP), p.n_chunks);
      });
}

template <typename E>
static int nm_launch_vm_backward(const rua_layout& L, const void* x, const void* mean, int mean_acc, const void* gvar,
                                 const void* gmean, void* out, int64_t H, int64_t correction, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  const uint64_t bases = (uint64_t)(uintptr_t)x | (uint64_t)(uintptr_t)gvar | (uint64_t)(uintptr_t)gmean |
                         (uint64_t)(uintptr_t)out;
  if (bases % sizeof(raw) || (uint64_t)(uintptr_t)mean % (mean_acc ? sizeof(A) : sizeof(raw))) return RUA_EALIGN;
  // enough workgroups per sequence for 16 elements per thread at the length bound, at most 64
  const double elems = (double)sm_len_bound(L) * (double)H;
  int parts = (int)(elems / (16.0 * RUA_BLOCK) > 64.0 ? 64.0 : elems / (16.0 * RUA_BLOCK));
  if (parts < 1) parts = 1;
  const int64_t grid = L.B * (int64_t)parts;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_var_mean_backward_kernel T=%s AL=0 kind=%d cut=0 op=var_mean parts=%d", E::name(), L.kind, parts);
  hipLaunchKernelGGL((seg_var_mean_backward_kernel<E>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L, (const raw*)x,
                     mean, mean_acc, (const raw*)gvar, (const raw*)gmean, (raw*)out, H, parts, (A)correction);
  return (int)hipGetLastError();
}

// the checks every entry shares; `dtype` loses its RUA_NORM_MEAN_ACC bit
static int nm_check(const rua_layout* lay, int64_t H, int32_t& dtype, int64_t correction, double eps, int& mean_acc) {
  mean_acc = (dtype >= 0 && (dtype & RUA_NORM_MEAN_ACC)) ? 1 : 0;
  if (dtype >= 0) dtype &= ~RUA_NORM_MEAN_ACC;
  const int e = seg_check_entry(lay, H, seg_esize(dtype, false));
  if (e != 0) return e;
  return correction < 0 || !(eps >= 0.0) ? RUA_EINVAL : 0;
}

template <int OP>
static int nm_dispatch(const rua_layout* lay, const void* x, const void* g, void* out, void* o1, void* o2, int64_t H,
                       int32_t dtype, int64_t correction, double eps, int mean_acc, void* ws, void* stream) {
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!x || (OP != NM_VM && !out) || (OP == NM_BWD && (!g || !o1))) return RUA_EINVAL;
  if (seg_too_large(lay, H, seg_esize(dtype, false))) return RUA_ERANGE;
#define RUA_NM(E) nm_launch<E, OP>(*lay, x, g, out, o1, o2, H, dtype, correction, eps, mean_acc, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_NM);
#undef RUA_NM
}

}  // namespace rua

extern "C" int64_t rua_norm_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  if (dtype >= 0) dtype &= ~RUA_NORM_MEAN_ACC;
  return rua::nm_make_plan(*lay, H, dtype).ws_bytes;
}

extern "C" int rua_segment_var_mean(const rua_layout* lay, const void* data, void* var, void* mean, int64_t H,
                                    int32_t dtype, int64_t correction, void* ws, void* stream) {
  using namespace rua;
  int e, macc;
  if ((e = nm_check(lay, H, dtype, correction, 0.0, macc)) != 0) return e;
  if ((var && var == data) || (mean && mean == data) || (var && var == mean)) return RUA_EINVAL;
  if (!var && !mean) return 0;
  return nm_dispatch<NM_VM>(lay, data, nullptr, nullptr, var, mean, H, dtype, correction, 0.0, macc, ws, stream);
}

extern "C" int rua_segment_var_mean_backward(const rua_layout* lay, const void* data, const void* mean,
                                             const void* grad_var, const void* grad_mean, void* grad_in, int64_t H,
                                             int32_t dtype, int64_t correction, void* stream) {
  using namespace rua;
  int e, macc;
  if ((e = nm_check(lay, H, dtype, correction, 0.0, macc)) != 0) return e;
  if (grad_in && (grad_in == mean || grad_in == grad_var || grad_in == grad_mean)) return RUA_EINVAL;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!data || !mean || !grad_in) return RUA_EINVAL;
  if (seg_too_large(lay, H, seg_esize(dtype, false))) return RUA_ERANGE;
#define RUA_NM_VMB(E)                                                                                                  \
  nm_launch_vm_backward<E>(*lay, data, mean, macc, grad_var, grad_mean, grad_in, H, correction, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_NM_VMB);
#undef RUA_NM_VMB
}

extern "C" int rua_segment_standardize(const rua_layout* lay, const void* data, void* out, void* rstd, int64_t H,
                                       int32_t dtype, int64_t correction, double eps, void* ws, void* stream) {
  using namespace rua;
  int e, macc;
  if ((e = nm_check(lay, H, dtype, correction, eps, macc)) != 0) return e;
  if (rstd && (rstd == data || rstd == out)) return RUA_EINVAL;
  return nm_dispatch<NM_STD>(lay, data, nullptr, out, rstd, nullptr, H, dtype, correction, eps, 0, ws, stream);
}

extern "C" int rua_segment_standardize_backward(const rua_layout* lay, const void* y, const void* rstd,
                                                const void* grad_out, void* grad_in, int64_t H, int32_t dtype,
                                                int64_t correction, void* ws, void* stream) {
  using namespace rua;
  int e, macc;
  if ((e = nm_check(lay, H, dtype, correction, 0.0, macc)) != 0) return e;
  if ((y && y == grad_in) || (rstd && rstd == grad_in)) return RUA_EINVAL;
  return nm_dispatch<NM_BWD>(lay, y, grad_out, grad_in, const_cast<void*>(rstd), nullptr, H, dtype, correction, 0.0, 0,
                             ws, stream);
}
