// rua_pool.hip — per-sequence softmax-weighted sum (attention pooling) over the tokens of a C / L / P / R container, and
// its backward (rua_segment_softmax_pool, rua_segment_softmax_pool_backward; include/rua.h).  An extension: the
// reference's users spell it as segment_logsumexp + repeat_interleave + exp, a broadcast multiply and segment_sum over
// [N, H] temporaries, for a CattedSequence only.
//
//   out[b, h] = sum over t < len[b] of softmax_t(scores[b, :, h / D])[t] * values[b, t, h]          G = H / D score columns
//
// FORWARD.  The softmax's fold (rua_softmax.hip) with the weighted accumulator added to the folded state: (m, l, acc) =
// (running max, sum of exp(s - m), sum of exp(s - m) * v).  ONE fold order per (sequence, column), whatever the layout,
// the kernel form's access width or the alignment:
//   - the tokens of a sequence are cut into BLOCKS of PL_BLOCK_TOK = 2 048 consecutive tokens;
//   - inside a block, SLOT r (of PL_SLOTS = 32) folds the tokens t = r (mod 32) in ascending order from the identity
//     (-inf, 0, 0) with the one-exp online update `pl_fold`;
//   - the 32 slots are combined by a butterfly over the slot number (xor 1, 2, 4, 8, 16); the combine rescales both
//     sides to max(m, m') and is symmetric in its arguments, and this file is compiled without fp contraction, so both
//     partners compute the same bits;
//   - the block results are combined in ascending block order, starting from the identity.
// out = acc / l, rounded once; lse = m + log(l).  The values cross HBM once, the scores once per 128-byte column chunk.
// Columns of one score column carry the same (m, l) bits: the state is computed once per score column and copied.
//
// BACKWARD.  Token-parallel given lse: p = exp(s - lse), grad_values = p * g, grad_scores = p * (dot_D(v, g) - delta),
// delta = dot_D(out, g).  The dot over the D columns of a score column has ONE order, fixed by (H, D, dtype): in the
// lanes form ascending; in the team form the columns are dealt in units (16 bytes when D is a multiple of that, else one
// element) to the S = min(64, pow2ceil(units)) slots of a team of lanes round-robin, every slot sums ascending and the
// slots are joined by a butterfly.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int PL_SLOTS = 32;               // parallel fold chains per (sequence, column)
constexpr int PL_BLOCK_TOK = SEG_BLOCK_TOK; // tokens per block = 64 per slot
constexpr int PL_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int PL_ROWS_UNR = 4;             // rows form: rows in flight per thread
constexpr int PL_LANES_UNR = 4;            // lanes form: tokens in flight per lane

// ---------------------------------------------------------------- the fold
// online (max, sum) with one exp per score; the caller then updates acc = acc * scale + p * v.  NaN and +inf poison the
// sum (the whole score column of the sequence is NaN); a -inf score has weight 0 — and 0 * v still poisons acc where v is
// not finite, as torch's softmax * values does.
template <typename A> __device__ __forceinline__ void pl_fold(A& m, A& l, A x, A& scale, A& p) {
  const A inf = seg_inf<A>();
  scale = (A)1;
  p = (A)0;
  if (!(x < inf)) {
    l = seg_nan<A>();
  } else if (x > m) {
    scale = seg_exp(m - x);
    l = l * scale + (A)1;
    p = (A)1;
    m = x;
  } else if (x > -inf) {
    p = seg_exp(x - m);
    l = l + p;
  }
}

// the factors that bring two states to their common max: symmetric (pl_factors(m2, m, M, fb, fa) gives the same bits)
template <typename A> __device__ __forceinline__ void pl_factors(A m, A m2, A& M, A& fa, A& fb) {
  M = m > m2 ? m : m2;
  if (M == -seg_inf<A>()) {
    fa = (A)1;
    fb = (A)1;
  } else {
    fa = seg_exp(m - M);
    fb = seg_exp(m2 - M);
  }
}

// ---------------------------------------------------------------- forward, lanes along time: rows of one vector
// A wave takes two sequences, 32 lanes each; lane r of a half is slot r.  Every lane keeps the state of all H <= VE
// columns of the row.
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_pool_lanes_kernel(rua_layout L, const char* vin,
                                                                   const typename E::raw* sin, void* out, int out_acc,
                                                                   typename E::acc* lse, int H, int D, int G, int W) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = PL_LANES_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (PL_SLOTS - 1);
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);

  int gc[VE];                                                // the score column of element e
  bool first[VE];                                            // ... and whether e opens it
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    gc[e] = e < H ? e / D : 0;
    first[e] = e == 0 || gc[e] != gc[e > 0 ? e - 1 : 0];
  }

  struct alignas(16) Row { raw e[VE]; };
  A M[VE], S[VE], ACC[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { M[e] = -seg_inf<A>(); S[e] = (A)0; ACC[e] = (A)0; }

  for (int64_t t0 = 0; t0 < maxlen; t0 += PL_BLOCK_TOK) {
    A m[VE], s[VE], acc[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) { m[e] = -seg_inf<A>(); s[e] = (A)0; acc[e] = (A)0; }
    const int64_t t1 = len < t0 + PL_BLOCK_TOK ? len : t0 + PL_BLOCK_TOK;
    const int64_t t1w = maxlen < t0 + PL_BLOCK_TOK ? maxlen : t0 + PL_BLOCK_TOK;
    for (int64_t tt = t0; tt < t1w; tt += (int64_t)PL_SLOTS * UNR) {
      bool ok[UNR];
      Row vx[UNR];
      A sx[UNR][VE];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t t = tt + (int64_t)u * PL_SLOTS + q;
        ok[u] = false;
        if (t < t1) {
          const int64_t row = token_to_row(L, b, t, len);
          if (row >= 0 && row < L.n_rows) {
            ok[u] = true;
            ld_row_w(vin + row * nb, nb, W, &vx[u]);
#pragma unroll
            for (int e = 0; e < VE; ++e)
              if (e < H && first[e]) sx[u][e] = E::up(sin[row * G + gc[e]]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (!ok[u]) continue;
        A scale = (A)1, p = (A)0;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          if (first[e]) {
            pl_fold(m[e], s[e], sx[u][e], scale, p);
          } else {
            m[e] = m[e > 0 ? e - 1 : 0];
            s[e] = s[e > 0 ? e - 1 : 0];
          }
          acc[e] = acc[e] * scale + p * E::up(vx[u].e[e]);
        }
      }
    }
#pragma unroll
    for (int k = 1; k < PL_SLOTS; k <<= 1) {
      A Mx = (A)0, fa = (A)1, fb = (A)1;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (e >= H) continue;
        const A a2 = seg_shfl_xor(acc[e], k);
        if (first[e]) {
          const A m2 = seg_shfl_xor(m[e], k), s2 = seg_shfl_xor(s[e], k);
          pl_factors(m[e], m2, Mx, fa, fb);
          s[e] = s[e] * fa + s2 * fb;
          m[e] = Mx;
        } else {
          m[e] = m[e > 0 ? e - 1 : 0];
          s[e] = s[e > 0 ? e - 1 : 0];
        }
        acc[e] = acc[e] * fa + a2 * fb;
      }
    }
    {
      A Mx = (A)0, fa = (A)1, fb = (A)1;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (e >= H) continue;
        if (first[e]) {
          pl_factors(M[e], m[e], Mx, fa, fb);
          S[e] = S[e] * fa + s[e] * fb;
          M[e] = Mx;
        } else {
          M[e] = M[e > 0 ? e - 1 : 0];
          S[e] = S[e > 0 ? e - 1 : 0];
        }
        ACC[e] = ACC[e] * fa + acc[e] * fb;
      }
    }
  }
  if (!have || q != 0) return;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (e >= H) continue;
    const A o = len > 0 ? ACC[e] / S[e] : (A)0;
    if (out_acc) ((A*)out)[b * H + e] = o; else ((raw*)out)[b * H + e] = E::down(o);
    if (lse && first[e]) lse[b * G + gc[e]] = M[e] + seg_log(S[e]);
  }
}

// ---------------------------------------------------------------- forward, rows wider than one vector
// A workgroup takes (sequence x 128-byte column chunk): thread (q, l) = (tid / 8, tid % 8) is slot q and owns the l-th
// 16-byte vector of the chunk.  LANE: D is a multiple of the vector, so a thread's elements share ONE score column and
// one (m, l); otherwise every element carries its own (copied from its neighbour where the two share the score column).
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.
template <typename E, bool AL, bool LANE>
__global__ __launch_bounds__(RUA_BLOCK) void seg_pool_rows_kernel(rua_layout L, const typename E::raw* vin,
                                                                  const typename E::raw* sin, void* out, int out_acc,
                                                                  typename E::acc* lse, int64_t H, int64_t D, int64_t G,
                                                                  int n_chunks) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = PL_LPR * VE;
  constexpr int UNR = PL_ROWS_UNR;
  constexpr int NS = LANE ? 1 : VE;                        // (m, l) states a thread keeps
  constexpr int STR = 2 * NS + VE;
  __shared__ A xch[RUA_WAVES_PER_BLOCK * PL_LPR * STR];    // [wave][l][m.. l.. acc..]
  struct alignas(16) Vec { raw e[VE]; };

  const int tid = threadIdx.x;
  const int l = tid & (PL_LPR - 1), q = tid >> 3, w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  const int64_t b = blockIdx.x / (unsigned)n_chunks;
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;

  int64_t gc[NS];
  bool first[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    gc[i] = i < nval ? (col0 + i) / D : 0;
    first[i] = i == 0 || gc[i] != gc[i > 0 ? i - 1 : 0];
  }

  auto ld = [&](int64_t row, Vec& v) {
    const raw* p = vin + row * H + col0;
    if constexpr (AL) {
      *(uint4*)&v = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = e < nval ? p[e] : E::down((A)0);
    }
  };

  A M[NS], S[NS], ACC[VE];
#pragma unroll
  for (int i = 0; i < NS; ++i) { M[i] = -seg_inf<A>(); S[i] = (A)0; }
#pragma unroll
  for (int e = 0; e < VE; ++e) ACC[e] = (A)0;

  for (int64_t t0 = 0; t0 < len; t0 += PL_BLOCK_TOK) {
    A m[NS], s[NS], acc[VE];
#pragma unroll
    for (int i = 0; i < NS; ++i) { m[i] = -seg_inf<A>(); s[i] = (A)0; }
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[e] = (A)0;
    const int64_t t1 = len < t0 + PL_BLOCK_TOK ? len : t0 + PL_BLOCK_TOK;
    if (active) {
      for (int64_t tt = t0 + q; tt < t1; tt += (int64_t)PL_SLOTS * UNR) {
        Vec vx[UNR];
        A sx[UNR][NS];
        bool ok[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int64_t t = tt + (int64_t)u * PL_SLOTS;
          ok[u] = false;
          if (t < t1) {
            const int64_t row = token_to_row(L, b, t, len);
            if (row >= 0 && row < L.n_rows) {
              ok[u] = true;
              ld(row, vx[u]);
#pragma unroll
              for (int i = 0; i < NS; ++i)
                if (i < nval && first[i]) sx[u][i] = E::up(sin[row * G + gc[i]]);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (!ok[u]) continue;
          A scale = (A)1, p = (A)0;
#pragma unroll
          for (int e = 0; e < VE; ++e) {
            if constexpr (LANE) {
              if (e == 0) pl_fold(m[0], s[0], sx[u][0], scale, p);
            } else {
              if (e >= nval) continue;
              if (first[e]) {
                pl_fold(m[e], s[e], sx[u][e], scale, p);
              } else {
                m[e] = m[e > 0 ? e - 1 : 0];
                s[e] = s[e > 0 ? e - 1 : 0];
              }
            }
            acc[e] = acc[e] * scale + p * E::up(vx[u].e[e]);
          }
        }
      }
    }
    // join two states: `get` hands the partner's (m, l) of state i and acc of element e
    auto join = [&](A* dm, A* ds, A* da, auto get_m, auto get_s, auto get_a) {
      A Mx = (A)0, fa = (A)1, fb = (A)1;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if constexpr (LANE) {
          if (e == 0) {
            pl_factors(dm[0], get_m(0), Mx, fa, fb);
            ds[0] = ds[0] * fa + get_s(0) * fb;
            dm[0] = Mx;
          }
        } else {
          if (e >= nval) continue;
          if (first[e]) {
            pl_factors(dm[e], get_m(e), Mx, fa, fb);
            ds[e] = ds[e] * fa + get_s(e) * fb;
            dm[e] = Mx;
          } else {
            dm[e] = dm[e > 0 ? e - 1 : 0];
            ds[e] = ds[e > 0 ? e - 1 : 0];
          }
        }
        da[e] = da[e] * fa + get_a(e) * fb;
      }
    };
    // slots 0 .. 7 of a wave: xor 8, 16, 32 of the lane number = xor 1, 2, 4 of the slot number
#pragma unroll
    for (int k = PL_LPR; k < RUA_WAVE; k <<= 1) {
      A m2[NS], s2[NS], a2[VE];
#pragma unroll
      for (int i = 0; i < NS; ++i) { m2[i] = seg_shfl_xor(m[i], k); s2[i] = seg_shfl_xor(s[i], k); }
#pragma unroll
      for (int e = 0; e < VE; ++e) a2[e] = seg_shfl_xor(acc[e], k);
      join(m, s, acc, [&](int i) { return m2[i]; }, [&](int i) { return s2[i]; }, [&](int e) { return a2[e]; });
    }
    // xor 8, 16 of the slot number = xor 1, 2 of the wave number, through LDS
    __syncthreads();
    if ((tid & (RUA_WAVE - 1)) < PL_LPR) {
      A* x = xch + (w * PL_LPR + l) * STR;
#pragma unroll
      for (int i = 0; i < NS; ++i) { x[i] = m[i]; x[NS + i] = s[i]; }
#pragma unroll
      for (int e = 0; e < VE; ++e) x[2 * NS + e] = acc[e];
    }
    __syncthreads();
    {
      A vm[RUA_WAVES_PER_BLOCK][NS], vs[RUA_WAVES_PER_BLOCK][NS], va[RUA_WAVES_PER_BLOCK][VE];
#pragma unroll
      for (int k = 0; k < RUA_WAVES_PER_BLOCK; ++k) {
        const A* x = xch + ((w ^ k) * PL_LPR + l) * STR;
#pragma unroll
        for (int i = 0; i < NS; ++i) { vm[k][i] = x[i]; vs[k][i] = x[NS + i]; }
#pragma unroll
        for (int e = 0; e < VE; ++e) va[k][e] = x[2 * NS + e];
      }
      join(vm[0], vs[0], va[0], [&](int i) { return vm[1][i]; }, [&](int i) { return vs[1][i]; },
           [&](int e) { return va[1][e]; });
      join(vm[2], vs[2], va[2], [&](int i) { return vm[3][i]; }, [&](int i) { return vs[3][i]; },
           [&](int e) { return va[3][e]; });
      join(vm[0], vs[0], va[0], [&](int i) { return vm[2][i]; }, [&](int i) { return vs[2][i]; },
           [&](int e) { return va[2][e]; });
      join(M, S, ACC, [&](int i) { return vm[0][i]; }, [&](int i) { return vs[0][i]; }, [&](int e) { return va[0][e]; });
    }
  }
  if (!active || q != 0) return;
  A oa[VE];
  Vec o;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    oa[e] = len > 0 ? ACC[e] / S[LANE ? 0 : e] : (A)0;
    o.e[e] = E::down(oa[e]);
  }
  if (out_acc) {                                             // RUA_POOL_OUT_ACC: unrounded, for the backward's delta
    A* pa = (A*)out + b * H + col0;
#pragma unroll
    for (int e = 0; e < VE; ++e) if (e < nval) pa[e] = oa[e];
  } else {
    raw* po = (raw*)out + b * H + col0;
    if constexpr (AL) {
      *(uint4*)po = *(const uint4*)&o;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (e < nval) po[e] = o.e[e];
    }
  }
  if (lse) {
#pragma unroll
    for (int i = 0; i < NS; ++i)
      if (i < nval && (col0 + i) % D == 0) lse[b * G + gc[i]] = M[i] + seg_log(S[i]);
  }
}

// ---------------------------------------------------------------- backward, lanes along time: rows of one vector
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_pool_backward_lanes_kernel(
    rua_layout L, const char* vin, const typename E::raw* sin, const void* outp, int out_acc, const typename E::raw* go,
    const typename E::acc* lse, char* gv, typename E::raw* gs, int H, int D, int G, int W) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (PL_SLOTS - 1);
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  if (b >= L.B) return;                                      // (no shuffles below)
  const int64_t len = safe_len(L, b);
  const int nb = H * (int)sizeof(raw);
  struct alignas(16) Row { raw e[VE]; };

  int gc[VE];
  bool first[VE], last[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) gc[e] = e < H ? e / D : -1;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    first[e] = e == 0 || gc[e] != gc[e > 0 ? e - 1 : 0];
    last[e] = e == VE - 1 || gc[e] != gc[e < VE - 1 ? e + 1 : e];
  }
  A g[VE], dl[VE], ls[VE];
  {
    A cur = (A)0;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      g[e] = (A)0; dl[e] = (A)0; ls[e] = (A)0;
      if (e >= H) continue;
      g[e] = E::up(go[b * H + e]);
      const A ov = out_acc ? ((const A*)outp)[b * H + e] : E::up(((const raw*)outp)[b * H + e]);
      const A pr = ov * g[e];
      cur = first[e] ? pr : cur + pr;
      dl[e] = cur;                                           // complete where last[e]
      ls[e] = lse[b * G + gc[e]];
    }
  }
  for (int64_t t = q; t < len; t += PL_SLOTS) {
    const int64_t row = token_to_row(L, b, t, len);
    if (row < 0 || row >= L.n_rows) continue;
    Row v, o;
    ld_row_w(vin + row * nb, nb, W, &v);
    A p = (A)0, cur = (A)0;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      o.e[e] = E::down((A)0);
      if (e >= H) continue;
      if (first[e]) p = seg_exp(E::up(sin[row * G + gc[e]]) - ls[e]);
      const A pr = E::up(v.e[e]) * g[e];
      cur = first[e] ? pr : cur + pr;
      o.e[e] = E::down(p * g[e]);
      if (gs && last[e]) gs[row * G + gc[e]] = E::down(p * (cur - dl[e]));
    }
    if (gv) st_row_w(gv + row * nb, nb, W, &o);
  }
  if (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) {
    Row z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = E::down((A)0);
    for (int64_t j = q; j < L.T_phys; j += PL_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row >= L.n_rows) continue;
      if (gv) st_row_w(gv + row * nb, nb, W, &z);
      if (gs) for (int e = 0; e < G; ++e) gs[row * G + e] = E::down((A)0);
    }
  }
}

// ---------------------------------------------------------------- backward, rows wider than one vector
// A workgroup takes a sequence, a wave every fourth token.  The lanes of a wave form 64 / S teams of S lanes; a team
// takes one score column per pass, its slots the column's units round-robin (UE elements each: a 16-byte vector when D
// is a multiple of one, else a single element).  AL: vector accesses for the units (UE == VE only).
template <typename E, bool AL, int UE>
__global__ __launch_bounds__(RUA_BLOCK) void seg_pool_backward_kernel(
    rua_layout L, const typename E::raw* vin, const typename E::raw* sin, const void* outp, int out_acc,
    const typename E::raw* go, const typename E::acc* lse, typename E::raw* gv, typename E::raw* gs, int64_t H, int64_t D,
    int64_t G, int S) {
  using raw = typename E::raw;
  using A = typename E::acc;
  struct alignas(AL ? 16 : sizeof(raw)) Unit { raw e[UE]; };
  const int tid = threadIdx.x;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int slot = lane & (S - 1), team = lane / S, tpw = RUA_WAVE / S;
  const int64_t b = blockIdx.x;
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  const int64_t DU = D / UE;
  const bool cached = DU <= 2 * (int64_t)S;                  // the cotangent's units stay in registers

  auto ldu = [&](const raw* p, Unit& u) {
    if constexpr (AL) {
      *(uint4*)&u = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < UE; ++e) u.e[e] = p[e];
    }
  };
  auto stu = [&](raw* p, const Unit& u) {
    if constexpr (AL) {
      *(uint4*)p = *(const uint4*)&u;
    } else {
#pragma unroll
      for (int e = 0; e < UE; ++e) p[e] = u.e[e];
    }
  };
  Unit zero;
#pragma unroll
  for (int e = 0; e < UE; ++e) zero.e[e] = E::down((A)0);

  for (int64_t g0 = 0; g0 < G; g0 += tpw) {                  // wave-uniform
    const int64_t g = g0 + team;
    const bool valid = g < G;
    const raw* gob = go + b * H + g * D;
    const raw* oub = (const raw*)outp + b * H + g * D;
    const A* oua = (const A*)outp + b * H + g * D;             // RUA_POOL_OUT_ACC: `out` in the accumulator type
    Unit gc0 = zero, gc1 = zero;
    A delta = (A)0;
    if (valid) {
      int i = 0;
      for (int64_t k = slot; k < DU; k += S, ++i) {
        Unit gg, oo = zero;
        ldu(gob + k * UE, gg);
        if (!out_acc) ldu(oub + k * UE, oo);
        if (i == 0) gc0 = gg; else if (i == 1) gc1 = gg;
#pragma unroll
        for (int e = 0; e < UE; ++e)
          delta = delta + (out_acc ? oua[k * UE + e] : E::up(oo.e[e])) * E::up(gg.e[e]);
      }
    }
    for (int k = 1; k < S; k <<= 1) delta = delta + seg_shfl_xor(delta, k);
    const A ls = valid ? lse[b * G + g] : (A)0;

    for (int64_t t = w; t < len; t += RUA_WAVES_PER_BLOCK) { // wave-uniform
      const int64_t row = token_to_row(L, b, t, len);
      if (row < 0 || row >= L.n_rows) continue;               // wave-uniform
      A p = (A)0, dot = (A)0;
      if (valid) {
        p = seg_exp(E::up(sin[row * G + g]) - ls);
        const raw* vb = vin + row * H + g * D;
        raw* gvb = gv ? gv + row * H + g * D : nullptr;
        int i = 0;
        for (int64_t k = slot; k < DU; k += S, ++i) {
          Unit vv, gg, oo;
          ldu(vb + k * UE, vv);
          if (cached) gg = i == 0 ? gc0 : gc1; else ldu(gob + k * UE, gg);
#pragma unroll
          for (int e = 0; e < UE; ++e) {
            const A ge = E::up(gg.e[e]);
            dot = dot + E::up(vv.e[e]) * ge;
            oo.e[e] = E::down(p * ge);
          }
          if (gvb) stu(gvb + k * UE, oo);
        }
      }
      for (int k = 1; k < S; k <<= 1) dot = dot + seg_shfl_xor(dot, k);
      if (valid && slot == 0 && gs) gs[row * G + g] = E::down(p * (dot - delta));
    }
  }
  if (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) {
    const int64_t HU = H / UE;
    for (int64_t j = w; j < L.T_phys; j += RUA_WAVES_PER_BLOCK) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row >= L.n_rows) continue;
      if (gv) for (int64_t k = lane; k < HU; k += RUA_WAVE) stu(gv + row * H + k * UE, zero);
      if (gs) for (int64_t k = lane; k < G; k += RUA_WAVE) gs[row * G + k] = E::down((A)0);
    }
  }
}

// ---------------------------------------------------------------- host side
template <typename E>
static int pl_forward(const rua_layout& L, const void* v, const void* sc, void* out, int oacc, void* lse, int64_t H,
                      int64_t D, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  const int64_t G = H / D;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t bases = (uint64_t)(uintptr_t)v | (uint64_t)(uintptr_t)out;
  if (((uint64_t)(uintptr_t)v | (uint64_t)(uintptr_t)sc) % sizeof(raw) || (uint64_t)(uintptr_t)lse % sizeof(A) ||
      (uint64_t)(uintptr_t)out % (oacc ? sizeof(A) : sizeof(raw)))
    return RUA_EALIGN;

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, (uint64_t)(uintptr_t)v, L.B);
    const int W = ln.W;
    const int64_t grid = ln.grid;
    if (!grid) return RUA_ERANGE;
    seg_trace("seg_pool_lanes_kernel T=%s AL=%d W=%d H=%d D=%d kind=%d", E::name(), (int)(W == 16), W, (int)H, (int)D,
              L.kind);
    hipLaunchKernelGGL((seg_pool_lanes_kernel<E>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L, (const char*)v,
                       (const raw*)sc, out, oacc, (A*)lse, (int)H, (int)D, (int)G, W);
    return (int)hipGetLastError();
  }

  const int n_chunks = (int)((row_bytes + 127) / 128);
  const bool al = row_bytes % 16 == 0 && bases % 16 == 0;
  const bool lane = D % VE == 0;
  const int64_t grid = L.B * (int64_t)n_chunks;
  if (row_bytes + 127 > 0x7fffffffLL * 128 || grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_pool_rows_kernel T=%s AL=%d lane=%d D=%lld kind=%d chunks=%d", E::name(), (int)al, (int)lane,
            (long long)D, L.kind, n_chunks);
#define RUA_PL_ROWS(ALV, LANEV)                                                                                        \
  hipLaunchKernelGGL((seg_pool_rows_kernel<E, ALV, LANEV>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L,            \
                     (const raw*)v, (const raw*)sc, out, oacc, (A*)lse, H, D, G, n_chunks)
  if (al) { if (lane) RUA_PL_ROWS(true, true); else RUA_PL_ROWS(true, false); }
  else    { if (lane) RUA_PL_ROWS(false, true); else RUA_PL_ROWS(false, false); }
#undef RUA_PL_ROWS
  return (int)hipGetLastError();
}

template <typename E>
static int pl_backward(const rua_layout& L, const void* go, const void* v, const void* sc, const void* out, int oacc,
                       const void* lse, void* gv, void* gs, int64_t H, int64_t D, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  const int64_t G = H / D;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t wide = (uint64_t)(uintptr_t)v | (uint64_t)(uintptr_t)gv;            // [N, H] operands
  const uint64_t all = wide | (uint64_t)(uintptr_t)go | (uint64_t)(uintptr_t)sc | (uint64_t)(uintptr_t)gs;
  if (all % sizeof(raw) || (uint64_t)(uintptr_t)lse % sizeof(A) ||
      (uint64_t)(uintptr_t)out % (oacc ? sizeof(A) : sizeof(raw)))
    return RUA_EALIGN;

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, wide, L.B);
    const int W = ln.W;
    const int64_t grid = ln.grid;
    if (!grid) return RUA_ERANGE;
    seg_trace("seg_pool_backward_kernel T=%s AL=%d form=lanes W=%d H=%d D=%d kind=%d", E::name(), (int)(W == 16), W,
              (int)H, (int)D, L.kind);
    hipLaunchKernelGGL((seg_pool_backward_lanes_kernel<E>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L,
                       (const char*)v, (const raw*)sc, out, oacc, (const raw*)go, (const A*)lse, (char*)gv,
                       (raw*)gs, (int)H, (int)D, (int)G, W);
    return (int)hipGetLastError();
  }

  if (L.B > 0x7fffffffLL) return RUA_ERANGE;
  const bool vec = D % VE == 0;
  const bool al = vec && (wide | (uint64_t)(uintptr_t)go | (oacc ? 0 : (uint64_t)(uintptr_t)out)) % 16 == 0;
  const int64_t DU = vec ? D / VE : D;
  int S = 1;
  while (S < RUA_WAVE && S < DU) S <<= 1;
  seg_trace("seg_pool_backward_kernel T=%s AL=%d form=team UE=%d S=%d D=%lld kind=%d", E::name(), (int)al, vec ? VE : 1,
            S, (long long)D, L.kind);
#define RUA_PL_BWD(ALV, UEV)                                                                                           \
  hipLaunchKernelGGL((seg_pool_backward_kernel<E, ALV, UEV>), dim3((unsigned)L.B), dim3(RUA_BLOCK), 0, s, L,           \
                     (const raw*)v, (const raw*)sc, out, oacc, (const raw*)go, (const A*)lse, (raw*)gv, (raw*)gs,       \
                     H, D, G, S)
  if (!vec) RUA_PL_BWD(false, 1);
  else if (al) RUA_PL_BWD(true, VE);
  else RUA_PL_BWD(false, VE);
#undef RUA_PL_BWD
  return (int)hipGetLastError();
}

// the checks both directions share; > 0: nothing to do
static int pl_check(const rua_layout* lay, int64_t H, int64_t D, int32_t& dtype, int& oacc) {
  oacc = (dtype & RUA_POOL_OUT_ACC) ? 1 : 0;
  if (dtype >= 0) dtype &= ~RUA_POOL_OUT_ACC;
  const int e = seg_check_entry(lay, H, seg_esize(dtype, false));
  if (e != 0) return e;
  return D <= 0 || H % D ? RUA_EINVAL : 0;
}

}  // namespace rua

extern "C" int64_t rua_softmax_pool_ws_bytes(const rua_layout* lay, int64_t H, int64_t D, int32_t dtype) {
  (void)lay; (void)H; (void)D; (void)dtype;
  return 0;                                                  // no form cuts a sequence across workgroups yet
}

extern "C" int rua_segment_softmax_pool(const rua_layout* lay, const void* values, const void* scores, void* out,
                                        void* lse, int64_t H, int64_t D, int32_t dtype, void* ws, void* stream) {
  using namespace rua;
  (void)ws;
  int e, oacc;
  if ((e = pl_check(lay, H, D, dtype, oacc)) != 0) return e;
  if (out && (out == values || out == scores || out == lse)) return RUA_EINVAL;
  if (lse && (lse == values || lse == scores)) return RUA_EINVAL;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!values || !scores || !out) return RUA_EINVAL;
  if (seg_too_large(lay, H, seg_esize(dtype, false))) return RUA_ERANGE;
#define RUA_PL(E) pl_forward<E>(*lay, values, scores, out, oacc, lse, H, D, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_PL);
#undef RUA_PL
}

extern "C" int rua_segment_softmax_pool_backward(const rua_layout* lay, const void* grad_out, const void* values,
                                                 const void* scores, const void* out, const void* lse,
                                                 void* grad_values, void* grad_scores, int64_t H, int64_t D,
                                                 int32_t dtype, void* ws, void* stream) {
  using namespace rua;
  (void)ws;
  int e, oacc;
  if ((e = pl_check(lay, H, D, dtype, oacc)) != 0) return e;
  const void* ins[5] = {grad_out, values, scores, out, lse};
  for (const void* p : ins)
    if (p && (p == grad_values || p == grad_scores)) return RUA_EINVAL;
  if (grad_values && grad_values == grad_scores) return RUA_EINVAL;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!grad_values && !grad_scores) return 0;
  if (!grad_out || !values || !scores || !out || !lse) return RUA_EINVAL;
  if (seg_too_large(lay, H, seg_esize(dtype, false))) return RUA_ERANGE;
#define RUA_PL(E)                                                                                                      \
  pl_backward<E>(*lay, grad_out, values, scores, out, oacc, lse, grad_values, grad_scores, H, D, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_PL);
#undef RUA_PL
}
