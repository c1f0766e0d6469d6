// rua_ctc.hip — per-sequence CTC over the frames of a C / L / P / R container of log-probabilities [rows, V] and the
// labels of a SECOND ragged container (rua_segment_ctc_forward, rua_segment_ctc_backtrace, rua_segment_ctc_backward;
// include/rua.h).  An extension: the loss the ragged speech pipeline ends in, its true gradient and the
// forced alignment.  The first kernels that read two containers of different raggedness: both layouts travel by value,
// sequence b is the same sequence in both (token_to_row resolves a P through `unsorted`).
//
// The extended target of sequence b is l' = (blank, y_0, blank, ..., y_{S-1}, blank), S' = 2 S + 1 states.
//
// Geometry.  A TEAM walks one sequence, frame by frame, and the teams of the launch stride over b:
//   lanes form      a team is one wave (4 per workgroup); thread i keeps the R consecutive states i R .. i R + R - 1
//                   and their labels in registers, R = 1 / 2 / 4 / 8 for S'_max <= 64 / 128 / 256 / 512; the two boundary
//                   values alpha[i R - 1], alpha[i R - 2] come from lane i - 1 by a cross-lane move (no LDS in the forward);
//   workgroup form  a team is one workgroup of 256 threads with R = 8 (512 < S'_max <= 2047); the boundary values go
//                   through LDS, one barrier per frame (two buffers, by the parity of t).
// The per-state arithmetic is ONE function (ctc_lse3 / ctc_best3) for both forms and every R: the same bits.
//
// ONE evaluation order per (sequence, frame, state) (fp32; fp64 for RUA_F64; no contraction):
//   v0 = alpha[s], v1 = alpha[s-1] (s >= 1), v2 = alpha[s-2] (s >= 2, l'_s != blank, l'_s != l'_{s-2}); a term that does
//   not exist is absent.  LOG: m = max (a NaN stays); m == -inf: -inf; else lp_t[l'_s] + (m + log(exp(v0-m) + exp(v1-m)
//   [+ exp(v2-m)])).  MAX: the maximum in ascending predecessor state (s-2, s-1, s) under argmax's order (a NaN beats
//   every number, the first of equals wins), its offset 0 / 1 / 2 is the code of (row, state); -inf stays -inf.
//   alpha_0[0] = lp_0[blank], alpha_0[1] = lp_0[y_0], -inf elsewhere.  The end folds alpha[S'-1], then alpha[S'-2].
// The lp values of frame t + 1 (blank once per thread, the labels gathered) are requested before the arithmetic of frame t.
//
// The backward walks from the end with beta (WITHOUT the emission at t) in registers:
//   u_s = lp_{t+1}[l'_s] + beta_{t+1}[s];   beta_t[s] = ctc_lse3(u_s, u_{s+1}, u_{s+2}) with the same existence rules,
//   post_t[s] = exp((alpha_t[s] + beta_t[s]) - logZ), staged in LDS, and
//   grad[t, c] = -g[b] * sum_{s : l'_s = c} post_t[s], rounded once.
// NO FLOAT ATOMICS.  The order of the class sum is fixed per (sequence, frame, class), whatever the layout, the form or R:
//   c != blank: the states of c in ascending s, added sequentially from 0 (the labels are rank-sorted by (label, index)
//               once per sequence into LDS; the distinct labels get a compacted table);
//   c == blank: lane i of 64 adds, sequentially from 0 and in ascending k = i, i + 64, ..., post[2 k] and then post[2 k + 1]
//               when y_k == blank; the 64 parts are folded by the butterfly xor 32, 16, 8, 4, 2, 1.
// A sweep over the V classes in chunks of 64 then writes the whole row once, zeros included: the wave keeps a pointer
// into the sorted distinct labels, the lanes whose label falls in the chunk scatter their sums through a 64-entry LDS
// row, and lane c mod 64 stores class c (coalesced).
//
// KNOWN LIMITS: one long target sends the whole batch to the workgroup form; one wave / workgroup walks all the frames
// of a sequence; the table alpha costs rows x (2 S_max + 1) accumulators.
#include <stdio.h>
#include <stdint.h>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int64_t CTC_MAX_GRID = 1024;
constexpr int CTC_LANES_MAX_SP = 512;                                  // S' of the lanes form, at most
static_assert(2 * RUA_CTC_MAX_TARGET + 1 <= RUA_BLOCK * 8, "the workgroup form holds 8 states per thread");

template <typename A> __device__ __forceinline__ A ctc_max(A m, A v) { return (v > m || v != v) ? v : m; }
template <typename A> __device__ __forceinline__ bool ctc_beats(A v, A m) { return v > m || (v != v && m == m); }

// the order of LDS accesses of ONE wave, for the compiler (the hardware keeps a wave's LDS accesses in order)
__device__ __forceinline__ void ctc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool WG> __device__ __forceinline__ void ctc_team_sync() {
  if constexpr (WG) __syncthreads(); else ctc_wave_sync();
}
template <bool WG> __device__ __forceinline__ bool ctc_team_any(bool p) {
  if constexpr (WG) return __syncthreads_or(p ? 1 : 0) != 0; else return __any(p ? 1 : 0) != 0;
}

// THE logsumexp of up to three terms, in this order; a term that does not exist (h1 / h2 false) is absent
template <typename A> __device__ __forceinline__ A ctc_lse3(A v0, A v1, bool h1, A v2, bool h2) {
  const A ninf = -seg_inf<A>();
  A m = v0;
  if (h1) m = ctc_max(m, v1);
  if (h2) m = ctc_max(m, v2);
  if (m == ninf) return ninf;
  A s = seg_exp(v0 - m);
  if (h1) s = s + seg_exp(v1 - m);
  if (h2) s = s + seg_exp(v2 - m);
  return m + seg_log(s);
}

// THE maximum of up to three terms in ascending predecessor state (v2: s-2, v1: s-1, v0: s); `code` = s - predecessor
template <typename A> __device__ __forceinline__ A ctc_best3(A v0, A v1, bool h1, A v2, bool h2, int& code) {
  A best = v0;
  code = 0;
  if (h2) {
    best = v2; code = 2;
    if (ctc_beats(v1, best)) { best = v1; code = 1; }
    if (ctc_beats(v0, best)) { best = v0; code = 0; }
  } else if (h1) {
    best = v1; code = 1;
    if (ctc_beats(v0, best)) { best = v0; code = 0; }
  }
  return best;
}

// label k of sequence b of the targets' container, range-checked where its row is formed; -1: there is none
__device__ __forceinline__ int64_t ctc_label(const rua_layout& LT, const int64_t* __restrict__ y, int64_t b, int64_t k,
                                             int64_t S) {
  const int64_t r = token_to_row(LT, b, k, S);
  return (r >= 0 && r < LT.n_rows) ? y[r] : (int64_t)-1;
}

// the number of labels of sequence b, never more than the launch was sized for
__device__ __forceinline__ int ctc_target_len(const rua_layout& LT, int64_t b, int S_max) {
  const int64_t S = safe_len(LT, b);
  return (int)(S < S_max ? S : S_max);
}

template <int R, bool WG> struct ctc_geo {
  static constexpr int THREADS = WG ? RUA_BLOCK : RUA_WAVE;
  static constexpr int TEAMS = WG ? 1 : RUA_WAVES_PER_BLOCK;            // per workgroup
};

// what thread `tid` of a team needs from its neighbour below: p1 = the state tid R - 1, p2 = the state tid R - 2
template <typename A, int R, bool WG>
__device__ __forceinline__ void ctc_from_below(const A (&a)[R], int tid, A* xch, A& p1, A& p2) {
  if constexpr (WG) {
    xch[2 * tid] = a[R - 1];
    xch[2 * tid + 1] = a[R - 2];
    __syncthreads();
    const int q = tid > 0 ? tid - 1 : 0;
    p1 = xch[2 * q];
    p2 = xch[2 * q + 1];
  } else {
    p1 = __shfl_up(a[R - 1], 1, RUA_WAVE);
    if constexpr (R >= 2) p2 = __shfl_up(a[R - 2], 1, RUA_WAVE); else p2 = __shfl_up(a[0], 2, RUA_WAVE);
  }
}
// ... and from its neighbour above: n1 = the state tid R + R, n2 = the state tid R + R + 1
template <typename A, int R, bool WG>
__device__ __forceinline__ void ctc_from_above(const A (&u)[R], int tid, A* xch, A& n1, A& n2) {
  if constexpr (WG) {
    xch[2 * tid] = u[0];
    xch[2 * tid + 1] = u[1];
    __syncthreads();
    const int q = tid < RUA_BLOCK - 1 ? tid + 1 : tid;
    n1 = xch[2 * q];
    n2 = xch[2 * q + 1];
  } else {
    n1 = __shfl_down(u[0], 1, RUA_WAVE);
    if constexpr (R >= 2) n2 = __shfl_down(u[1], 1, RUA_WAVE); else n2 = __shfl_down(u[0], 2, RUA_WAVE);
  }
}

// ---------------------------------------------------------------- forward: LOG (the loss) and MAX (the alignment)
template <typename E, int R, bool WG, bool VIT>
__global__ __launch_bounds__(RUA_BLOCK) void seg_ctc_forward_kernel(rua_layout LF, rua_layout LT,
                                                                    const typename E::raw* __restrict__ lp,
                                                                    const int64_t* __restrict__ y,
                                                                    typename E::acc* __restrict__ alpha,
                                                                    uint8_t* __restrict__ codes,
                                                                    typename E::acc* __restrict__ out,
                                                                    typename E::acc* __restrict__ logz,
                                                                    int64_t* __restrict__ last, int V, int S_max, int blank,
                                                                    int zero_inf) {
  using A = typename E::acc;
  using G = ctc_geo<R, WG>;
  __shared__ A xch_lds[WG ? 4 * RUA_BLOCK : 1];
  const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & (RUA_WAVE - 1));
  const int64_t team = WG ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * G::TEAMS + (threadIdx.x >> 6);
  const int64_t teams = (int64_t)gridDim.x * G::TEAMS;
  const A ninf = -seg_inf<A>();
  const int64_t SP = 2 * (int64_t)S_max + 1;
  const int s0 = tid * R;

  for (int64_t b = team; b < LF.B; b += teams) {
    const int64_t T = safe_len(LF, b);
    const int S = ctc_target_len(LT, b, S_max);
    const int SS = 2 * S + 1;

    int lab[R];
    bool h2[R];
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int s = s0 + r;
      lab[r] = blank;
      h2[r] = false;
      if ((s & 1) && s < SS) {
        const int k = s >> 1;
        int64_t yk = ctc_label(LT, y, b, k, S);
        if (yk < 0 || yk >= V) { bad = true; yk = blank; }
        lab[r] = (int)yk;
        if (k > 0) h2[r] = yk != blank && yk != ctc_label(LT, y, b, k - 1, S);
      }
    }
    bad = ctc_team_any<WG>(bad);
    if (bad || T <= 0) {
      // a label outside [0, V): NaN, never dereferenced.  No frame: 0 for an empty target, else no alignment
      if (tid == 0) {
        const A z = bad ? seg_nan<A>() : (S == 0 ? (A)0 : ninf);
        if (VIT) {
          out[b] = z;
          last[b] = -1;
        } else {
          const A loss = -z;
          out[b] = (zero_inf && loss == seg_inf<A>()) ? (A)0 : loss;
          if (logz) logz[b] = z;
        }
      }
      continue;
    }
    auto row_of = [&](int64_t t) {
      const int64_t r = token_to_row(LF, b, t, T);
      return (r >= 0 && r < LF.n_rows) ? r : (int64_t)-1;
    };
    auto fetch = [&](int64_t row, A (&x)[R]) {
      const typename E::raw* p = lp + (row >= 0 ? row : 0) * (int64_t)V;
      const A xb = row >= 0 ? E::up(p[blank]) : (A)0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool odd = R > 1 ? (r & 1) != 0 : (tid & 1) != 0;
        x[r] = (odd && row >= 0 && s0 + r < SS) ? E::up(p[lab[r]]) : xb;
      }
    };

    A a[R], x[R], xn[R];
    int64_t row = row_of(0);
    fetch(row, x);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int s = s0 + r;
      a[r] = (s < 2 && s < SS) ? x[r] : ninf;
      if (!VIT && alpha && s < SS && row >= 0) alpha[row * SP + s] = a[r];
    }
    int64_t row_n = T > 1 ? row_of(1) : -1;
    fetch(row_n, xn);

    for (int64_t t = 1; t < T; ++t) {
      row = row_n;
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = xn[r];
      row_n = t + 1 < T ? row_of(t + 1) : -1;                    // the next frame is in flight during this one
      fetch(row_n, xn);
      A p1, p2;
      ctc_from_below<A, R, WG>(a, tid, xch_lds + (t & 1) * 2 * RUA_BLOCK, p1, p2);
      A na[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int s = s0 + r;
        const A v1 = r >= 1 ? a[r >= 1 ? r - 1 : 0] : p1;
        const A v2 = r >= 2 ? a[r >= 2 ? r - 2 : 0] : (r == 1 ? p1 : p2);
        const bool e1 = s >= 1, e2 = s >= 2 && h2[r];
        A f;
        if constexpr (VIT) {
          int code;
          f = ctc_best3(a[r], v1, e1, v2, e2, code);
          if (s < SS && row >= 0) codes[row * SP + s] = (uint8_t)code;
        } else {
          f = ctc_lse3(a[r], v1, e1, v2, e2);
        }
        na[r] = (s < SS && f != ninf) ? x[r] + f : ninf;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        a[r] = na[r];
        if (!VIT && alpha && s0 + r < SS && row >= 0) alpha[row * SP + s0 + r] = a[r];
      }
    }

    // the end: the thread that holds the state S' - 1 folds it with S' - 2
    A p1, p2;
    ctc_from_below<A, R, WG>(a, tid, xch_lds + (T & 1) * 2 * RUA_BLOCK, p1, p2);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (s0 + r != SS - 1) continue;
      const A va = a[r], vb = r >= 1 ? a[r >= 1 ? r - 1 : 0] : p1;
      const bool hb = SS >= 2;
      if constexpr (VIT) {
        A best = va;
        int64_t arg = SS - 1;
        if (hb) {
          best = vb; arg = SS - 2;
          if (ctc_beats(va, best)) { best = va; arg = SS - 1; }
        }
        out[b] = best;
        last[b] = best == ninf ? (int64_t)-1 : arg;
      } else {
        const A z = ctc_lse3(va, vb, hb, (A)0, false);
        const A loss = -z;
        out[b] = (zero_inf && loss == seg_inf<A>()) ? (A)0 : loss;
        if (logz) logz[b] = z;
      }
    }
    (void)p2;
  }
}

// ---------------------------------------------------------------- the alignment's backtrace: a thread per sequence
__global__ __launch_bounds__(RUA_BLOCK) void seg_ctc_backtrace_kernel(rua_layout LF, rua_layout LT,
                                                                      const int64_t* __restrict__ y,
                                                                      const uint8_t* __restrict__ codes,
                                                                      const int64_t* __restrict__ last,
                                                                      int64_t* __restrict__ labels,
                                                                      int64_t* __restrict__ positions, int S_max,
                                                                      int blank) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= LF.B) return;
  const int64_t T = safe_len(LF, b);
  const int S = ctc_target_len(LT, b, S_max);
  const int64_t SP = 2 * (int64_t)S_max + 1;
  int64_t s = last[b];
  if (s < 0 || s > 2 * (int64_t)S) s = -1;
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t row = token_to_row(LF, b, t, T);
    if (row < 0 || row >= LF.n_rows) continue;
    int64_t lab = blank, pos = -1;
    if (s >= 0 && (s & 1)) {
      pos = s >> 1;
      lab = ctc_label(LT, y, b, pos, S);
      if (lab < 0) lab = blank;
    }
    labels[row] = lab;
    positions[row] = pos;
    if (s >= 0 && t > 0) {
      int c = codes[row * SP + s];
      if (c > 2) c = 0;
      s -= c;
      if (s < 0) s = 0;
    }
  }
  seg_fill_padding(LF, b, T, 0, 1, [&](int64_t row) { labels[row] = 0; positions[row] = 0; });
}

// ---------------------------------------------------------------- backward of the loss
template <typename A, int NS, int NW> struct ctc_bwd_lds {
  A post[2 * NS + 2];          // the state posteriors of the frame
  A sum[NS];                   // the class sum of every distinct label
  A row[NW][RUA_WAVE];         // a wave's 64 classes of the sweep
  A gblank;
  int ylab[NS];                // the labels
  int ulab[NS];                // the distinct labels, ascending
  uint16_t order[NS];          // the label indices sorted by (label, index)
  uint16_t ustart[NS + 1];     // where the distinct label j starts in `order`
  int n_distinct;
};

template <typename E, int R, bool WG>
__global__ __launch_bounds__(RUA_BLOCK) void seg_ctc_backward_kernel(rua_layout LF, rua_layout LT,
                                                                     const typename E::acc* __restrict__ grad,
                                                                     const typename E::raw* __restrict__ lp,
                                                                     const int64_t* __restrict__ y,
                                                                     const typename E::acc* __restrict__ alpha,
                                                                     const typename E::acc* __restrict__ logz,
                                                                     typename E::raw* __restrict__ gx, int V, int S_max,
                                                                     int blank) {
  using A = typename E::acc;
  using raw = typename E::raw;
  using G = ctc_geo<R, WG>;
  constexpr int NS = WG ? RUA_CTC_MAX_TARGET + 1 : CTC_LANES_MAX_SP / 2;
  constexpr int NW = G::THREADS / RUA_WAVE;
  __shared__ ctc_bwd_lds<A, NS, NW> lds[G::TEAMS];
  __shared__ A xch_lds[WG ? 2 * RUA_BLOCK : 1];
  const int lane = (int)(threadIdx.x & (RUA_WAVE - 1));
  const int tid = WG ? (int)threadIdx.x : lane;
  const int wv = WG ? (int)(threadIdx.x >> 6) : 0;                      // the wave of the team
  ctc_bwd_lds<A, NS, NW>& sh = lds[WG ? 0 : (int)(threadIdx.x >> 6)];
  const int64_t team = WG ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * G::TEAMS + (threadIdx.x >> 6);
  const int64_t teams = (int64_t)gridDim.x * G::TEAMS;
  const A ninf = -seg_inf<A>();
  const int64_t SP = 2 * (int64_t)S_max + 1;
  const int s0 = tid * R;

  for (int64_t b = team; b < LF.B; b += teams) {
    const int64_t T = safe_len(LF, b);
    const int S = ctc_target_len(LT, b, S_max);
    const int SS = 2 * S + 1;
    if (LF.kind == RUA_LEFT || LF.kind == RUA_RIGHT) {
      // the padding rows of the gradient: zeros
      const int64_t n = LF.T_phys * (int64_t)V;
      for (int64_t idx = tid; idx < n; idx += G::THREADS) {
        const int64_t pos = div_rows(idx, V);
        const int64_t row = b * LF.T_phys + pos;
        if (is_pad(LF, pos, T) && row < LF.n_rows) gx[b * n + idx] = (raw)0;
      }
    }
    if (T <= 0) continue;
    auto row_of = [&](int64_t t) {
      const int64_t r = token_to_row(LF, b, t, T);
      return (r >= 0 && r < LF.n_rows) ? r : (int64_t)-1;
    };

    // the labels, once per sequence
    ctc_team_sync<WG>();                                        // (the previous sequence's readers are done)
    bool bad = false;
    for (int k = tid; k < S; k += G::THREADS) {
      int64_t yk = ctc_label(LT, y, b, k, S);
      if (yk < 0 || yk >= V) { bad = true; yk = blank; }
      sh.ylab[k] = (int)yk;
    }
    bad = ctc_team_any<WG>(bad);
    const A g = grad[b], lz = logz[b];
    if (bad || lz == ninf) {
      // no alignment, or a label outside [0, V): exact zeros (a documented choice)
      for (int64_t t = 0; t < T; ++t) {
        const int64_t r = row_of(t);
        if (r < 0) continue;
        for (int c = tid; c < V; c += G::THREADS) gx[r * V + c] = (raw)0;
      }
      continue;
    }
    ctc_team_sync<WG>();
    for (int k = tid; k < S; k += G::THREADS) {
      const int yk = sh.ylab[k];
      int rank = 0;
      for (int j = 0; j < S; ++j) {
        const int yj = sh.ylab[j];
        rank += (yj < yk || (yj == yk && j < k)) ? 1 : 0;
      }
      sh.order[rank] = (uint16_t)k;
    }
    ctc_team_sync<WG>();
    if (wv == 0) {
      int n = 0;
      for (int q0 = 0; q0 < S; q0 += RUA_WAVE) {
        const int q = q0 + lane;
        const bool head = q < S && (q == 0 || sh.ylab[sh.order[q]] != sh.ylab[sh.order[q > 0 ? q - 1 : 0]]);
        const unsigned long long mask = __ballot(head ? 1 : 0);
        if (head) {
          const int j = n + __popcll(mask & ((1ull << lane) - 1ull));
          sh.ulab[j] = sh.ylab[sh.order[q]];
          sh.ustart[j] = (uint16_t)q;
        }
        n += __popcll(mask);
      }
      if (lane == 0) {
        sh.ustart[n] = (uint16_t)S;
        sh.n_distinct = n;
      }
    }
    ctc_team_sync<WG>();
    const int U = sh.n_distinct;

    int lab[R];
    bool h2n[R];                                                // may the state s move on to s + 2?
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int s = s0 + r;
      lab[r] = blank;
      h2n[r] = false;
      if ((s & 1) && s < SS) {
        const int k = s >> 1;
        lab[r] = sh.ylab[k];
        if (k + 1 < S) h2n[r] = sh.ylab[k + 1] != blank && sh.ylab[k + 1] != lab[r];
      }
    }
    auto fetch = [&](int64_t row, A (&x)[R], A (&al)[R]) {
      const raw* p = lp + (row >= 0 ? row : 0) * (int64_t)V;
      const A xb = row >= 0 ? E::up(p[blank]) : (A)0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool odd = R > 1 ? (r & 1) != 0 : (tid & 1) != 0;
        const bool live = row >= 0 && s0 + r < SS;
        x[r] = (odd && live) ? E::up(p[lab[r]]) : xb;
        al[r] = live ? alpha[row * SP + s0 + r] : ninf;
      }
    };

    A beta[R], x[R], al[R], xn[R], aln[R];
#pragma unroll
    for (int r = 0; r < R; ++r) beta[r] = (s0 + r == SS - 1 || s0 + r == SS - 2) ? (A)0 : ninf;
    int64_t row = row_of(T - 1);
    fetch(row, x, al);
    int64_t row_n = T > 1 ? row_of(T - 2) : -1;
    fetch(row_n, xn, aln);

    for (int64_t t = T - 1; t >= 0; --t) {
      // the posteriors of frame t
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (s0 + r < SS) sh.post[s0 + r] = seg_exp((al[r] + beta[r]) - lz);
      }
      ctc_team_sync<WG>();
      // the class sums: a distinct label's states in ascending s; blank by 64 lanes and a butterfly
      for (int j = tid; j < U; j += G::THREADS) {
        A acc = (A)0;
        const int qe = sh.ustart[j + 1];
        for (int q = sh.ustart[j]; q < qe; ++q) acc = acc + sh.post[2 * (int)sh.order[q] + 1];
        sh.sum[j] = acc;
      }
      if (wv == 0) {
        A acc = (A)0;
        for (int k = lane; k <= S; k += RUA_WAVE) {
          acc = acc + sh.post[2 * k];
          if (k < S && sh.ylab[k] == blank) acc = acc + sh.post[2 * k + 1];
        }
#pragma unroll
        for (int m = RUA_WAVE / 2; m >= 1; m >>= 1) acc = acc + seg_shfl_xor(acc, m);
        if (lane == 0) sh.gblank = acc;
      }
      ctc_team_sync<WG>();
      // the sweep over the classes: every wave of the team takes every NW-th chunk of 64 and writes it once
      if (row >= 0) {
        const A gb = sh.gblank;
        int p = 0;
        for (int c0 = wv * RUA_WAVE; c0 < V; c0 += NW * RUA_WAVE) {
          int ul;
          for (;;) {                                            // the first distinct label >= c0
            ul = p + lane < U ? sh.ulab[p + lane] : 0x7fffffff;
            const int below = __popcll(__ballot(ul < c0 ? 1 : 0));
            p += below;
            if (below < RUA_WAVE) break;
          }
          ul = p + lane < U ? sh.ulab[p + lane] : 0x7fffffff;
          const bool hit = ul < c0 + RUA_WAVE;
          sh.row[wv][lane] = (A)0;
          ctc_wave_sync();
          if (hit) sh.row[wv][ul - c0] = sh.sum[p + lane];
          ctc_wave_sync();
          A v = sh.row[wv][lane];
          ctc_wave_sync();
          p += __popcll(__ballot(hit ? 1 : 0));
          const int c = c0 + lane;
          if (c == blank) v = gb;
          if (c < V) gx[row * V + c] = E::down(-g * v);
        }
      }
      if (t == 0) break;
      // beta of frame t - 1
      A u[R];
#pragma unroll
      for (int r = 0; r < R; ++r) u[r] = (s0 + r < SS && beta[r] != ninf) ? x[r] + beta[r] : ninf;
      A n1, n2;
      ctc_from_above<A, R, WG>(u, tid, xch_lds, n1, n2);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int s = s0 + r;
        const A v1 = r + 1 < R ? u[r + 1 < R ? r + 1 : 0] : n1;
        const A v2 = r + 2 < R ? u[r + 2 < R ? r + 2 : 0] : (r + 2 == R ? n1 : n2);
        beta[r] = s < SS ? ctc_lse3(u[r], v1, s + 1 < SS, v2, s + 2 < SS && h2n[r]) : ninf;
      }
      row = row_n;
#pragma unroll
      for (int r = 0; r < R; ++r) { x[r] = xn[r]; al[r] = aln[r]; }
      row_n = t >= 2 ? row_of(t - 2) : -1;                       // the rows of the next step are in flight
      fetch(row_n, xn, aln);
      if constexpr (!WG) ctc_wave_sync();                        // (the workgroup form: the barrier of the exchange)
    }
  }
}

// ---------------------------------------------------------------- host side
static int ctc_check_entry(const rua_layout* lf, const rua_layout* lt, int32_t V, int32_t S_max, int32_t blank, int es) {
  int e = seg_check_entry(lf, 0, es);
  if (e != 0) return e;
  if ((e = sm_check_layout(lt)) != 0) return e;
  if (lt->B != lf->B) return RUA_EINVAL;
  if (V < 1 || S_max < 0 || S_max > RUA_CTC_MAX_TARGET || blank < 0 || blank >= V) return RUA_EINVAL;
  return 0;
}

static int ctc_bucket(int S_max) {                                      // R of the lanes form; 0: the workgroup form
  const int sp = 2 * S_max + 1;
  return sp <= 64 ? 1 : sp <= 128 ? 2 : sp <= 256 ? 4 : sp <= CTC_LANES_MAX_SP ? 8 : 0;
}

static unsigned ctc_grid(int64_t B, bool wg) {
  const int64_t teams = wg ? B : (B - 1) / RUA_WAVES_PER_BLOCK + 1;
  return (unsigned)(teams < CTC_MAX_GRID ? teams : CTC_MAX_GRID);
}

#define RUA_CTC_BUCKET(R, LAUNCH)                                                                                      \
  switch (R) {                                                                                                         \
    case 1: LAUNCH(1, false); break;                                                                                   \
    case 2: LAUNCH(2, false); break;                                                                                   \
    case 4: LAUNCH(4, false); break;                                                                                   \
    case 8: LAUNCH(8, false); break;                                                                                   \
    default: LAUNCH(8, true); break;                                                                                   \
  }

template <typename E>
static int ctc_forward(const rua_layout& LF, const rua_layout& LT, const void* lp, const void* y, void* alpha, void* codes,
                       void* out, void* logz, void* last, int V, int S_max, int blank, bool vit, int zero_inf,
                       hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  if ((uintptr_t)lp % sizeof(raw) || (uintptr_t)alpha % sizeof(A) || (uintptr_t)out % sizeof(A) ||
      (uintptr_t)logz % sizeof(A) || (uintptr_t)y % 8 || (uintptr_t)last % 8)
    return RUA_EALIGN;
  const int R = ctc_bucket(S_max);
  const unsigned grid = ctc_grid(LF.B, R == 0);
  seg_trace("seg_ctc_forward_kernel T=%s V=%d S_max=%d form=%s R=%d semiring=%s alpha=%d kind=%d tkind=%d grid=%u",
            E::name(), V, S_max, R ? "lanes" : "workgroup", R ? R : 8, vit ? "max" : "log", (int)(alpha != nullptr),
            LF.kind, LT.kind, grid);
#define RUA_CTC_FWD(RR, WG)                                                                                            \
  do {                                                                                                                 \
    if (vit)                                                                                                           \
      hipLaunchKernelGGL((seg_ctc_forward_kernel<E, RR, WG, true>), dim3(grid), dim3(RUA_BLOCK), 0, s, LF, LT,         \
                         (const raw*)lp, (const int64_t*)y, (A*)nullptr, (uint8_t*)codes, (A*)out, (A*)nullptr,        \
                         (int64_t*)last, V, S_max, blank, 0);                                                          \
    else                                                                                                               \
      hipLaunchKernelGGL((seg_ctc_forward_kernel<E, RR, WG, false>), dim3(grid), dim3(RUA_BLOCK), 0, s, LF, LT,        \
                         (const raw*)lp, (const int64_t*)y, (A*)alpha, (uint8_t*)nullptr, (A*)out, (A*)logz,           \
                         (int64_t*)nullptr, V, S_max, blank, zero_inf);                                                \
  } while (0)
  RUA_CTC_BUCKET(R, RUA_CTC_FWD);
#undef RUA_CTC_FWD
  return (int)hipGetLastError();
}

template <typename E>
static int ctc_backward(const rua_layout& LF, const rua_layout& LT, const void* grad, const void* lp, const void* y,
                        const void* alpha, const void* logz, void* gx, int V, int S_max, int blank, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  if ((uintptr_t)lp % sizeof(raw) || (uintptr_t)gx % sizeof(raw) || (uintptr_t)alpha % sizeof(A) ||
      (uintptr_t)logz % sizeof(A) || (uintptr_t)grad % sizeof(A) || (uintptr_t)y % 8)
    return RUA_EALIGN;
  const int R = ctc_bucket(S_max);
  const unsigned grid = ctc_grid(LF.B, R == 0);
  seg_trace("seg_ctc_backward_kernel T=%s V=%d S_max=%d form=%s R=%d kind=%d tkind=%d grid=%u", E::name(), V, S_max,
            R ? "lanes" : "workgroup", R ? R : 8, LF.kind, LT.kind, grid);
#define RUA_CTC_BWD(RR, WG)                                                                                            \
  hipLaunchKernelGGL((seg_ctc_backward_kernel<E, RR, WG>), dim3(grid), dim3(RUA_BLOCK), 0, s, LF, LT, (const A*)grad,  \
                     (const raw*)lp, (const int64_t*)y, (const A*)alpha, (const A*)logz, (raw*)gx, V, S_max, blank)
  RUA_CTC_BUCKET(R, RUA_CTC_BWD);
#undef RUA_CTC_BWD
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int rua_segment_ctc_forward(const rua_layout* frames, const rua_layout* targets, const void* log_probs,
                                       const void* labels, void* alpha, void* codes, void* out, void* logz, void* last,
                                       int32_t V, int32_t S_max, int32_t blank, int32_t dtype, int32_t semiring,
                                       int32_t zero_infinity, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = ctc_check_entry(frames, targets, V, S_max, blank, es)) != 0) return e;
  if (semiring != RUA_CRF_LOG && semiring != RUA_CRF_MAX) return RUA_EINVAL;
  if (frames->B == 0) return 0;
  const bool vit = semiring == RUA_CRF_MAX;
  if (!out || (frames->n_rows > 0 && !log_probs) || (targets->n_rows > 0 && !labels)) return RUA_EINVAL;
  if (vit && (!last || (frames->n_rows > 0 && !codes))) return RUA_EINVAL;
  if (seg_too_large(frames, V, es) || seg_too_large(frames, 2 * (int64_t)S_max + 1, 8)) return RUA_ERANGE;
#define RUA_CTC(E) ctc_forward<E>(*frames, *targets, log_probs, labels, alpha, codes, out, logz, last, V, S_max, blank, vit, zero_infinity != 0, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CTC);
#undef RUA_CTC
}

extern "C" int rua_segment_ctc_backtrace(const rua_layout* frames, const rua_layout* targets, const void* labels,
                                         const void* codes, const void* last, void* out_labels, void* out_positions,
                                         int32_t V, int32_t S_max, int32_t blank, void* stream) {
  using namespace rua;
  int e;
  if ((e = ctc_check_entry(frames, targets, V, S_max, blank, 4)) != 0) return e;
  if (frames->B == 0 || frames->n_rows == 0) return 0;
  if (!codes || !last || !out_labels || !out_positions || (targets->n_rows > 0 && !labels)) return RUA_EINVAL;
  if ((uintptr_t)last % 8 || (uintptr_t)out_labels % 8 || (uintptr_t)out_positions % 8 || (uintptr_t)labels % 8)
    return RUA_EALIGN;
  const int64_t grid = (frames->B - 1) / RUA_BLOCK + 1;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_ctc_backtrace_kernel S_max=%d kind=%d tkind=%d", S_max, frames->kind, targets->kind);
  hipLaunchKernelGGL(seg_ctc_backtrace_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *frames,
                     *targets, (const int64_t*)labels, (const uint8_t*)codes, (const int64_t*)last, (int64_t*)out_labels,
                     (int64_t*)out_positions, S_max, blank);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_ctc_backward(const rua_layout* frames, const rua_layout* targets, const void* grad,
                                        const void* log_probs, const void* labels, const void* alpha, const void* logz,
                                        void* grad_log_probs, int32_t V, int32_t S_max, int32_t blank, int32_t dtype,
                                        void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = ctc_check_entry(frames, targets, V, S_max, blank, es)) != 0) return e;
  if (frames->B == 0 || frames->n_rows == 0) return 0;
  if (!grad || !log_probs || !alpha || !logz || !grad_log_probs || (targets->n_rows > 0 && !labels)) return RUA_EINVAL;
  if (seg_too_large(frames, V, es) || seg_too_large(frames, 2 * (int64_t)S_max + 1, 8)) return RUA_ERANGE;
#define RUA_CTC(E) ctc_backward<E>(*frames, *targets, grad, log_probs, labels, alpha, logz, grad_log_probs, V, S_max, blank, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CTC);
#undef RUA_CTC
}
