// rua_crf.hip — per-sequence linear-chain CRF over the tokens of a C / L / P / R container of emissions [rows, K]
// (rua_segment_crf_forward, rua_segment_crf_backtrace, rua_segment_crf_backward, rua_crf_ws_bytes; include/rua.h;
// DESIGN 3.2o).  An extension: the structured operator the reference's users build on these containers — the log
// partition function, its gradients (the marginals) and Viterbi.  The state of the scan is a VECTOR of K tag scores and
// the combine a K x K semiring product, so none of the one-register-per-element skeletons fits.
//
// Geometry: one wave per sequence, RUA_WAVES_PER_BLOCK waves per workgroup, lane j < K owns tag j; wave w of the launch
// walks the sequences w, w + waves, ... .  The forward keeps COLUMN transitions[:, j] in registers for the whole walk
// (a fully unrolled array of the tag bucket KB = 8 / 16 / 32 / 64), the backward ROW transitions[i, :].  Per step lane j
// needs every alpha[i]; i is wave-uniform, so it is read with a readlane in ascending i — no LDS, no barrier.
//
// ONE evaluation order per (sequence, tag, step), whatever the layout or the bucket (fp32; fp64 for RUA_F64; no
// contraction):
//   alpha_0[j] = start[j] + x_0[j]                                   (start == NULL: 0, the same bits as a zeros tensor)
//   v_i = alpha_{t-1}[i] + transitions[i, j]    for i = 0 .. K-1
//   LOG:  m = max_i v_i;   m == -inf: alpha_t[j] = x_t[j] + (-inf);   else s = sum_i exp(v_i - m) in ascending i and
//         alpha_t[j] = x_t[j] + (m + log s).   A NaN v_i makes m NaN (and so alpha_t[j]).
//   MAX:  the maximum under argmax's total order (a NaN beats every number, the first of equals wins), its i is the
//         backpointer, alpha_t[j] = x_t[j] + max.
//   the end: f_j = alpha_{n-1}[j] + end[j]  (NULL: + 0), folded over j the same way by every lane; lane 0 writes.
// The emission row of step t + 1 is requested before the arithmetic of step t.  Padding rows are never read.
//
// The backward (LOG) walks from the end: beta_{n-1} = end, u_j = x_t[j] + beta_t[j] (lane j),
//   v_j = transitions[i, j] + u_j,  m = max_j v_j,  e_j = exp(v_j - m),  beta_{t-1}[i] = m + log(sum_j e_j)   (lane i)
//   grad_emissions[t, j] = g[b] * exp((alpha_t[j] + beta_t[j]) - logZ[b])
//   grad_transitions[i, j] += e_j * (g[b] * exp((alpha_{t-1}[i] + m) - logZ[b]))        (the pair marginal, the e_j reused)
//   grad_start += g * marginal_0,  grad_end += g * marginal_{n-1}.
// A wave keeps its [K, K] / [K] / [K] sums in registers over all the sequences it walks and leaves ONE part in the
// workspace; a finish launch adds the parts in part order.  No float atomics: the parameter gradients are bitwise
// reproducible from run to run for the same container (the causal conv's rule; nothing is promised across layouts).
//
// KNOWN LIMIT: one very long sequence is walked by one wave (correct, slow).  Cutting a sequence needs K x K matrix
// products per block and is out of scope.
#include <stdio.h>
#include <stdint.h>
#include <initializer_list>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int64_t CRF_FWD_MAX_GRID = 1024;                              // workgroups of the forward: 4 waves per SIMD
constexpr int64_t CRF_MAX_PARTS = 1024;                                 // waves (= parts) of the backward, at most
constexpr int64_t CRF_BWD_MAX_GRID = CRF_MAX_PARTS / RUA_WAVES_PER_BLOCK;
static_assert(RUA_CRF_MAX_TAGS == RUA_WAVE, "a lane per tag");

// the value lane `i` holds (i a constant after unrolling: one v_readlane per 32 bits, the result is wave-uniform)
__device__ __forceinline__ float crf_lane(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}
__device__ __forceinline__ double crf_lane(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// NaN-propagating running maximum: once m is a NaN it stays one
template <typename A> __device__ __forceinline__ A crf_max(A m, A v) { return (v > m || v != v) ? v : m; }
// argmax's order: does v beat the incumbent m?  (a NaN beats every number; equals and later NaNs do not)
template <typename A> __device__ __forceinline__ bool crf_beats(A v, A m) { return v > m || (v != v && m == m); }

// logsumexp of f over the lanes j < K, in ascending j, the same value in every lane
template <typename A, int KB> __device__ __forceinline__ A crf_lse_lanes(A f, int K) {
  A m = -seg_inf<A>();
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j < K) m = crf_max(m, crf_lane(f, j));
  }
  if (m == -seg_inf<A>()) return m;
  A s = (A)0;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j < K) s = s + seg_exp(crf_lane(f, j) - m);
  }
  return m + seg_log(s);
}

// ---------------------------------------------------------------- forward: LOG (the partition) and MAX (Viterbi)
template <typename E, int KB, bool VIT>
__global__ __launch_bounds__(RUA_BLOCK) void seg_crf_forward_kernel(rua_layout L, const typename E::raw* __restrict__ x,
                                                                    const typename E::raw* __restrict__ trans,
                                                                    const typename E::raw* __restrict__ start,
                                                                    const typename E::raw* __restrict__ end,
                                                                    typename E::acc* __restrict__ alpha,
                                                                    uint8_t* __restrict__ backptr,
                                                                    typename E::acc* __restrict__ out,
                                                                    int64_t* __restrict__ last, int K) {
  using A = typename E::acc;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * RUA_WAVES_PER_BLOCK;
  const bool own = lane < K;
  const A ninf = -seg_inf<A>();

  A col[KB];                                                   // transitions[:, lane]
#pragma unroll
  for (int i = 0; i < KB; ++i) col[i] = (own && i < K) ? E::up(trans[i * K + lane]) : ninf;
  const A sv = (own && start) ? E::up(start[lane]) : (A)0;
  const A ev = (own && end) ? E::up(end[lane]) : (A)0;

  for (int64_t b = wave; b < L.B; b += waves) {
    const int64_t len = safe_len(L, b);
    if (len <= 0) {
      if (lane == 0) {
        out[b] = (A)0;
        if (VIT) last[b] = -1;
      }
      continue;
    }
    auto row_of = [&](int64_t t) {
      const int64_t r = token_to_row(L, b, t, len);
      return (r >= 0 && r < L.n_rows) ? r : (int64_t)-1;
    };
    auto emit = [&](int64_t r) { return (own && r >= 0) ? E::up(x[r * K + lane]) : (A)0; };

    int64_t row = row_of(0);
    A a = sv + emit(row);
    if (!own) a = ninf;
    if (alpha && own && row >= 0) alpha[row * K + lane] = a;
    int64_t row_n = len > 1 ? row_of(1) : -1;
    A x_n = emit(row_n);

    for (int64_t t = 1; t < len; ++t) {
      row = row_n;
      const A xt = x_n;
      row_n = t + 1 < len ? row_of(t + 1) : -1;                // the next row is in flight during this step
      x_n = emit(row_n);
      A r;
      if constexpr (VIT) {
        A best = crf_lane(a, 0) + col[0];
        int arg = 0;
#pragma unroll
        for (int i = 1; i < KB; ++i) {
          const A v = crf_lane(a, i) + col[i];
          if (i < K && crf_beats(v, best)) { best = v; arg = i; }
        }
        r = xt + best;
        if (own && row >= 0) backptr[row * K + lane] = (uint8_t)arg;
      } else {
        A m = ninf;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          if (i < K) m = crf_max(m, crf_lane(a, i) + col[i]);
        }
        A s = (A)0;
        const A mm = m == ninf ? (A)0 : m;                     // (a lane whose every v is -inf: s = 0, not used)
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          if (i < K) s = s + seg_exp((crf_lane(a, i) + col[i]) - mm);
        }
        r = xt + (m == ninf ? ninf : m + seg_log(s));
      }
      a = own ? r : ninf;
      if (alpha && own && row >= 0) alpha[row * K + lane] = a;
    }

    const A f = a + ev;
    if constexpr (VIT) {
      A best = crf_lane(f, 0);
      int arg = 0;
#pragma unroll
      for (int j = 1; j < KB; ++j) {
        const A v = crf_lane(f, j);
        if (j < K && crf_beats(v, best)) { best = v; arg = j; }
      }
      if (lane == 0) { out[b] = best; last[b] = arg; }
    } else {
      const A z = crf_lse_lanes<A, KB>(f, K);
      if (lane == 0) out[b] = z;
    }
  }
}

// ---------------------------------------------------------------- Viterbi's backtrace: a thread per sequence
__global__ __launch_bounds__(RUA_BLOCK) void seg_crf_backtrace_kernel(rua_layout L, const uint8_t* __restrict__ backptr,
                                                                      const int64_t* __restrict__ last,
                                                                      int64_t* __restrict__ tags, int K) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  int64_t tag = last[b];
  if (tag < 0 || tag >= K) tag = 0;
  for (int64_t t = len - 1; t >= 0; --t) {
    const int64_t row = token_to_row(L, b, t, len);
    if (row < 0 || row >= L.n_rows) continue;
    tags[row] = tag;
    if (t > 0) {
      tag = backptr[row * K + tag];
      if (tag >= K) tag = 0;
    }
  }
  seg_fill_padding(L, b, len, 0, 1, [&](int64_t row) { tags[row] = 0; });
}

// ---------------------------------------------------------------- backward of the partition
// lane i holds row transitions[i, :] and the sums of grad_transitions[i, :]; lane j the emission / alpha / beta of tag j
template <typename E, int KB>
__global__ __launch_bounds__(RUA_BLOCK) void seg_crf_backward_kernel(rua_layout L, const typename E::acc* __restrict__ grad,
                                                                     const typename E::raw* __restrict__ x,
                                                                     const typename E::raw* __restrict__ trans,
                                                                     const typename E::raw* __restrict__ end,
                                                                     const typename E::acc* __restrict__ alpha,
                                                                     const typename E::acc* __restrict__ logz,
                                                                     typename E::raw* __restrict__ gx,
                                                                     typename E::acc* __restrict__ ws, int K) {
  using A = typename E::acc;
  using raw = typename E::raw;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int64_t wave = (int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * RUA_WAVES_PER_BLOCK;
  const bool own = lane < K;
  const A ninf = -seg_inf<A>();

  A rw[KB], gt[KB];                                            // transitions[lane, :], the sums of its gradient
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    rw[j] = (own && j < K) ? E::up(trans[lane * K + j]) : ninf;
    gt[j] = (A)0;
  }
  const A ev = (own && end) ? E::up(end[lane]) : (A)0;
  A gs = (A)0, ge = (A)0;

  for (int64_t b = wave; b < L.B; b += waves) {
    const int64_t len = safe_len(L, b);
    if (gx && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
      // the padding rows of grad_emissions: zeros, 64 elements per step
      const int64_t n = L.T_phys * K;
      for (int64_t idx = lane; idx < n; idx += RUA_WAVE) {
        const int64_t pos = div_rows(idx, K);
        const int64_t row = b * L.T_phys + pos;
        if (is_pad(L, pos, len) && row < L.n_rows) gx[b * n + idx] = (raw)0;
      }
    }
    if (len <= 0) continue;
    auto row_of = [&](int64_t t) {
      const int64_t r = token_to_row(L, b, t, len);
      return (r >= 0 && r < L.n_rows) ? r : (int64_t)-1;
    };
    const A g = grad[b], lz = logz[b];
    if (lz == ninf) {
      // every path of the sequence is forbidden: exact zeros, and nothing for the parameters (a documented choice)
      if (gx && own) {
        for (int64_t t = 0; t < len; ++t) {
          const int64_t r = row_of(t);
          if (r >= 0) gx[r * K + lane] = (raw)0;
        }
      }
      continue;
    }
    int64_t row = row_of(len - 1);
    A a_t = (own && row >= 0) ? alpha[row * K + lane] : ninf;
    A x_t = (own && row >= 0) ? E::up(x[row * K + lane]) : (A)0;
    A beta = own ? ev : ninf;
    A marg = g * seg_exp((a_t + beta) - lz);
    if (gx && own && row >= 0) gx[row * K + lane] = E::down(marg);
    if (own) ge = ge + marg;
    int64_t row_p = len > 1 ? row_of(len - 2) : -1;
    A a_p = (own && row_p >= 0) ? alpha[row_p * K + lane] : ninf;
    A x_p = (own && row_p >= 0) ? E::up(x[row_p * K + lane]) : (A)0;

    for (int64_t t = len - 1; t >= 1; --t) {
      const A u = x_t + beta;                                  // lane j: x_t[j] + beta_t[j]
      const A a_prev = a_p;                                    // lane i: alpha_{t-1}[i]
      const int64_t row_prev = row_p;
      x_t = x_p;
      row_p = t >= 2 ? row_of(t - 2) : -1;                     // the rows of the next step are in flight during this one
      a_p = (own && row_p >= 0) ? alpha[row_p * K + lane] : ninf;
      x_p = (own && row_p >= 0) ? E::up(x[row_p * K + lane]) : (A)0;

      A m = ninf;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < K) m = crf_max(m, rw[j] + crf_lane(u, j));
      }
      const A mm = m == ninf ? (A)0 : m;
      const A w = m == ninf ? (A)0 : g * seg_exp((a_prev + m) - lz);
      A s = (A)0;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < K) {
          const A e = seg_exp((rw[j] + crf_lane(u, j)) - mm);
          s = s + e;
          gt[j] = gt[j] + e * w;
        }
      }
      beta = (own && m != ninf) ? m + seg_log(s) : ninf;
      marg = g * seg_exp((a_prev + beta) - lz);
      if (gx && own && row_prev >= 0) gx[row_prev * K + lane] = E::down(marg);
    }
    if (own) gs = gs + marg;                                   // the marginal of token 0
  }

  if (ws && own) {
    // ws[part][K * K + K + K]: grad_transitions (row-major), grad_start, grad_end — in the accumulator type
    A* p = ws + wave * ((int64_t)K * K + 2 * K);
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < K) p[lane * K + j] = gt[j];
    }
    p[K * K + lane] = gs;
    p[K * K + K + lane] = ge;
  }
}

// the finish: the parts, in part order
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_crf_finish_kernel(const typename E::acc* __restrict__ ws,
                                                                   typename E::raw* __restrict__ gt,
                                                                   typename E::raw* __restrict__ gs,
                                                                   typename E::raw* __restrict__ ge, int K, int parts) {
  using A = typename E::acc;
  const int n = K * K + 2 * K;
  const int i = (int)(blockIdx.x * RUA_BLOCK + threadIdx.x);
  if (i >= n) return;
  A sum = (A)0;
  for (int64_t p = 0; p < parts; ++p) sum = sum + ws[p * n + i];
  if (i < K * K) {
    if (gt) gt[i] = E::down(sum);
  } else if (i < K * K + K) {
    if (gs) gs[i - K * K] = E::down(sum);
  } else if (ge) {
    ge[i - K * K - K] = E::down(sum);
  }
}

// ---------------------------------------------------------------- host side
static int64_t crf_groups(int64_t B) { return (B - 1) / RUA_WAVES_PER_BLOCK + 1; }                 // B > 0
static int64_t crf_parts(int64_t B) {
  const int64_t g = crf_groups(B);
  return (g < CRF_BWD_MAX_GRID ? g : CRF_BWD_MAX_GRID) * RUA_WAVES_PER_BLOCK;
}

// the layout, the dtype (`es`) and K
static int crf_check_entry(const rua_layout* lay, int32_t K, int es) {
  const int e = seg_check_entry(lay, 0, es);
  if (e != 0) return e;
  return (K < 1 || K > RUA_CRF_MAX_TAGS) ? RUA_EINVAL : 0;
}

static bool crf_misaligned(std::initializer_list<const void*> ptrs, size_t to) {
  for (const void* p : ptrs) if ((uintptr_t)p % to) return true;
  return false;
}

#define RUA_CRF_BUCKET(K, LAUNCH)                                                                                      \
  do {                                                                                                                 \
    if (K <= 8) LAUNCH(8); else if (K <= 16) LAUNCH(16); else if (K <= 32) LAUNCH(32); else LAUNCH(64);                \
  } while (0)

template <typename E>
static int crf_forward(const rua_layout& L, const void* x, const void* trans, const void* start, const void* end,
                       void* alpha, void* backptr, void* out, void* last, int K, bool vit, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  if (crf_misaligned({x, trans, start, end}, sizeof(raw)) || crf_misaligned({alpha, out}, sizeof(A)) ||
      crf_misaligned({last}, 8))
    return RUA_EALIGN;
  const int64_t groups = crf_groups(L.B);
  const unsigned grid = (unsigned)(groups < CRF_FWD_MAX_GRID ? groups : CRF_FWD_MAX_GRID);
  seg_trace("seg_crf_forward_kernel T=%s K=%d bucket=%d semiring=%s alpha=%d kind=%d grid=%u", E::name(), K,
            K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64, vit ? "max" : "log", (int)(alpha != nullptr), L.kind, grid);
#define RUA_CRF_FWD(KB)                                                                                                \
  do {                                                                                                                 \
    if (vit)                                                                                                           \
      hipLaunchKernelGGL((seg_crf_forward_kernel<E, KB, true>), dim3(grid), dim3(RUA_BLOCK), 0, s, L, (const raw*)x,   \
                         (const raw*)trans, (const raw*)start, (const raw*)end, (A*)nullptr, (uint8_t*)backptr,        \
                         (A*)out, (int64_t*)last, K);                                                                  \
    else                                                                                                               \
      hipLaunchKernelGGL((seg_crf_forward_kernel<E, KB, false>), dim3(grid), dim3(RUA_BLOCK), 0, s, L, (const raw*)x,  \
                         (const raw*)trans, (const raw*)start, (const raw*)end, (A*)alpha, (uint8_t*)nullptr, (A*)out, \
                         (int64_t*)nullptr, K);                                                                        \
  } while (0)
  RUA_CRF_BUCKET(K, RUA_CRF_FWD);
#undef RUA_CRF_FWD
  return (int)hipGetLastError();
}

template <typename E>
static int crf_backward(const rua_layout& L, const void* grad, const void* x, const void* trans, const void* end,
                        const void* alpha, const void* logz, void* gx, void* gt, void* gs, void* ge, int K, void* ws,
                        hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  if (crf_misaligned({x, trans, end, gx, gt, gs, ge}, sizeof(raw)) || crf_misaligned({grad, alpha, logz, ws}, sizeof(A)))
    return RUA_EALIGN;
  const int parts = (int)crf_parts(L.B);
  const unsigned grid = (unsigned)(parts / RUA_WAVES_PER_BLOCK);
  const bool params = gt || gs || ge;
  seg_trace("seg_crf_backward_kernel T=%s K=%d bucket=%d kind=%d grid=%u parts=%d", E::name(), K,
            K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64, L.kind, grid, params ? parts : 0);
#define RUA_CRF_BWD(KB)                                                                                                \
  hipLaunchKernelGGL((seg_crf_backward_kernel<E, KB>), dim3(grid), dim3(RUA_BLOCK), 0, s, L, (const A*)grad,           \
                     (const raw*)x, (const raw*)trans, (const raw*)end, (const A*)alpha, (const A*)logz, (raw*)gx,     \
                     params ? (A*)ws : (A*)nullptr, K)
  RUA_CRF_BUCKET(K, RUA_CRF_BWD);
#undef RUA_CRF_BWD
  int e = (int)hipGetLastError();
  if (e || !params) return e;
  const int n = K * K + 2 * K;
  seg_trace("seg_crf_finish_kernel T=%s K=%d parts=%d", E::name(), K, parts);
  hipLaunchKernelGGL((seg_crf_finish_kernel<E>), dim3((unsigned)((n + RUA_BLOCK - 1) / RUA_BLOCK)), dim3(RUA_BLOCK), 0, s,
                     (const A*)ws, (raw*)gt, (raw*)gs, (raw*)ge, K, parts);
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int64_t rua_crf_ws_bytes(const rua_layout* lay, int32_t K, int32_t dtype) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  if (crf_check_entry(lay, K, es) != 0 || lay->B <= 0) return 0;
  return crf_parts(lay->B) * ((int64_t)K * K + 2 * K) * (es == 8 ? 8 : 4);
}

extern "C" int rua_segment_crf_forward(const rua_layout* lay, const void* emissions, const void* transitions,
                                       const void* start, const void* end, void* alpha, void* backptr, void* out,
                                       void* last, int32_t K, int32_t dtype, int32_t semiring, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = crf_check_entry(lay, K, es)) != 0) return e;
  if (semiring != RUA_CRF_LOG && semiring != RUA_CRF_MAX) return RUA_EINVAL;
  if (lay->B == 0) return 0;
  const bool vit = semiring == RUA_CRF_MAX;
  if (!transitions || !out || (lay->n_rows > 0 && !emissions)) return RUA_EINVAL;
  if (vit && (!last || (lay->n_rows > 0 && !backptr))) return RUA_EINVAL;
  if (seg_too_large(lay, K, es == 8 ? 8 : 4)) return RUA_ERANGE;
#define RUA_CRF(E) crf_forward<E>(*lay, emissions, transitions, start, end, alpha, backptr, out, last, K, vit, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CRF);
#undef RUA_CRF
}

extern "C" int rua_segment_crf_backtrace(const rua_layout* lay, const void* backptr, const void* last, void* tags,
                                         int32_t K, void* stream) {
  using namespace rua;
  int e;
  if ((e = crf_check_entry(lay, K, 4)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0) return 0;
  if (!backptr || !last || !tags) return RUA_EINVAL;
  if ((uintptr_t)last % 8 || (uintptr_t)tags % 8) return RUA_EALIGN;
  const int64_t grid = (lay->B - 1) / RUA_BLOCK + 1;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_crf_backtrace_kernel K=%d kind=%d", K, lay->kind);
  hipLaunchKernelGGL(seg_crf_backtrace_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *lay,
                     (const uint8_t*)backptr, (const int64_t*)last, (int64_t*)tags, K);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_crf_backward(const rua_layout* lay, const void* grad, const void* emissions,
                                        const void* transitions, const void* end, const void* alpha, const void* logz,
                                        void* grad_emissions, void* grad_transitions, void* grad_start, void* grad_end,
                                        int32_t K, int32_t dtype, void* ws, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = crf_check_entry(lay, K, es)) != 0) return e;
  if (lay->B == 0) return 0;
  if (!grad_emissions && !grad_transitions && !grad_start && !grad_end) return 0;
  if (!grad || !transitions || !logz || (lay->n_rows > 0 && (!emissions || !alpha))) return RUA_EINVAL;
  if ((grad_transitions || grad_start || grad_end) && !ws) return RUA_EINVAL;
  if (seg_too_large(lay, K, es == 8 ? 8 : 4)) return RUA_ERANGE;
#define RUA_CRF(E) crf_backward<E>(*lay, grad, emissions, transitions, end, alpha, logz, grad_emissions, grad_transitions, grad_start, grad_end, K, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CRF);
#undef RUA_CRF
}
