// rua_window.hip — per-sequence sliding-window pooling over the tokens of a C / L / P / R container (rua_window_lens,
// rua_segment_window_pool, rua_segment_window_spread; include/rua.h).  An extension, and the first operator whose new
// raggedness is a CLOSED FORM of the old one: a sequence of n tokens, a window K and a step S give
//   floor:  n_out = (n - K) / S + 1 if n >= K, else 0
//   ceil:   m = ceil(max(n - K, 0) / S) + 1, n_out = m - 1 if (m - 1) * S >= n, else m        (n <= 0: 0)
// windows, and window u covers the tokens [u * S, min(u * S + K, n)) — clipped at the end of the sequence, never empty.
// The pool is DESTINATION-driven: a window reads its at most K source rows through the source layout's own row formula
// and writes one row, so any two kinds meet and padding is never read.  The spread — the adjoint — is SOURCE-driven:
// token t gathers the windows [ceil((t - K + 1) / S), floor(t / S)] that exist, in ascending u; no atomics.
//
// ONE evaluation order per (window, column), whatever the layouts, the kernel form, the alignment or the block border:
//   sum / mean  the accumulator (fp32; fp64 for RUA_F64; int64, wrapping, for RUA_I64) starts at the window's first token
//               and adds the others in ascending position; mean divides once by the number of tokens IN the window, in the
//               accumulator type; one rounding.  The value about to be rounded is opaque to the optimiser (wp_pin), as in
//               rua_conv.hip.
//   max         argmax's total order on (value, position): a NaN beats every number, the first NaN or first maximum
//               wins, -0.0 == +0.0.  The output holds the winner's BITS; `arg` its offset inside the window (one byte).
//   take        out[u] = data[u * S + arg[u]]: max, given its arg table, as the linear map it is.
//   spread      the accumulator starts at +0 and adds g[u] (sum), g[u] / cnt[u] (mean: divided first) or g[u] where
//               arg[u] == t - u * S (max / take); one rounding.  Tokens in no window and padding rows get +0.
// Nothing is folded across windows or tokens, so blocks and tiles change no bit.
//
// Forms (rua_conv.hip's): rows of one vector (<= 16 bytes) put consecutive windows (the spread: tokens) of a
// sequence on 32 consecutive lanes, two sequences per wave; wider rows give a workgroup per (sequence x 128-byte column
// chunk), thread (q, l) = (tid / 8, tid % 8) takes the windows q, q + 32, ... and the l-th 16-byte vector of the chunk
// (AL = false: rows or bases off 16 bytes, the same geometry with elementwise accesses).  Few but long sequences — the
// family's cut rule over the BIG side — are cut across workgroups: block i of the spread takes the tokens
// [2048 i, 2048 (i + 1)), block i of the pool the windows that BEGIN there.  Blocks need nothing of each other: no
// workspace, no second launch.
#include <stdio.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int WP_SLOTS = 32;               // windows (tokens) a workgroup of the rows form, or a half wave, has in flight
constexpr int WP_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
static_assert(WP_SLOTS * WP_LPR == RUA_BLOCK, "a thread per (slot, 16-byte lane of the chunk)");
static_assert(RUA_WINDOW_MAX_K <= 256, "a window offset fits one byte");
static_assert(RUA_WINDOW_TAKE != RUA_SUM && RUA_WINDOW_TAKE != RUA_MEAN && RUA_WINDOW_TAKE != RUA_MAX, "four modes");

struct wp_i64 {                            // unsigned accumulation: the sum wraps
  using raw = int64_t; using acc = uint64_t;
  static __device__ __forceinline__ acc up(raw v) { return (acc)v; }
  static __device__ __forceinline__ raw down(acc v) { return (raw)v; }
  static const char* name() { return "i64"; }
};

// x, at a later position, takes the window from `best`
template <typename E> __device__ __forceinline__ bool wp_beats(typename E::raw x, typename E::raw best) {
  if constexpr (std::is_same<E, wp_i64>::value) {
    return x > best;
  } else {
    const typename E::acc xv = E::up(x), bv = E::up(best);
    return xv > bv || (xv != xv && bv == bv);
  }
}

// a value about to be rounded to the payload dtype, opaque to the optimiser (see the head of rua_conv.hip)
template <typename A> __device__ __forceinline__ A wp_pin(A v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ int64_t wp_ceil_div(int64_t a, int64_t s) { return (a + s - 1) / s; }    // a >= 0, s >= 1

// the number of windows of a sequence of n tokens
__device__ __forceinline__ int64_t wp_n_out(int64_t n, int64_t K, int64_t S, int ceil_mode) {
  if (n <= 0) return 0;
  if (!ceil_mode) return n >= K ? (n - K) / S + 1 : 0;
  const int64_t m1 = wp_ceil_div(n > K ? n - K : 0, S);      // m - 1
  return m1 * S >= n ? m1 : m1 + 1;
}

// the tokens [t0, te) of window u of a sequence of `slen`; t0 == te: the window does not exist
__device__ __forceinline__ void wp_window(int64_t u, int64_t K, int64_t S, int64_t slen, int64_t& t0, int64_t& te) {
  if (__builtin_mul_overflow(u, S, &t0) || t0 >= slen) { t0 = te = 0; return; }
  te = slen - t0 > K ? t0 + K : slen;
}

// the windows [ulo, uhi] that hold token t (ulo > uhi: none — a gap of S > K, or a dropped tail), of `dlen` windows
__device__ __forceinline__ void wp_windows_of(int64_t t, int64_t K, int64_t S, int64_t dlen, int64_t& ulo, int64_t& uhi) {
  uhi = div_rows(t, S);
  const int64_t r = t - uhi * S;                             // the token's offset in the LAST window that begins before it
  ulo = uhi + 1;
  if (r > K - 1) return;
  const int64_t room = K - 1 - r;                            // < 64
  const int64_t back = S > room ? 0 : (int64_t)((uint32_t)room / (uint32_t)S);
  ulo = uhi - back > 0 ? uhi - back : 0;
  if (uhi > dlen - 1) uhi = dlen - 1;
}

// the windows [ub, ue) of a sequence of `dlen` windows that block `blk` of `maxblk` takes: those that begin in its
// SEG_BLOCK_TOK tokens; the last block takes what a length bound that understates left over
__device__ __forceinline__ void wp_block_windows(int maxblk, int blk, int64_t S, int64_t dlen, int64_t& ub, int64_t& ue) {
  ub = 0;
  ue = dlen;
  if (maxblk > 0) {
    ub = wp_ceil_div((int64_t)blk * SEG_BLOCK_TOK, S);
    if (blk < maxblk - 1) {
      const int64_t e = wp_ceil_div((int64_t)(blk + 1) * SEG_BLOCK_TOK, S);
      if (e < ue) ue = e;
    }
    if (ub > ue) ub = ue;
  }
}

// ---------------------------------------------------------------- the lengths
// a thread per sequence.  out[b] = the windows of the sequence's CLAMPED length; own_out[b] (optional) = the length as
// the layout GIVES it (what a host mirror of that vector holds)
__global__ __launch_bounds__(RUA_BLOCK) void seg_window_lens_kernel(rua_layout L, int K, int64_t S, int ceil_mode,
                                                                    int64_t* __restrict__ out,
                                                                    int64_t* __restrict__ own_out) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= L.B) return;
  out[b] = wp_n_out(safe_len(L, b), K, S, ceil_mode);
  if (own_out) own_out[b] = seq_len(L, b);
}

// ---------------------------------------------------------------- one window / one token, VE columns of it
// `ld(row, v)` loads the thread's VE columns of a storage row (columns past the row as zeros)
template <typename E, int VE> struct wp_vec { typename E::raw e[VE]; };

// window u of sequence b -> o (and, MAX, a: the winners' offsets).  TAKE reads `a`.
template <typename E, int VE, typename Ld>
__device__ __forceinline__ void wp_pool_one(const rua_layout& Sl, int64_t b, int64_t slen, int64_t u, int K, int64_t S,
                                            int mode, Ld ld, wp_vec<E, VE>& o, uint8_t (&a)[VE]) {
  using raw = typename E::raw;
  using A = typename E::acc;
  A acc[VE];
  raw best[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { acc[e] = (A)0; best[e] = (raw)0; }
  int64_t t0, te;
  wp_window(u, K, S, slen, t0, te);
  bool first = true;
  int cnt = 0;
#pragma unroll 4
  for (int64_t t = t0; t < te; ++t) {
    const int64_t row = token_to_row(Sl, b, t, slen);
    if (row < 0 || row >= Sl.n_rows) continue;
    wp_vec<E, VE> v;
    ld(row, v);
    ++cnt;
    const int off = (int)(t - t0);
    if (mode == RUA_WINDOW_TAKE) {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (a[e] == off) best[e] = v.e[e];
    } else if (mode == RUA_MAX) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (first || wp_beats<E>(v.e[e], best[e])) { best[e] = v.e[e]; a[e] = (uint8_t)off; }
      }
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[e] = first ? E::up(v.e[e]) : acc[e] + E::up(v.e[e]);
    }
    first = false;
  }
  if (mode == RUA_MAX && first) {
#pragma unroll
    for (int e = 0; e < VE; ++e) a[e] = 0;
  }
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (mode == RUA_MAX || mode == RUA_WINDOW_TAKE) o.e[e] = best[e];
    else if (mode == RUA_MEAN && cnt > 0) o.e[e] = E::down(wp_pin((A)(acc[e] / (A)cnt)));
    else o.e[e] = E::down(wp_pin(acc[e]));
  }
}

// token t of sequence b of the big side <- the windows that hold it.  `lda(row, a)`: the VE arg bytes of a pooled row
template <typename E, int VE, typename Ld, typename Lda>
__device__ __forceinline__ void wp_spread_one(const rua_layout& Pl, int64_t b, int64_t slen, int64_t dlen, int64_t t, int K,
                                              int64_t S, int mode, Ld ld, Lda lda, wp_vec<E, VE>& o) {
  using A = typename E::acc;
  A acc[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) acc[e] = (A)0;
  int64_t ulo, uhi;
  wp_windows_of(t, K, S, dlen, ulo, uhi);
  for (int64_t u = ulo; u <= uhi; ++u) {
    const int64_t row = token_to_row(Pl, b, u, dlen);
    if (row < 0 || row >= Pl.n_rows) continue;
    wp_vec<E, VE> v;
    ld(row, v);
    const int64_t t0 = u * S;                                // (u <= t / S: no overflow)
    if (mode == RUA_SUM) {
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[e] = acc[e] + E::up(v.e[e]);
    } else if (mode == RUA_MEAN) {
      const A cnt = (A)(slen - t0 > K ? (int64_t)K : slen - t0);
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[e] = acc[e] + (A)(E::up(v.e[e]) / cnt);
    } else {
      uint8_t a[VE];
      lda(row, a);
      const int off = (int)(t - t0);
#pragma unroll
      for (int e = 0; e < VE; ++e) if (a[e] == off) acc[e] = acc[e] + E::up(v.e[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VE; ++e) o.e[e] = E::down(wp_pin(acc[e]));
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup per unit and 128-byte column chunk; a unit is a sequence, or (maxblk > 0: few but long sequences) a block
// of one.  SPREAD == false: the pool — D is the pooled side (written), Sl the big side; SPREAD == true: the spread — D is
// the big side (written), Sl the pooled side.  `argal`: H and the arg table's base are multiples of VE, so the VE bytes
// of a thread are one access.
template <typename E, bool AL, bool SPREAD>
__global__ __launch_bounds__(RUA_BLOCK) void seg_window_rows_kernel(rua_layout Sl, rua_layout D,
                                                                    const typename E::raw* __restrict__ in,
                                                                    typename E::raw* __restrict__ out, uint8_t* arg,
                                                                    int64_t H, int n_chunks, int maxblk, int K, int64_t S,
                                                                    int mode, int argal) {
  using raw = typename E::raw;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = WP_LPR * VE;
  using Vec = wp_vec<E, VE>;
  using ArgWord = typename row_word<VE>::t;

  const int tid = threadIdx.x;
  const int l = tid & (WP_LPR - 1), q = tid >> 3;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  const int64_t unit = blockIdx.x / (unsigned)n_chunks;
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  if (nval <= 0) return;                                      // (no collective below)
  int64_t b = unit;
  int blk = 0;
  if (maxblk > 0) { blk = (int)(unit % maxblk); b = unit / maxblk; }
  if (b >= D.B) return;

  auto ld = [&](int64_t row, Vec& v) {
    const raw* p = in + row * H + col0;
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
  auto lda = [&](int64_t row, uint8_t (&a)[VE]) {
    const uint8_t* p = arg + row * H + col0;
    if (AL && argal) {
      const ArgWord wv = *(const ArgWord*)p;
      __builtin_memcpy(a, &wv, VE);
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) a[e] = e < nval ? p[e] : (uint8_t)0xff;
    }
  };
  auto sta = [&](int64_t row, const uint8_t (&a)[VE]) {
    uint8_t* p = arg + row * H + col0;
    if (AL && argal) {
      ArgWord wv;
      __builtin_memcpy(&wv, a, VE);
      *(ArgWord*)p = wv;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (e < nval) p[e] = a[e];
    }
  };

  const int64_t rlen = safe_len(Sl, b), wlen = safe_len(D, b);       // the side that is read, the side that is written
  if constexpr (!SPREAD) {
    int64_t ub, ue;
    wp_block_windows(maxblk, blk, S, wlen, ub, ue);
    for (int64_t u = ub + q; u < ue; u += WP_SLOTS) {
      const int64_t row = token_to_row(D, b, u, wlen);
      if (row < 0 || row >= D.n_rows) continue;
      Vec o;
      uint8_t a[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) a[e] = 0;
      if (mode == RUA_WINDOW_TAKE) lda(row, a);
      wp_pool_one<E, VE>(Sl, b, rlen, u, K, S, mode, ld, o, a);
      st(row, o);
      if (mode == RUA_MAX && arg) sta(row, a);
    }
  } else {
    int64_t tb, te;
    seg_block_range(maxblk, blk, wlen, tb, te);
    for (int64_t t = tb + q; t < te; t += WP_SLOTS) {
      const int64_t row = token_to_row(D, b, t, wlen);
      if (row < 0 || row >= D.n_rows) continue;
      Vec o;
      wp_spread_one<E, VE>(Sl, b, wlen, rlen, t, K, S, mode, ld, lda, o);
      st(row, o);
    }
  }

  if (blk == 0 && (D.kind == RUA_LEFT || D.kind == RUA_RIGHT)) {
    Vec z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < D.T_phys; j += WP_SLOTS) {
      if (!is_pad(D, j, wlen)) continue;
      const int64_t row = b * D.T_phys + j;
      if (row < D.n_rows) st(row, z);
    }
  }
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// Two sequences per wave, 32 lanes each; lane r of a half takes the windows (the spread: tokens) r, r + 32, ... of its
// sequence.  Rows move in accesses of W bytes (seg_access_width).  No collective: lanes need nothing of each other.
template <typename E, bool SPREAD>
__global__ __launch_bounds__(RUA_BLOCK) void seg_window_lanes_kernel(rua_layout Sl, rua_layout D, const char* __restrict__ in,
                                                                     char* __restrict__ out, uint8_t* arg, int H, int W,
                                                                     int K, int64_t S, int mode) {
  using raw = typename E::raw;
  constexpr int VE = 16 / (int)sizeof(raw);
  union alignas(16) Row { wp_vec<E, VE> v; uint32_t d[4]; };

  const int tid = threadIdx.x;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int q = lane & (WP_SLOTS - 1);
  const int nb = H * (int)sizeof(raw);
  const int64_t b = ((int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + w) * 2 + (lane >> 5);
  if (b >= D.B) return;

  auto ld = [&](int64_t row, wp_vec<E, VE>& v) {
    Row r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.d[i] = 0u;
    ld_row_w(in + row * nb, nb, W, &r);
    v = r.v;
  };
  auto st = [&](int64_t row, const wp_vec<E, VE>& v) {
    Row r;
    r.v = v;
    st_row_w(out + row * nb, nb, W, &r);
  };
  auto lda = [&](int64_t row, uint8_t (&a)[VE]) {
#pragma unroll
    for (int e = 0; e < VE; ++e) a[e] = e < H ? arg[row * H + e] : (uint8_t)0xff;
  };

  const int64_t rlen = safe_len(Sl, b), wlen = safe_len(D, b);       // the side that is read, the side that is written
  for (int64_t u = q; u < wlen; u += WP_SLOTS) {
    const int64_t row = token_to_row(D, b, u, wlen);
    if (row < 0 || row >= D.n_rows) continue;
    wp_vec<E, VE> o;
    if constexpr (!SPREAD) {
      uint8_t a[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) a[e] = 0;
      if (mode == RUA_WINDOW_TAKE) lda(row, a);
      wp_pool_one<E, VE>(Sl, b, rlen, u, K, S, mode, ld, o, a);
      if (mode == RUA_MAX && arg) {
#pragma unroll
        for (int e = 0; e < VE; ++e) if (e < H) arg[row * H + e] = a[e];
      }
    } else {
      wp_spread_one<E, VE>(Sl, b, wlen, rlen, u, K, S, mode, ld, lda, o);
    }
    st(row, o);
  }
  if (D.kind == RUA_LEFT || D.kind == RUA_RIGHT) {
    wp_vec<E, VE> z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
    for (int64_t j = q; j < D.T_phys; j += WP_SLOTS) {
      if (!is_pad(D, j, wlen)) continue;
      const int64_t row = b * D.T_phys + j;
      if (row < D.n_rows) st(row, z);
    }
  }
}

// ---------------------------------------------------------------- host side
static const char* wp_mode_name(int mode) {
  switch (mode) {
    case RUA_SUM:  return "sum";
    case RUA_MEAN: return "mean";
    case RUA_MAX:  return "max";
  }
  return "take";
}

// `big` decides the form and the cut (the family's rule: seg_make_plan); `wr` is the side that is written (the pooled
// side of the pool, the big side of the spread), `rd` the side that is read
template <typename E, bool SPREAD>
static int wp_launch(const rua_layout& big, const rua_layout& rd, const rua_layout& wr, const void* in, void* out,
                     const void* arg, int64_t H, int K, int64_t S, int mode, hipStream_t s) {
  using raw = typename E::raw;
  const int es = (int)sizeof(raw);
  const int64_t row_bytes = H * es;
  const uint64_t bases = (uint64_t)(uintptr_t)in | (uint64_t)(uintptr_t)out;
  if (bases % sizeof(raw)) return RUA_EALIGN;
  const seg_plan p = seg_make_plan(big, H, es, 0);
  if (p.n_chunks <= 0) return RUA_ERANGE;
  const char* name = SPREAD ? "seg_window_spread_kernel" : "seg_window_pool_kernel";

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, wr.B);
    if (!ln.grid) return RUA_ERANGE;
    seg_trace("%s form=lanes T=%s K=%d S=%lld mode=%s kind=%d from=%d W=%d H=%d cut=0 blocks=0", name, E::name(), K,
              (long long)S, wp_mode_name(mode), wr.kind, rd.kind, ln.W, (int)H);
    hipLaunchKernelGGL((seg_window_lanes_kernel<E, SPREAD>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, rd, wr,
                       (const char*)in, (char*)out, (uint8_t*)arg, (int)H, ln.W, K, S, mode);
    return (int)hipGetLastError();
  }
  const bool cut = p.maxblk > 0;
  const int64_t grid = seg_rows_grid(big, p, cut);
  if (!grid) return RUA_ERANGE;
  const bool al = row_bytes % 16 == 0 && bases % 16 == 0;
  constexpr int VE = 16 / es;
  const int argal = arg && H % VE == 0 && (uint64_t)(uintptr_t)arg % VE == 0;
  seg_trace("%s form=%s T=%s K=%d S=%lld mode=%s kind=%d from=%d AL=%d cut=%d blocks=%d chunks=%d", name,
            al ? "rows" : "unaligned", E::name(), K, (long long)S, wp_mode_name(mode), wr.kind, rd.kind, (int)al, (int)cut,
            p.maxblk, p.n_chunks);
  seg_with_al(al, [&](auto AL) {
    hipLaunchKernelGGL((seg_window_rows_kernel<E, decltype(AL)::value, SPREAD>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0,
                       s, rd, wr, (const raw*)in, (raw*)out, (uint8_t*)arg, H, p.n_chunks, p.maxblk, K, S, mode, argal);
  });
  return (int)hipGetLastError();
}

template <bool SPREAD>
static int wp_dispatch(const rua_layout* big, const rua_layout* rd, const rua_layout* wr, const void* in, void* out,
                       const void* arg, int64_t H, int K, int64_t S, int mode, int32_t dtype, void* stream) {
#define RUA_WP(E) wp_launch<E, SPREAD>(*big, *rd, *wr, in, out, arg, H, K, S, mode, (hipStream_t)stream)
  if (dtype == RUA_I64) return RUA_WP(wp_i64);
  RUA_DISPATCH_FLOAT(dtype, RUA_WP);
#undef RUA_WP
}

// K, then S
static int wp_check_window(int32_t K, int32_t S) {
  if (K < 1 || S < 1) return RUA_EINVAL;
  return K > RUA_WINDOW_MAX_K ? RUA_ERANGE : 0;
}

// both layouts, then H and the dtype, the mode, K and S — before any pointer is looked at
static int wp_check_entry(const rua_layout* pooled, const rua_layout* big, int64_t H, int32_t K, int32_t S, int32_t mode,
                          int32_t dtype, int es) {
  int e;
  if ((e = seg_check_entry(big, H, es)) != 0) return e;
  if ((e = seg_check_entry(pooled, H, es)) != 0) return e;
  if (pooled->B != big->B) return RUA_EINVAL;
  if (mode != RUA_SUM && mode != RUA_MEAN && mode != RUA_MAX && mode != RUA_WINDOW_TAKE) return RUA_EINVAL;
  if (dtype == RUA_I64 && mode == RUA_MEAN) return RUA_EINVAL;
  return wp_check_window(K, S);
}

}  // namespace rua

extern "C" int rua_window_lens(const rua_layout* lay, int32_t K, int32_t S, int32_t ceil_mode, int64_t* out_lens,
                               int64_t* own_lens, void* stream) {
  using namespace rua;
  int e;
  if ((e = seg_check_entry(lay, 1, 1)) != 0) return e;
  if ((e = wp_check_window(K, S)) != 0) return e;
  if (lay->B == 0) return 0;
  if (!out_lens || out_lens == own_lens) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)out_lens % 8 || (uint64_t)(uintptr_t)own_lens % 8) return RUA_EALIGN;
  const int64_t grid = (lay->B - 1) / RUA_BLOCK + 1;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_window_lens_kernel K=%d S=%d ceil=%d kind=%d B=%lld", (int)K, (int)S, ceil_mode ? 1 : 0, lay->kind,
            (long long)lay->B);
  hipLaunchKernelGGL(seg_window_lens_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *lay, (int)K,
                     (int64_t)S, ceil_mode ? 1 : 0, out_lens, own_lens);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_window_pool(const rua_layout* src_lay, const rua_layout* dst_lay, const void* data, void* out,
                                       uint8_t* arg, int64_t H, int32_t K, int32_t S, int32_t mode, int32_t dtype,
                                       void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, true);
  int e;
  if ((e = wp_check_entry(dst_lay, src_lay, H, K, S, mode, dtype, es)) != 0) return e;
  if (dst_lay->B == 0 || dst_lay->n_rows == 0 || H == 0) return 0;
  if (!out || (src_lay->n_rows > 0 && !data) || (mode == RUA_WINDOW_TAKE && !arg)) return RUA_EINVAL;
  if (out == data || (arg && ((const void*)arg == data || (const void*)arg == out))) return RUA_EINVAL;
  if (seg_too_large(src_lay, H, es) || seg_too_large(dst_lay, H, es)) return RUA_ERANGE;
  return wp_dispatch<false>(src_lay, src_lay, dst_lay, data, out, arg, H, K, S, mode, dtype, stream);
}

extern "C" int rua_segment_window_spread(const rua_layout* pooled_lay, const rua_layout* big_lay, const void* grad_out,
                                         const uint8_t* arg, void* grad_in, int64_t H, int32_t K, int32_t S, int32_t mode,
                                         int32_t dtype, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, true);
  int e;
  if ((e = wp_check_entry(pooled_lay, big_lay, H, K, S, mode, dtype, es)) != 0) return e;
  if (big_lay->B == 0 || big_lay->n_rows == 0 || H == 0) return 0;
  const bool by_arg = mode == RUA_MAX || mode == RUA_WINDOW_TAKE;
  if (!grad_in || (pooled_lay->n_rows > 0 && (!grad_out || (by_arg && !arg)))) return RUA_EINVAL;
  if (grad_in == grad_out || (arg && ((const void*)arg == grad_out || (const void*)arg == grad_in))) return RUA_EINVAL;
  if (seg_too_large(big_lay, H, es) || seg_too_large(pooled_lay, H, es)) return RUA_ERANGE;
  return wp_dispatch<true>(big_lay, pooled_lay, big_lay, grad_out, grad_in, arg, H, K, S, mode, dtype, stream);
}
