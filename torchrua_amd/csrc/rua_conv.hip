// rua_conv.hip — per-sequence causal depthwise convolution over the tokens of a C / L / P / R container
// (rua_segment_causal_conv, rua_segment_causal_conv_backward; include/rua.h).  An extension: the short convolution
// that sits next to the state update of diagonal linear RNNs and SSMs (rua_linear_scan.hip).  Without it a ragged batch
// pads (`left()`), transposes, calls a grouped conv1d, slices, transposes and casts back.
//
// With u the position along the walk (u = t, or u = len - 1 - t for `reverse`), per sequence and column h:
//   y[u] = bias[h] + sum_{k = 0 .. K-1, u - (K-1) + k >= 0}  weight[k,h] * x[u - (K-1) + k]
// weight[K-1] multiplies the current token.  A tap that falls outside the sequence is NOT EVALUATED (no 0 * weight): a
// non-finite weight does not poison the first K - 1 tokens.
//
// ONE evaluation order per (token, column), whatever the layout, kernel form, alignment or block boundary: the
// accumulator starts at the bias (+0 without one), the taps that exist are added in ascending k with an explicit fused
// multiply-add in the accumulator type (fp32; fp64 for RUA_F64), and the result is rounded once.  The value about to be
// rounded is made opaque to the optimiser (cv_pin), so that no form folds the last fma and the conversion into one
// mixed-precision instruction (as rua_linear_scan.hip had to for f16).  Nothing is folded across tokens, so blocks,
// runs and tiles change no bit.
//
// The backward walks the other way: grad_in is the same convolution of grad_out with `reverse` flipped, and with
// u' the position of that walk  grad_weight[k,h] = sum x[u'] * g[u' - (K-1) + k]  (the window of g the walk holds anyway)
// and grad_bias[h] = sum g[u'].  A workgroup keeps these sums in registers over all the units it walks, folds them over
// its threads in a fixed tree and leaves ONE partial per (part, chunk) in the workspace; a finish launch adds the parts
// in part order.  No float atomics: the sums are bitwise reproducible for the same container.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <initializer_list>
#include <type_traits>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int CV_SLOTS = 32;               // rows form: contiguous runs of tokens per workgroup; lanes form: tokens of a tile
constexpr int CV_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int CV_UNR = 4;                  // rows form: tokens in flight per thread
constexpr int64_t CV_MAX_PARTS = 1024;     // partial sums per chunk the backward leaves in its workspace, at most
static_assert(RUA_CONV_MAX_TAPS == 8, "the dispatch below instantiates K = 1 .. 8");
static_assert(CV_SLOTS * CV_LPR == RUA_BLOCK, "a thread per (run, 16-byte lane of the chunk)");

__device__ __forceinline__ float cv_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double cv_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// a value about to be rounded to the payload dtype, opaque to the optimiser (see the head of this file)
template <typename A> __device__ __forceinline__ A cv_pin(A v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup per unit and 128-byte column chunk; a unit is a sequence, or (maxblk > 0: few but long sequences) a block
// of SEG_BLOCK_TOK tokens of one.  The tokens of the unit are split into CV_SLOTS contiguous runs; thread (q, l) =
// (tid / 8, tid % 8) walks run q and owns the l-th 16-byte vector of the chunk.  It keeps the previous K - 1 vectors,
// the chunk's K weight vectors and the bias in registers: every row is read once (plus K - 1 rows in front of a run,
// lines the neighbouring thread loads anyway) and written once.  No LDS for the payload.
// Part `blockIdx.x / n_chunks` walks the units part, part + parts, ...: the forward has a part per unit; WG (the
// backward that wants grad_weight / grad_bias) has at most CV_MAX_PARTS and sums over its units in registers.
// `sync`: out == xin — the rows in front of a run are loaded before any thread of the workgroup stores.
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.  `walign`: weight and bias sit
// on 16 bytes (checked apart: they are small tensors of their own).
template <typename E, int K, bool AL, bool WG>
__global__ __launch_bounds__(RUA_BLOCK) void seg_conv_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                  const typename E::raw* pin,
                                                                  const typename E::raw* weight,
                                                                  const typename E::raw* bias, typename E::raw* out,
                                                                  int64_t H, int n_chunks, int maxblk, int64_t units,
                                                                  int parts, typename E::acc* ws, int rev, int sync,
                                                                  int walign) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = CV_LPR * VE;
  constexpr int U = CV_UNR;
  constexpr int NS = (K + 1) * VE;                            // sums a thread keeps (WG)
  __shared__ A red[WG ? RUA_WAVES_PER_BLOCK * CV_LPR * NS : 1];
  struct alignas(16) Vec { raw e[VE]; };

  const int tid = threadIdx.x;
  const int l = tid & (CV_LPR - 1), q = tid >> 3;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  const int64_t part = blockIdx.x / (unsigned)n_chunks;
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;

  auto ld = [&](const raw* src, int64_t row, Vec& v) {
    const raw* p = src + row * H + col0;
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

  // the chunk's K weight vectors and the bias: one 16-byte load each where the rows and `walign` (their bases) allow
  auto small = [&](const raw* src, A* dst) {
    Vec v;
#pragma unroll
    for (int e = 0; e < VE; ++e) v.e[e] = (raw)0;
    if (src && active) {
      if (AL && walign) {
        v = *(const Vec*)(src + col0);
      } else {
#pragma unroll
        for (int e = 0; e < VE; ++e) if (e < nval) v.e[e] = src[col0 + e];
      }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) dst[e] = E::up(v.e[e]);
  };
  A wv[K][VE], bv[VE], gw[WG ? K : 1][VE], gb[VE];
  small(bias, bv);
#pragma unroll
  for (int k = 0; k < K; ++k) small(weight ? weight + (int64_t)k * H : nullptr, wv[k]);
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    gb[e] = (A)0;
#pragma unroll
    for (int k = 0; k < (WG ? K : 1); ++k) gw[k][e] = (A)0;
  }

  for (int64_t unit = part; unit < units; unit += parts) {
    int64_t b = unit;
    int blk = 0;
    if (maxblk > 0) { blk = (int)(unit % maxblk); b = unit / maxblk; }
    const int64_t len = safe_len(L, b);
    int64_t tb, te;
    seg_block_range(maxblk, blk, len, tb, te);
    const int64_t run = (te - tb + CV_SLOTS - 1) / CV_SLOTS;
    const int64_t s = tb + (int64_t)q * run < te ? tb + (int64_t)q * run : te;
    const int64_t se = s + run < te ? s + run : te;

    // X[j] holds position u0 - (K-1) + j of the walk: the K - 1 rows in front of the group, then its U rows
    A X[K - 1 + U][VE];
#pragma unroll
    for (int j = 0; j < K - 1; ++j) {
      const int64_t pos = s - (K - 1) + j;
      Vec v;
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = (raw)0;
      if (active && s < se && pos >= 0) {
        const int64_t row = token_to_row(L, b, rev ? len - 1 - pos : pos, len);
        if (row >= 0 && row < L.n_rows) ld(xin, row, v);
      }
#pragma unroll
      for (int e = 0; e < VE; ++e) X[j][e] = E::up(v.e[e]);
    }
    if (sync) __syncthreads();                                // (workgroup-uniform: `units` and `parts` are)

    for (int64_t u0 = s; u0 < se; u0 += U) {
      Vec xr[U], pr[U];
      int64_t rows[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int64_t u = u0 + i;
        rows[i] = -1;
#pragma unroll
        for (int e = 0; e < VE; ++e) { xr[i].e[e] = (raw)0; pr[i].e[e] = (raw)0; }
        if (active && u < se) {
          const int64_t row = token_to_row(L, b, rev ? len - 1 - u : u, len);
          if (row >= 0 && row < L.n_rows) {
            rows[i] = row;
            ld(xin, row, xr[i]);
            if constexpr (WG) { if (pin) ld(pin, row, pr[i]); }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
#pragma unroll
        for (int e = 0; e < VE; ++e) X[K - 1 + i][e] = E::up(xr[i].e[e]);
      }
      // taps in front of the sequence exist for no token of a group that starts at K - 1 or later
      auto group = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int i = 0; i < U; ++i) {
          if (rows[i] < 0) continue;
          const int64_t first = (K - 1) - (u0 + i);           // taps k < first do not exist
          if (out) {
            A acc[VE];
#pragma unroll
            for (int e = 0; e < VE; ++e) acc[e] = bv[e];
#pragma unroll
            for (int k = 0; k < K; ++k) {
              if (FULL || k >= first) {
#pragma unroll
                for (int e = 0; e < VE; ++e) acc[e] = cv_fma(wv[k][e], X[i + k][e], acc[e]);
              }
            }
            Vec o;
#pragma unroll
            for (int e = 0; e < VE; ++e) o.e[e] = E::down(cv_pin(acc[e]));
            st(rows[i], o);
          }
          if constexpr (WG) {
#pragma unroll
            for (int e = 0; e < VE; ++e) gb[e] = gb[e] + X[K - 1 + i][e];
            if (pin) {
#pragma unroll
              for (int k = 0; k < K; ++k) {
                if (FULL || k >= first) {
#pragma unroll
                  for (int e = 0; e < VE; ++e) gw[k][e] = cv_fma(E::up(pr[i].e[e]), X[i + k][e], gw[k][e]);
                }
              }
            }
          }
        }
      };
      if (u0 >= K - 1) group(std::true_type{}); else group(std::false_type{});
#pragma unroll
      for (int j = 0; j < K - 1; ++j) {
#pragma unroll
        for (int e = 0; e < VE; ++e) X[j][e] = X[j + U][e];
      }
    }

    if (out && active && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
      Vec z;
#pragma unroll
      for (int e = 0; e < VE; ++e) z.e[e] = (raw)0;
      for (int64_t j = q; j < L.T_phys; j += CV_SLOTS) {
        if (!is_pad(L, j, len)) continue;
        const int64_t row = b * L.T_phys + j;
        if (row < L.n_rows) st(row, z);
      }
    }
  }

  if constexpr (WG) {
    // the 8 runs of a wave (xor 8, 16, 32 of the lane number), then the 4 waves through LDS in wave order
    const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
#pragma unroll
    for (int m = CV_LPR; m < RUA_WAVE; m <<= 1) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        gb[e] = gb[e] + seg_shfl_xor(gb[e], m);
#pragma unroll
        for (int k = 0; k < K; ++k) gw[k][e] = gw[k][e] + seg_shfl_xor(gw[k][e], m);
      }
    }
    if (lane < CV_LPR) {
      A* r = red + (w * CV_LPR + l) * NS;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
#pragma unroll
        for (int k = 0; k < K; ++k) r[k * VE + e] = gw[k][e];
        r[K * VE + e] = gb[e];
      }
    }
    __syncthreads();
    if (tid < CV_LPR) {
      // ws[part][chunk][k = 0 .. K (K: the bias)][CW]
      A* pw = ws + ((part * n_chunks + c) * (K + 1)) * CW + l * VE;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        A sum = red[(0 * CV_LPR + l) * NS + i];
#pragma unroll
        for (int ww = 1; ww < RUA_WAVES_PER_BLOCK; ++ww) sum = sum + red[(ww * CV_LPR + l) * NS + i];
        pw[(i / VE) * CW + (i % VE)] = sum;
      }
    }
  }
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// The family's lanes geometry: a wave takes two sequences, 32 lanes each; lane r of a half is position r of a tile of
// CV_SLOTS positions.  The K - 1 rows before a position come from the lanes below by shuffle, or — the first lanes of a
// tile — from the previous tile, which the half wave keeps in registers: every row is loaded once, so `out` may be
// the payload itself.  Workgroup g walks the groups of 8 sequences g, g + gridDim.x, ... (WG: at most CV_MAX_PARTS
// workgroups; otherwise one group each).
template <typename E, int K, bool WG>
__global__ __launch_bounds__(RUA_BLOCK) void seg_conv_lanes_kernel(rua_layout L, const char* xin, const char* pin,
                                                                   const typename E::raw* weight,
                                                                   const typename E::raw* bias, char* out, int H, int W,
                                                                   int64_t groups, typename E::acc* ws, int rev) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = CV_LPR * VE;
  constexpr int NS = (K + 1) * VE;
  __shared__ A red[WG ? RUA_WAVES_PER_BLOCK * NS : 1];
  union alignas(16) Row { raw e[VE]; uint32_t d[4]; };

  const int tid = threadIdx.x;
  const int lane = tid & (RUA_WAVE - 1), w = tid >> 6;
  const int q = lane & (CV_SLOTS - 1);
  const int nb = H * (int)sizeof(raw);

  A wv[K][VE], bv[VE], gw[WG ? K : 1][VE], gb[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    bv[e] = (bias && e < H) ? E::up(bias[e]) : (A)0;
    gb[e] = (A)0;
#pragma unroll
    for (int k = 0; k < K; ++k) wv[k][e] = (weight && e < H) ? E::up(weight[k * H + e]) : (A)0;
#pragma unroll
    for (int k = 0; k < (WG ? K : 1); ++k) gw[k][e] = (A)0;
  }

  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t b = (g * RUA_WAVES_PER_BLOCK + w) * 2 + (lane >> 5);
    const bool have = b < L.B;
    const int64_t len = have ? safe_len(L, b) : 0;
    const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
    const int64_t maxlen = len > other ? len : other;        // wave-uniform
    Row prev;
#pragma unroll
    for (int i = 0; i < 4; ++i) prev.d[i] = 0u;

    for (int64_t u0 = 0; u0 < maxlen; u0 += CV_SLOTS) {
      const int64_t u = u0 + q;
      Row cur, pc;
#pragma unroll
      for (int i = 0; i < 4; ++i) { cur.d[i] = 0u; pc.d[i] = 0u; }
      int64_t row = -1;
      if (u < len) {
        row = token_to_row(L, b, rev ? len - 1 - u : u, len);
        if (row >= 0 && row < L.n_rows) {
          ld_row_w(xin + row * nb, nb, W, &cur);
          if constexpr (WG) { if (pin) ld_row_w(pin + row * nb, nb, W, &pc); }
        } else {
          row = -1;
        }
      }
      A acc[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[e] = bv[e];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = K - 1 - k;                             // the tap reads position u - j
        Row v = cur;
        if (j > 0) {
          // lane s hands its row of this tile to lane s + j, or — the last j lanes — its row of the previous tile to
          // lane s + j - 32 of this one
#pragma unroll
          for (int i = 0; i < 4; ++i) v.d[i] = __shfl(q < CV_SLOTS - j ? cur.d[i] : prev.d[i], (q - j) & (CV_SLOTS - 1), CV_SLOTS);
        }
        if (row >= 0 && u - j >= 0) {
#pragma unroll
          for (int e = 0; e < VE; ++e) {
            if (e >= H) continue;
            const A xv = E::up(v.e[e]);
            if (out) acc[e] = cv_fma(wv[k][e], xv, acc[e]);
            if constexpr (WG) { if (pin) gw[k][e] = cv_fma(E::up(pc.e[e]), xv, gw[k][e]); }
          }
        }
      }
      if (row >= 0) {
        if constexpr (WG) {
#pragma unroll
          for (int e = 0; e < VE; ++e) if (e < H) gb[e] = gb[e] + E::up(cur.e[e]);
        }
        if (out) {
          Row o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o.d[i] = 0u;
#pragma unroll
          for (int e = 0; e < VE; ++e) if (e < H) o.e[e] = E::down(cv_pin(acc[e]));
          st_row_w(out + row * nb, nb, W, &o);
        }
      }
      prev = cur;
    }
    if (out && have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
      Row z;
#pragma unroll
      for (int i = 0; i < 4; ++i) z.d[i] = 0u;
      for (int64_t j = q; j < L.T_phys; j += CV_SLOTS) {
        if (!is_pad(L, j, len)) continue;
        const int64_t row = b * L.T_phys + j;
        if (row < L.n_rows) st_row_w(out + row * nb, nb, W, &z);
      }
    }
  }

  if constexpr (WG) {
    // the 64 lanes of a wave by a butterfly, then the 4 waves through LDS in wave order
#pragma unroll
    for (int m = 1; m < RUA_WAVE; m <<= 1) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        gb[e] = gb[e] + seg_shfl_xor(gb[e], m);
#pragma unroll
        for (int k = 0; k < K; ++k) gw[k][e] = gw[k][e] + seg_shfl_xor(gw[k][e], m);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[w * NS + k * VE + e] = gw[k][e];
        red[w * NS + K * VE + e] = gb[e];
      }
    }
    __syncthreads();
    if (tid < NS) {
      A sum = red[tid];
#pragma unroll
      for (int ww = 1; ww < RUA_WAVES_PER_BLOCK; ++ww) sum = sum + red[ww * NS + tid];
      // ws[part][chunk 0][k = 0 .. K][CW]
      ws[((int64_t)blockIdx.x * (K + 1) + tid / VE) * CW + tid % VE] = sum;
    }
  }
}

// ---------------------------------------------------------------- the finish: the parts, in part order
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_conv_finish_kernel(const typename E::acc* ws, typename E::raw* gw,
                                                                    typename E::raw* gb, int64_t H, int K, int n_chunks,
                                                                    int parts) {
  using A = typename E::acc;
  constexpr int CW = CV_LPR * (16 / (int)sizeof(typename E::raw));
  const int64_t i = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (i >= (int64_t)(K + 1) * H) return;
  const int64_t k = i / H, h = i - k * H;
  const int64_t c = h / CW, col = h - c * CW;
  A sum = (A)0;
  for (int64_t p = 0; p < parts; ++p) sum = sum + ws[((p * n_chunks + c) * (K + 1) + k) * CW + col];
  if (k < K) {
    if (gw) gw[k * H + h] = E::down(sum);
  } else if (gb) {
    gb[h] = E::down(sum);
  }
}

// ---------------------------------------------------------------- host side
struct cv_plan {
  seg_plan seg;       // n_chunks and the cut rule of the family (no workspace of its own)
  bool lanes;         // rows of one vector
  int64_t units;      // rows form: sequences, or (sequence, block) when cut; lanes form: groups of 8 sequences
  int parts;          // partial sums per chunk of the backward: min(units, CV_MAX_PARTS)
};

static cv_plan cv_make_plan(const rua_layout& L, int64_t H, int es) {
  cv_plan p = {seg_make_plan(L, H, es, 0), false, 0, 0};
  if (!es || H <= 0 || L.B <= 0 || p.seg.n_chunks <= 0) return p;
  p.lanes = H * es <= 16;
  if (p.lanes) p.units = ((L.B + 1) / 2 + SEG_WAVES_PER_BLOCK - 1) / SEG_WAVES_PER_BLOCK;
  else p.units = L.B * (int64_t)(p.seg.maxblk > 0 ? p.seg.maxblk : 1);
  p.parts = (int)(p.units < CV_MAX_PARTS ? p.units : CV_MAX_PARTS);
  return p;
}

static int64_t cv_ws_bytes(const cv_plan& p, int es, int K) {
  return (int64_t)p.parts * p.seg.n_chunks * (128 / es) * (K + 1) * (es == 8 ? 8 : 4);
}

// xin: what the walk convolves (data, or grad_out in the backward); pin / gw / gb: the backward's sums (WG)
template <typename E, int K, bool WG>
static int cv_launch_k(const rua_layout& L, const void* xin, const void* pin, const void* weight, const void* bias,
                       void* out, void* gw, void* gb, int64_t H, int rev, void* ws, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  const int es = (int)sizeof(raw);
  const int64_t row_bytes = H * es;
  const uint64_t bases = (uint64_t)(uintptr_t)xin | (uint64_t)(uintptr_t)pin | (uint64_t)(uintptr_t)out;
  const uint64_t small = (uint64_t)(uintptr_t)weight | (uint64_t)(uintptr_t)bias | (uint64_t)(uintptr_t)gw |
                         (uint64_t)(uintptr_t)gb;
  if ((bases | small) % sizeof(raw) || (uint64_t)(uintptr_t)ws % sizeof(A)) return RUA_EALIGN;
  const cv_plan p = cv_make_plan(L, H, es);
  if (p.seg.n_chunks <= 0 || p.units <= 0) return RUA_ERANGE;

  if (p.lanes) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    const int64_t grid = WG ? p.parts : p.units;
    seg_trace("seg_conv_lanes_kernel T=%s K=%d W=%d H=%d rev=%d kind=%d bwd=%d cut=0 parts=%d", E::name(), K, ln.W,
              (int)H, rev, L.kind, (int)WG, WG ? p.parts : 0);
    hipLaunchKernelGGL((seg_conv_lanes_kernel<E, K, WG>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L,
                       (const char*)xin, (const char*)pin, (const raw*)weight, (const raw*)bias, (char*)out, (int)H,
                       ln.W, p.units, (A*)ws, rev);
  } else {
    // a cut block reads K - 1 rows of the block before it, which another workgroup writes: in place (the forward
    // only; the backward refuses grad_in == grad_out) a sequence stays with one workgroup
    const bool inplace = out && out == xin;
    const bool cut = p.seg.maxblk > 0 && !inplace;
    const int64_t units = cut ? p.units : L.B;
    const int64_t parts = WG ? p.parts : units;
    const int64_t grid = parts * p.seg.n_chunks;
    if (grid > 0x7fffffffLL) return RUA_ERANGE;
    const bool al = row_bytes % 16 == 0 && bases % 16 == 0;
    seg_trace("seg_conv_rows_kernel T=%s K=%d AL=%d rev=%d kind=%d bwd=%d cut=%d blocks=%d chunks=%d parts=%d", E::name(),
              K, (int)al, rev, L.kind, (int)WG, (int)cut, cut ? p.seg.maxblk : 0, p.seg.n_chunks, WG ? (int)parts : 0);
    seg_with_al(al, [&](auto AL) {
      hipLaunchKernelGGL((seg_conv_rows_kernel<E, K, decltype(AL)::value, WG>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0,
                         s, L, (const raw*)xin, (const raw*)pin, (const raw*)weight, (const raw*)bias, (raw*)out, H,
                         p.seg.n_chunks, cut ? p.seg.maxblk : 0, units, (int)parts, (A*)ws, rev, (int)inplace,
                         (int)(small % 16 == 0));
    });
  }
  int e = (int)hipGetLastError();
  if (e || !WG) return e;
  const int64_t n_out = (int64_t)(K + 1) * H;
  seg_trace("seg_conv_finish_kernel T=%s K=%d parts=%d chunks=%d", E::name(), K, p.parts, p.seg.n_chunks);
  hipLaunchKernelGGL((seg_conv_finish_kernel<E>), dim3((unsigned)((n_out + RUA_BLOCK - 1) / RUA_BLOCK)), dim3(RUA_BLOCK),
                     0, s, (const A*)ws, (raw*)gw, (raw*)gb, H, K, p.seg.n_chunks, p.parts);
  return (int)hipGetLastError();
}

template <typename E, bool WG>
static int cv_launch(const rua_layout& L, const void* xin, const void* pin, const void* weight, const void* bias,
                     void* out, void* gw, void* gb, int64_t H, int K, int rev, void* ws, hipStream_t s) {
  switch (K) {
#define RUA_CV_K(KV) case KV: return cv_launch_k<E, KV, WG>(L, xin, pin, weight, bias, out, gw, gb, H, rev, ws, s)
    RUA_CV_K(1); RUA_CV_K(2); RUA_CV_K(3); RUA_CV_K(4); RUA_CV_K(5); RUA_CV_K(6); RUA_CV_K(7); RUA_CV_K(8);
#undef RUA_CV_K
  }
  return RUA_EINVAL;
}

template <bool WG>
static int cv_dispatch(const rua_layout* lay, const void* xin, const void* pin, const void* weight, const void* bias,
                       void* out, void* gw, void* gb, int64_t H, int32_t K, int32_t dtype, int rev, void* ws,
                       void* stream) {
#define RUA_CV(E) cv_launch<E, WG>(*lay, xin, pin, weight, bias, out, gw, gb, H, K, rev, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_CV);
#undef RUA_CV
}

// the layout, then H, the dtype and K
static int cv_check_entry(const rua_layout* lay, int64_t H, int32_t K, int es) {
  const int e = seg_check_entry(lay, H, es);
  if (e != 0) return e;
  if (K < 1) return RUA_EINVAL;
  return K > RUA_CONV_MAX_TAPS ? RUA_ERANGE : 0;
}

}  // namespace rua

extern "C" int64_t rua_causal_conv_ws_bytes(const rua_layout* lay, int64_t H, int32_t K, int32_t dtype) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  if (cv_check_entry(lay, H, K, es) != 0) return 0;
  const cv_plan p = cv_make_plan(*lay, H, es);
  return p.parts > 0 ? cv_ws_bytes(p, es, K) : 0;
}

extern "C" int rua_segment_causal_conv(const rua_layout* lay, const void* data, const void* weight, const void* bias,
                                       void* out, int64_t H, int32_t K, int32_t dtype, int32_t reverse, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = cv_check_entry(lay, H, K, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!data || !weight || !out) return RUA_EINVAL;
  if (out == weight || out == bias) return RUA_EINVAL;
  if (seg_too_large(lay, H, es)) return RUA_ERANGE;
  return cv_dispatch<false>(lay, data, nullptr, weight, bias, out, nullptr, nullptr, H, K, dtype, reverse ? 1 : 0,
                            nullptr, stream);
}

extern "C" int rua_segment_causal_conv_backward(const rua_layout* lay, const void* grad_out, const void* data,
                                                const void* weight, void* grad_in, void* grad_weight, void* grad_bias,
                                                int64_t H, int32_t K, int32_t dtype, int32_t reverse, void* ws,
                                                void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = cv_check_entry(lay, H, K, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!grad_in && !grad_weight && !grad_bias) return 0;
  if (!grad_out || (grad_in && !weight) || (grad_weight && !data)) return RUA_EINVAL;
  if (grad_in && (grad_in == grad_out || grad_in == data || grad_in == weight)) return RUA_EINVAL;
  for (const void* o : {(const void*)grad_weight, (const void*)grad_bias}) {
    if (o && (o == grad_out || o == data || o == weight || o == grad_in)) return RUA_EINVAL;
  }
  if (grad_weight && grad_weight == grad_bias) return RUA_EINVAL;
  if (seg_too_large(lay, H, es)) return RUA_ERANGE;
  // the backward walks the other way
  const int rev = reverse ? 0 : 1;
  if (!grad_weight && !grad_bias)
    return cv_dispatch<false>(lay, grad_out, nullptr, weight, nullptr, grad_in, nullptr, nullptr, H, K, dtype, rev,
                              nullptr, stream);
  if (!ws) return RUA_EINVAL;
  return cv_dispatch<true>(lay, grad_out, grad_weight ? data : nullptr, grad_in ? weight : nullptr, nullptr, grad_in,
                           grad_weight, grad_bias, H, K, dtype, rev, ws, stream);
}
