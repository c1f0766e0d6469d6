// rua_argreduce.hip — per-sequence argmax / argmin over the tokens of a C / L / P / R container, with the selected
// values, and the two row operators their autograd is made of (rua_segment_argreduce, rua_segment_take,
// rua_segment_put; include/rua.h).  An extension: the reference has no position-returning reduction; its users pad
// (`left(fill_value=-inf)`), call torch.argmax along dim 1 — a copy of the payload plus the padding, a wrong answer for a
// sequence that holds only -inf, and nothing at all for a PackedSequence.
//
// index[b,h] is the token position t in [0, len[b]) — not a storage row, so it is the same number in every layout — of
// the largest (smallest) element of column h of sequence b; -1 for an empty sequence, whose value is the identity
// (-inf / +inf, INT64_MIN / INT64_MAX).  The order on (value, position) is TOTAL:
//   - a NaN beats every number, for max AND for min;
//   - otherwise the greater (smaller) value wins, +0.0 == -0.0;
//   - between equals (two NaNs included) the smaller position wins; "no token" (-1) loses against every token.
// A fold over a total order is associative and commutative: every kernel form, launch geometry, alignment and `ws`
// gives the same bits, so nothing below has to keep a fold order.  These are torch.max(seq, dim=0) / torch.min of every
// sequence on its own (CPU torch).  bf16 / f16 compare after the exact widening to fp32.
//
// Forms, chosen as rua_softmax.hip chooses its own: LANES (rows of one vector: consecutive tokens on consecutive lanes,
// two sequences per wave), ROWS (a workgroup per sequence x 128-byte column chunk, 32 rows x 4 in flight, combined through
// LDS) and CUT (the blocks of few but long sequences on different workgroups, partial (value, position) pairs in `ws`,
// a finish launch).  A thread tracks a 32-bit offset inside a block of 2 048 tokens and a 64-bit block base.
// Padding rows of a LEFT / RIGHT input are never read; lengths are clamped to the storage and every row is range-checked.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

namespace rua {

constexpr int AR_SLOTS = 32;               // tokens a step of a sequence puts side by side
constexpr int AR_BLOCK_TOK = SEG_BLOCK_TOK; // tokens per block: 32-bit offsets inside, a 64-bit base outside
constexpr int AR_LPR = 8;                  // rows form: 16-byte lanes per row chunk (128 bytes)
constexpr int AR_ROWS_UNR = 4;             // rows form: rows in flight per thread
constexpr int AR_LANES_UNR = 8;            // lanes form: tokens in flight per lane
static_assert(AR_SLOTS * AR_LPR == RUA_BLOCK, "a step of the rows form is a workgroup");

// ---------------------------------------------------------------- element types
struct ar_i64 {
  using raw = int64_t; using acc = int64_t;
  static __device__ __forceinline__ acc up(raw v) { return v; }
  static __device__ __forceinline__ raw down(acc v) { return v; }
  static const char* name() { return "i64"; }
};

template <typename A, int OP> __device__ __forceinline__ A ar_ident();
template <> __device__ __forceinline__ float ar_ident<float, RUA_MAX>() { return -__builtin_inff(); }
template <> __device__ __forceinline__ float ar_ident<float, RUA_MIN>() { return __builtin_inff(); }
template <> __device__ __forceinline__ double ar_ident<double, RUA_MAX>() { return -__builtin_inf(); }
template <> __device__ __forceinline__ double ar_ident<double, RUA_MIN>() { return __builtin_inf(); }
template <> __device__ __forceinline__ int64_t ar_ident<int64_t, RUA_MAX>() { return INT64_MIN; }
template <> __device__ __forceinline__ int64_t ar_ident<int64_t, RUA_MIN>() { return INT64_MAX; }

// ---------------------------------------------------------------- the order
// does (v, i) come before (bv, bi)?  Positions compare UNSIGNED: "no token" (-1, or ~0 as an offset) is the largest.
template <int OP, typename A, typename I>
__device__ __forceinline__ bool ar_better(A v, I i, A bv, I bi) {
  const bool vn = v != v, bn = bv != bv;                      // (integers: constant false)
  if (vn || bn) return vn && (!bn || i < bi);
  const bool gt = OP == RUA_MAX ? v > bv : v < bv;
  return gt || (v == bv && i < bi);
}
template <int OP, typename A>
__device__ __forceinline__ void ar_merge(A& V, int64_t& I, A v, int64_t i) {
  if (ar_better<OP>(v, (uint64_t)i, V, (uint64_t)I)) { V = v; I = i; }
}
// a block's (value, offset) joins the running (value, position)
template <int OP, typename A>
__device__ __forceinline__ void ar_merge_block(A& V, int64_t& I, A v, uint32_t o, int64_t t0) {
  if (o != 0xffffffffu) ar_merge<OP>(V, I, v, t0 + (int64_t)o);
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// A wave takes two sequences, 32 lanes each: consecutive lanes take consecutive tokens (one contiguous run of whole
// lines for CAT), eight tokens in flight per lane; the 32 lanes are combined by a butterfly of shuffles.
template <typename E, int OP>
__global__ __launch_bounds__(RUA_BLOCK) void seg_argreduce_lanes_kernel(rua_layout L, const char* xin,
                                                                        typename E::raw* vout, int64_t* iout, int H,
                                                                        int W) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = AR_LANES_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (AR_SLOTS - 1);
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);

  struct alignas(16) Row { raw e[VE]; };
  A V[VE];
  int64_t I[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { V[e] = ar_ident<A, OP>(); I[e] = -1; }

  for (int64_t t0 = 0; t0 < maxlen; t0 += AR_BLOCK_TOK) {
    A v[VE];
    uint32_t o[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) { v[e] = ar_ident<A, OP>(); o[e] = 0xffffffffu; }
    const int64_t t1 = len < t0 + AR_BLOCK_TOK ? len : t0 + AR_BLOCK_TOK;
    const int64_t t1w = maxlen < t0 + AR_BLOCK_TOK ? maxlen : t0 + AR_BLOCK_TOK;
    for (int64_t tt = t0; tt < t1w; tt += (int64_t)AR_SLOTS * UNR) {
      Row x[UNR];
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t t = tt + (int64_t)u * AR_SLOTS + q;
        ok[u] = false;
        if (t < t1) {
          const int64_t row = token_to_row(L, b, t, len);
          if (row >= 0 && row < L.n_rows) {
            ok[u] = true;
            ld_row_w(xin + row * nb, nb, W, &x[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (!ok[u]) continue;
        const uint32_t off = (uint32_t)(tt - t0) + (uint32_t)(u * AR_SLOTS + q);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          const A a = E::up(x[u].e[e]);
          if (ar_better<OP>(a, off, v[e], o[e])) { v[e] = a; o[e] = off; }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) ar_merge_block<OP>(V[e], I[e], v[e], o[e], t0);
  }
#pragma unroll
  for (int k = 1; k < AR_SLOTS; k <<= 1) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (e >= H) continue;
      const A v2 = __shfl_xor(V[e], k, RUA_WAVE);
      const int64_t i2 = __shfl_xor(I[e], k, RUA_WAVE);
      ar_merge<OP>(V[e], I[e], v2, i2);
    }
  }
  if (have && q == 0) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (e >= H) continue;
      iout[b * H + e] = I[e];
      if (vout) vout[b * H + e] = E::down(V[e]);
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup takes (sequence x 128-byte column chunk): thread (q, l) = (tid / 8, tid % 8) takes the tokens t = q
// (mod 32), four of them in flight, and owns the l-th 16-byte vector of the chunk.  The 32 threads of a vector are
// combined by shuffles inside a wave (lanes 8, 16, 32 apart) and through LDS across the four waves.
// mode SEG_PARTIAL: the CUT form — a workgroup per (sequence, block of 2 048 tokens, chunk) leaves its block's (value,
// position) in `ws`; SEG_FINISH: a workgroup per (sequence, chunk) combines the pairs of the sequence's blocks.
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.
template <typename E, int OP, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_argreduce_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                       typename E::raw* vout, int64_t* iout, int64_t H,
                                                                       int n_chunks, int mode, int maxblk, char* ws) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = AR_LPR * VE;
  constexpr int UNR = AR_ROWS_UNR;
  __shared__ A xv[RUA_WAVES_PER_BLOCK][AR_LPR][VE];
  __shared__ int64_t xi[RUA_WAVES_PER_BLOCK][AR_LPR][VE];
  struct alignas(16) Vec { raw e[VE]; };

  const int tid = threadIdx.x;
  const int l = tid & (AR_LPR - 1), q = tid >> 3, w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode == SEG_PARTIAL) { blk = (int)(b % maxblk); b /= maxblk; }
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: a CAT layout whose T_log understates a length
  // must not walk past the maxblk blocks that exist (rua.h: T_log has to be a true bound)
  const int64_t have_blk = (len + AR_BLOCK_TOK - 1) / AR_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode == SEG_PARTIAL && blk > 0 && blk >= nblk) return;    // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  int64_t tb = 0, te = len;
  if (mode == SEG_PARTIAL) {
    tb = (int64_t)blk * AR_BLOCK_TOK;
    te = len < tb + AR_BLOCK_TOK ? len : tb + AR_BLOCK_TOK;
    if (tb > te) tb = te;
  }
  // `ws`: the positions of every (sequence, block, chunk, lane, element), then the values
  const int64_t ws_elems = L.B * (int64_t)maxblk * n_chunks * CW;
  int64_t* wsi = (int64_t*)ws;
  A* wsv = (A*)(ws + ws_elems * 8);

  A V[VE];
  int64_t I[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { V[e] = ar_ident<A, OP>(); I[e] = -1; }

  if (mode == SEG_FINISH) {
    if (active) {
      for (int64_t k = q; k < nblk; k += AR_SLOTS) {
        const int64_t at = (((b * maxblk + k) * n_chunks + c) * AR_LPR + l) * VE;
#pragma unroll
        for (int e = 0; e < VE; ++e) ar_merge<OP>(V[e], I[e], wsv[at + e], wsi[at + e]);
      }
    }
  } else if (active) {
    for (int64_t t0 = tb; t0 < te; t0 += AR_BLOCK_TOK) {
      A v[VE];
      uint32_t o[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) { v[e] = ar_ident<A, OP>(); o[e] = 0xffffffffu; }
      const int64_t t1 = te < t0 + AR_BLOCK_TOK ? te : t0 + AR_BLOCK_TOK;
      for (int64_t tt = t0 + q; tt < t1; tt += (int64_t)AR_SLOTS * UNR) {
        Vec x[UNR];
        bool ok[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int64_t t = tt + (int64_t)u * AR_SLOTS;
          ok[u] = false;
          if (t < t1) {
            const int64_t row = token_to_row(L, b, t, len);
            if (row >= 0 && row < L.n_rows) {
              ok[u] = true;
              const raw* p = xin + row * H + col0;
              if constexpr (AL) {
                *(uint4*)&x[u] = *(const uint4*)p;
              } else {
#pragma unroll
                for (int e = 0; e < VE; ++e) x[u].e[e] = e < nval ? p[e] : (raw)0;
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (!ok[u]) continue;
          const uint32_t off = (uint32_t)(tt - t0) + (uint32_t)(u * AR_SLOTS);
#pragma unroll
          for (int e = 0; e < VE; ++e) {
            const A a = E::up(x[u].e[e]);
            if (ar_better<OP>(a, off, v[e], o[e])) { v[e] = a; o[e] = off; }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VE; ++e) ar_merge_block<OP>(V[e], I[e], v[e], o[e], t0);
    }
  }

  // tokens 0 .. 7 (mod 8) of a wave sit 8 lanes apart
#pragma unroll
  for (int k = AR_LPR; k < RUA_WAVE; k <<= 1) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      const A v2 = __shfl_xor(V[e], k, RUA_WAVE);
      const int64_t i2 = __shfl_xor(I[e], k, RUA_WAVE);
      ar_merge<OP>(V[e], I[e], v2, i2);
    }
  }
  if ((tid & (RUA_WAVE - 1)) < AR_LPR) {
#pragma unroll
    for (int e = 0; e < VE; ++e) { xv[w][l][e] = V[e]; xi[w][l][e] = I[e]; }
  }
  __syncthreads();
  if (tid >= AR_LPR || !active) return;
#pragma unroll
  for (int k = 1; k < RUA_WAVES_PER_BLOCK; ++k) {
#pragma unroll
    for (int e = 0; e < VE; ++e) ar_merge<OP>(V[e], I[e], xv[k][l][e], xi[k][l][e]);
  }
  if (mode == SEG_PARTIAL) {
    const int64_t at = (((b * maxblk + blk) * n_chunks + c) * AR_LPR + l) * VE;
#pragma unroll
    for (int e = 0; e < VE; ++e) { wsv[at + e] = V[e]; wsi[at + e] = I[e]; }
    return;
  }
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (e >= nval) continue;
    iout[b * H + col0 + e] = I[e];
    if (vout) vout[b * H + col0 + e] = E::down(V[e]);
  }
}

// ---------------------------------------------------------------- take: out[b,h] = data[row(b, index[b,h]), h]
// One thread per output element; 0 where the position names no token of the sequence.  U: the element as bits.
template <typename U>
__global__ __launch_bounds__(RUA_BLOCK) void seg_take_kernel(rua_layout L, const U* data, const int64_t* index, U* out,
                                                             int64_t H, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int64_t b = div_rows(i, H);
  const int64_t h = i - b * H;
  const int64_t len = safe_len(L, b);
  const int64_t t = index[i];
  U v = 0;
  if (t >= 0 && t < len) {
    const int64_t row = token_to_row(L, b, t, len);
    if (row >= 0 && row < L.n_rows) v = data[row * H + h];
  }
  out[i] = v;
}

// ---------------------------------------------------------------- put: out[row(b,t),h] = t == index[b,h] ? src[b,h] : 0
// A workgroup takes (sequence x column chunk x block of positions): thread (q, l) owns the l-th 16-byte vector of the
// chunk — it loads the chunk's positions and source elements ONCE — and writes the rows q, q + slots, ...  A chunk is
// `lpr` vectors (a power of two up to 8: 128 bytes), so narrow rows put more rows side by side.  The positions of a LEFT /
// RIGHT storage are its T_phys rows per sequence, padding included (zeros): the whole payload is written in the one
// pass.  A row takes no value from another block, so long sequences are cut into blocks with no second launch.
template <typename U, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_put_kernel(rua_layout L, const U* src, const int64_t* index, U* out,
                                                            int64_t H, int n_chunks, int lpr_log2, int nblk) {
  constexpr int VE = 16 / (int)sizeof(U);
  struct alignas(16) Vec { U e[VE]; };
  const int tid = threadIdx.x;
  const int l = tid & ((1 << lpr_log2) - 1), q = tid >> lpr_log2, slots = RUA_BLOCK >> lpr_log2;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  const int blk = (int)(b % nblk);
  b /= nblk;
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  const bool padded = L.kind == RUA_LEFT || L.kind == RUA_RIGHT;
  const int64_t col0 = ((int64_t)c << lpr_log2) * VE + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  if (nval == 0) return;
  int64_t idx[VE];
  U s[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    idx[e] = e < nval ? index[b * H + col0 + e] : -1;
    s[e] = e < nval ? src[b * H + col0 + e] : (U)0;
  }
  int64_t pb = 0, pe = padded ? L.T_phys : len;
  if (nblk > 1) {
    pb = (int64_t)blk * AR_BLOCK_TOK;
    if (pb > pe) pb = pe;
    if (pe > pb + AR_BLOCK_TOK) pe = pb + AR_BLOCK_TOK;
  }
  const int64_t lo = L.kind == RUA_RIGHT ? L.T_log - len : 0;
  for (int64_t p = pb + q; p < pe; p += slots) {
    int64_t row, t;
    if (padded) {
      row = b * L.T_phys + p;
      t = is_pad(L, p, len) ? -1 : p - lo;
    } else {
      t = p;
      row = token_to_row(L, b, p, len);
    }
    if (row < 0 || row >= L.n_rows) continue;
    Vec o;
#pragma unroll
    for (int e = 0; e < VE; ++e) o.e[e] = (t >= 0 && t == idx[e]) ? s[e] : (U)0;
    U* d = out + row * H + col0;
    if constexpr (AL) {
      *(uint4*)d = *(const uint4*)&o;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) if (e < nval) d[e] = o.e[e];
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps a position (8 bytes) and a value (one accumulator) per block and (padded) column
static seg_plan ar_make_plan(const rua_layout& L, int64_t H, int32_t dtype) {
  const int es = seg_esize(dtype, true);
  return seg_make_plan(L, H, es, 8 + (es == 8 ? 8 : 4));
}

template <typename E, int OP>
static int ar_launch(const rua_layout& L, const void* x, void* values, int64_t* index, int64_t H, int32_t dtype, void* ws,
                     hipStream_t s) {
  using raw = typename E::raw;
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t base = (uint64_t)(uintptr_t)x;
  const char* opn = OP == RUA_MAX ? "max" : "min";
  if (base % sizeof(raw) || (uint64_t)(uintptr_t)values % sizeof(raw) || (uint64_t)(uintptr_t)index % 8)
    return RUA_EALIGN;                                         // (elements themselves are always aligned)

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, base, L.B);
    if (!ln.grid) return RUA_ERANGE;
    seg_trace("seg_argreduce_lanes_kernel T=%s op=%s W=%d H=%d values=%d kind=%d", E::name(), opn, ln.W, (int)H,
              (int)(values != nullptr), L.kind);
    hipLaunchKernelGGL((seg_argreduce_lanes_kernel<E, OP>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, L,
                       (const char*)x, (raw*)values, index, (int)H, ln.W);
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(ar_make_plan(L, H, dtype), L, row_bytes, base, ws != nullptr);
  const seg_plan& p = r.p;
  if (p.n_chunks <= 0) return RUA_ERANGE;
  if (r.cut && (uint64_t)(uintptr_t)ws % 8) return RUA_EALIGN;
  if (!r.grid) return RUA_ERANGE;
  return seg_launch_rows(
      r,
      [&](int mode) {                                          // the finish: a workgroup per (sequence, chunk)
        const int64_t grid = mode == SEG_FINISH ? L.B * (int64_t)p.n_chunks : r.grid;
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_argreduce_rows_kernel<E, OP, decltype(AL)::value>), dim3((unsigned)grid), dim3(RUA_BLOCK),
                             0, s, L, (const raw*)x, (raw*)values, index, H, p.n_chunks, mode, r.cut ? p.maxblk : 1,
                             (char*)ws);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("seg_argreduce_rows_kernel T=%s op=%s AL=%d values=%d kind=%d cut=1 phase=%s blocks=%d chunks=%d",
                    E::name(), opn, (int)r.al, (int)(values != nullptr), L.kind, phase, p.maxblk, p.n_chunks);
        else
          seg_trace("seg_argreduce_rows_kernel T=%s op=%s AL=%d values=%d kind=%d cut=0 chunks=%d", E::name(), opn,
                    (int)r.al, (int)(values != nullptr), L.kind, p.n_chunks);
      });
}

static int ar_dispatch(const rua_layout* lay, const void* x, void* values, int64_t* index, int64_t H, int32_t dtype,
                       int32_t op, void* ws, void* stream) {
  const int es = seg_esize(dtype, true);
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (op != RUA_MAX && op != RUA_MIN) return RUA_EINVAL;
  if (lay->B == 0 || H == 0) return 0;
  if (!index || (!x && lay->n_rows > 0)) return RUA_EINVAL;    // (an empty storage still owes every sequence its -1)
  if (seg_too_large(lay, H, es) || (double)lay->B * (double)H >= 1.0e18)
    return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
#define RUA_AR(E)                                                                                                      \
  (op == RUA_MAX ? ar_launch<E, RUA_MAX>(*lay, x, values, index, H, dtype, ws, s)                                      \
                 : ar_launch<E, RUA_MIN>(*lay, x, values, index, H, dtype, ws, s))
  if (dtype == RUA_I64) return RUA_AR(ar_i64);
  RUA_DISPATCH_FLOAT(dtype, RUA_AR);
#undef RUA_AR
}

// take / put move elements as bits: one instantiation per element size
template <typename U>
static int take_launch(const rua_layout& L, const void* data, const int64_t* index, void* out, int64_t H, hipStream_t s) {
  if (((uint64_t)(uintptr_t)data | (uint64_t)(uintptr_t)out) % sizeof(U) || (uint64_t)(uintptr_t)index % 8) return RUA_EALIGN;
  const int64_t total = L.B * H;
  const int64_t grid = (total + RUA_BLOCK - 1) / RUA_BLOCK;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_take_kernel esize=%d H=%lld kind=%d", (int)sizeof(U), (long long)H, L.kind);
  hipLaunchKernelGGL((seg_take_kernel<U>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L, (const U*)data, index, (U*)out,
                     H, total);
  return (int)hipGetLastError();
}

template <typename U>
static int put_launch(const rua_layout& L, const void* src, const int64_t* index, void* out, int64_t H, hipStream_t s) {
  const uint64_t bases = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)out;
  if (bases % sizeof(U) || (uint64_t)(uintptr_t)index % 8) return RUA_EALIGN;
  const int64_t row_bytes = H * (int64_t)sizeof(U);
  const int64_t vecs = (row_bytes + 15) / 16;
  int lpr_log2 = 0;
  while (lpr_log2 < 3 && (1 << lpr_log2) < vecs) ++lpr_log2;
  const int64_t chunks = (vecs + (1 << lpr_log2) - 1) >> lpr_log2;
  if (chunks > 0x7fffffff) return RUA_ERANGE;
  const bool al = row_bytes % 16 == 0 && (uint64_t)(uintptr_t)out % 16 == 0;
  const int64_t units = L.B * chunks;
  const int64_t cutblk = seg_cut_blocks(L, units);             // (rows of one vector are cut too: a row per thread)
  const int64_t nblk = cutblk > 0 ? cutblk : 1;
  if (nblk > SEG_CUT_MAX_BLOCKS) return RUA_ERANGE;
  const int64_t grid = units * nblk;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_put_kernel esize=%d AL=%d kind=%d lpr=%d chunks=%d blocks=%d", (int)sizeof(U), (int)al, L.kind,
            1 << lpr_log2, (int)chunks, (int)nblk);
  seg_with_al(al, [&](auto AL) {
    hipLaunchKernelGGL((seg_put_kernel<U, decltype(AL)::value>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, L,
                       (const U*)src, index, (U*)out, H, (int)chunks, lpr_log2, (int)nblk);
  });
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int64_t rua_argreduce_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::ar_make_plan(*lay, H, dtype).ws_bytes;
}

extern "C" int rua_segment_argreduce(const rua_layout* lay, const void* data, void* values, int64_t* index, int64_t H,
                                     int32_t dtype, int32_t op, void* ws, void* stream) {
  return rua::ar_dispatch(lay, data, values, index, H, dtype, op, ws, stream);
}

extern "C" int rua_segment_take(const rua_layout* lay, const void* data, const int64_t* index, void* out, int64_t H,
                                int32_t dtype, void* stream) {
  const int es = rua::seg_esize(dtype, true);
  int e;
  if ((e = rua::seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || H == 0) return 0;
  if (!index || !out || (!data && lay->n_rows > 0)) return RUA_EINVAL;
  if (data && data == out) return RUA_EINVAL;
  if (rua::seg_too_large(lay, H, es) || (double)lay->B * (double)H >= 1.0e18)
    return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  switch (es) {
    case 2: return rua::take_launch<uint16_t>(*lay, data, index, out, H, s);
    case 4: return rua::take_launch<uint32_t>(*lay, data, index, out, H, s);
    case 8: return rua::take_launch<uint64_t>(*lay, data, index, out, H, s);
  }
  return RUA_EINVAL;
}

extern "C" int rua_segment_put(const rua_layout* lay, const void* src, const int64_t* index, void* out, int64_t H,
                               int32_t dtype, void* stream) {
  const int es = rua::seg_esize(dtype, true);
  int e;
  if ((e = rua::seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!src || !index || !out || src == out) return RUA_EINVAL;
  if (rua::seg_too_large(lay, H, es) || (double)lay->B * (double)H >= 1.0e18)
    return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  switch (es) {
    case 2: return rua::put_launch<uint16_t>(*lay, src, index, out, H, s);
    case 4: return rua::put_launch<uint32_t>(*lay, src, index, out, H, s);
    case 8: return rua::put_launch<uint64_t>(*lay, src, index, out, H, s);
  }
  return RUA_EINVAL;
}
