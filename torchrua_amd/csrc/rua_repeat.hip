// rua_repeat.hip — per-sequence repeat_interleave: every token of a C / L / P / R container `counts[b, t]` times in its
// own sequence (rua_segment_repeat_plan, rua_segment_repeat_move, rua_segment_repeat_sum; include/rua.h).  An extension,
// the inverse direction of rua_compress.hip: the result's raggedness GROWS from the data.
//
// Three steps, with the caller's one read-back of the new lengths between the first two (they size the result):
//   plan  a per-sequence exclusive scan of the int64 counts in the input's storage layout: first[row] = the position of
//         the token's first copy in its new sequence, -1 for a padding row; new_lens[b]; new_lens[B] = how many counts
//         were invalid (negative or above 2^31 - 1: taken as 0).  Integer work: every form gives the same bits.
//   move  DESTINATION-driven: the row of every token (b, u) of the result reads the row of the source token t, the
//         largest t with first[row(b, t)] <= u (or u / uniform without a table).  A workgroup owns a block of consecutive
//         destination tokens of one sequence, finds the source tokens that block covers once, stages their `first`
//         entries in LDS and searches there.  The copies of a long run are different destination tokens: they spread
//         over the threads of a workgroup, and over workgroups only where the destination is cut.
//   sum   the adjoint, SOURCE-driven: every token adds the rows of its run in ascending u in fp32 (fp64 for float64)
//         and rounds once.  A run is walked by one thread group: correct for any count, slow for a very long one.
// All walk sequence by sequence (token_to_row), so a PackedSequence, whose tokens of one sequence are strided, and a
// right-aligned batch take the same walk as a CattedSequence.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_scan.h"
#include "rua_repeat_plan.h"

namespace rua {

constexpr int RM_UNR = 4;                  // tokens in flight per thread
constexpr int RM_STAGE = SEG_BLOCK_TOK;    // `first` entries a workgroup stages per block of destination tokens
static_assert(RUA_WAVE == 64, "the scans below shuffle inside 64 lanes");
static_assert(RUA_BLOCK == 256, "a row chunk of eight 16-byte pieces on 32 token slots, or a token per thread");

// ---------------------------------------------------------------- the plan
// the family's offsets scan (rua_seg_scan.h) over the counts: a token's value is its count (an invalid one: counted,
// taken as 0), the sum in front of a lane a shuffle scan, and every token stores the position of its first copy
struct rp_scan {
  using in_t = int64_t;
  using out_t = int64_t;
  using sum_t = int64_t;
  using val_t = int64_t;
  static constexpr bool COUNTS_INVALID = true;
  static constexpr int64_t PAD = -1;
  static const char* kernel() { return "seg_repeat_plan_kernel"; }
  static const char* phase1() { return "sum"; }
  static __device__ __forceinline__ int64_t load(const int64_t* counts, int64_t row, int& bad) {
    int64_t c = counts[row];
    if (c < 0 || c > RP_MAX_COUNT) { c = 0; ++bad; }
    return c;
  }
  template <int G>
  static __device__ __forceinline__ void wave_prefix(int64_t c, int lane, int q, int64_t& before, int64_t& total) {
    constexpr int GW = G < RUA_WAVE ? G : RUA_WAVE;            // the lanes that scan together by shuffles
    int64_t inc = c;                                           // inclusive scan over the GW lanes
#pragma unroll
    for (int d = 1; d < GW; d <<= 1) {
      const int64_t o = __shfl_up(inc, d, GW);
      if ((lane & (GW - 1)) >= d) inc += o;
    }
    total = __shfl(inc, GW - 1, GW);
    before = inc - c;
  }
  static __device__ __forceinline__ int64_t store(int64_t, int64_t pos) { return pos; }
};
static_assert(sizeof(rp_scan::sum_t) == RP_WS_ELEM_BYTES, "the workspace the host plan sizes holds the kernel's sums");

// first[] of source token (b, t); a token whose row is not in the storage never matches
__device__ __forceinline__ int64_t rm_first(const rua_layout& S, const int64_t* __restrict__ first, int64_t b, int64_t t,
                                            int64_t slen) {
  const int64_t row = token_to_row(S, b, t, slen);
  return row >= 0 && row < S.n_rows ? first[row] : 0x7fffffffffffffffLL;
}

// largest t in [lo, hi) with first(b, t) <= u   (requires lo < hi; when first(b, lo) > u the answer is lo all the same)
__device__ __forceinline__ int64_t rm_search(const rua_layout& S, const int64_t* __restrict__ first, int64_t b,
                                             int64_t slen, int64_t lo, int64_t hi, int64_t u) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rm_first(S, first, b, mid, slen) <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// the unit of a walk: sequence b, column chunk c, and the blocks [k0, ...) of SEG_BLOCK_TOK tokens it takes — all of
// them (maxblk == 0), its own (cut), or its own and what a bound that understates left over (the last block of a cut)
__device__ __forceinline__ void rm_unit(int n_chunks, int maxblk, int& c, int64_t& b, int64_t& k0, bool& one_block) {
  c = (int)(blockIdx.x % (unsigned)n_chunks);
  const int64_t unit = blockIdx.x / (unsigned)n_chunks;
  b = unit;
  k0 = 0;
  one_block = false;
  if (maxblk > 0) {
    k0 = unit % maxblk;
    b = unit / maxblk;
    one_block = k0 < maxblk - 1;
  }
}

// ---------------------------------------------------------------- the move
// A workgroup per (sequence of D, 128-byte column chunk[, block]).  Thread (q, l) = (tid >> lpr_log2, tid & (lpr - 1))
// takes the destination tokens q, q + slots, ... of the block, RM_UNR of them in flight, and owns the l-th 16-byte piece
// of the chunk (rows of one vector: lpr = 1, a token per thread).  Per block of destination tokens [ub, ue) the source
// tokens [t_lo, t_hi] it covers are found once (two searches, the same for every thread), their `first` entries go to
// LDS as offsets from ub, and every destination token searches there; a block that covers more source tokens than the
// stage holds (long stretches of zero counts) searches the table itself.
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_repeat_move_kernel(rua_layout D, rua_layout S,
                                                                    const int64_t* __restrict__ first, int64_t uniform,
                                                                    char* __restrict__ dst, const char* __restrict__ src,
                                                                    int64_t rb, int n_chunks, int lpr_log2, int maxblk) {
  __shared__ int32_t stage[RM_STAGE];
  const int tid = threadIdx.x;
  const int l = tid & ((1 << lpr_log2) - 1), q = tid >> lpr_log2;
  const int slots = RUA_BLOCK >> lpr_log2;
  int c;
  int64_t b, k0;
  bool one_block;
  rm_unit(n_chunks, maxblk, c, b, k0, one_block);
  if (b >= D.B) return;                                        // (workgroup-uniform)
  const int64_t col0 = (int64_t)c * 128 + (int64_t)l * 16;
  const int nb = rb - col0 >= 16 ? 16 : (rb - col0 > 0 ? (int)(rb - col0) : 0);
  const int64_t dlen = safe_len(D, b), slen = safe_len(S, b);

  for (int64_t k = k0; k * SEG_BLOCK_TOK < dlen; ++k) {        // (workgroup-uniform trip count)
    const int64_t ub = k * SEG_BLOCK_TOK;
    const int64_t ue = dlen - ub > SEG_BLOCK_TOK ? ub + SEG_BLOCK_TOK : dlen;
    int64_t t_lo = 0, n_src = 0;
    bool staged = false;
    if (first && slen > 0) {
      t_lo = rm_search(S, first, b, slen, 0, slen, ub);
      n_src = rm_search(S, first, b, slen, t_lo, slen, ue - 1) - t_lo + 1;
      staged = n_src <= RM_STAGE;
      __syncthreads();                                         // the block before has been searched
      if (staged) {
        for (int i = tid; i < (int)n_src; i += RUA_BLOCK) {
          const int64_t f = rm_first(S, first, b, t_lo + i, slen) - ub;
          stage[i] = f <= 0 ? 0 : (f > SEG_BLOCK_TOK ? SEG_BLOCK_TOK : (int32_t)f);
        }
      }
      __syncthreads();
    }
    if (nb > 0) {
      for (int64_t u0 = ub + q; u0 < ue; u0 += (int64_t)slots * RM_UNR) {
        int64_t drows[RM_UNR], srows[RM_UNR];
        row_vec v[RM_UNR];
#pragma unroll
        for (int i = 0; i < RM_UNR; ++i) {
          const int64_t u = u0 + (int64_t)i * slots;
          drows[i] = srows[i] = -1;
          row_zero(v[i]);
          if (u >= ue) continue;
          const int64_t drow = token_to_row(D, b, u, dlen);
          if (drow < 0 || drow >= D.n_rows) continue;
          drows[i] = drow;
          int64_t t = -1;
          if (!first) {
            if (uniform > 0) t = div_rows(u, uniform);
          } else if (staged) {
            const int32_t x = (int32_t)(u - ub);
            int lo = 0, hi = (int)n_src;
            while (hi - lo > 1) {
              const int mid = (lo + hi) >> 1;
              if (stage[mid] <= x) lo = mid; else hi = mid;
            }
            t = t_lo + lo;
          } else if (n_src > 0) {
            t = rm_search(S, first, b, slen, t_lo, t_lo + n_src, u);
          }
          if (t < 0 || t >= slen) continue;                    // a token nothing maps to is written as zeros
          const int64_t srow = token_to_row(S, b, t, slen);
          if (srow >= 0 && srow < S.n_rows) srows[i] = srow;
        }
#pragma unroll
        for (int i = 0; i < RM_UNR; ++i)
          if (srows[i] >= 0) row_ld<W>(src + srows[i] * rb + col0, nb, v[i]);
#pragma unroll
        for (int i = 0; i < RM_UNR; ++i)
          if (drows[i] >= 0) row_st<W>(dst + drows[i] * rb + col0, nb, v[i]);
      }
    }
    if (one_block) break;
  }

  // padding rows of a LEFT / RIGHT destination as zeros: position q, q + slots, ... of [0, T_phys)
  if (k0 == 0 && nb > 0 && (D.kind == RUA_LEFT || D.kind == RUA_RIGHT)) {
    row_vec z;
    row_zero(z);
    for (int64_t j = q; j < D.T_phys; j += slots) {
      if (!is_pad(D, j, dlen)) continue;
      const int64_t row = b * D.T_phys + j;
      if (row < D.n_rows) row_st<W>(dst + row * rb + col0, nb, z);
    }
  }
}

// ---------------------------------------------------------------- the run sum
// A workgroup per (sequence of S, 128-byte column chunk[, block of source tokens]); thread (q, l) takes the source tokens
// q, q + slots, ... and the l-th 16-byte piece of the chunk: EPL elements, folded over u = first, first + 1, ... in the
// accumulator type and rounded once.  ONE fold order per (token, column) whatever the two layouts are.  `vec`: the row
// width and both bases allow 16-byte accesses; otherwise element by element.
template <typename E>
__global__ __launch_bounds__(RUA_BLOCK) void seg_repeat_sum_kernel(rua_layout S, rua_layout D,
                                                                   const int64_t* __restrict__ first,
                                                                   const int64_t* __restrict__ counts, int64_t uniform,
                                                                   typename E::raw* __restrict__ gsrc,
                                                                   const typename E::raw* __restrict__ gdst, int64_t H,
                                                                   int n_chunks, int lpr_log2, int maxblk, int vec) {
  using raw = typename E::raw;
  using acc = typename E::acc;
  constexpr int EPL = 16 / (int)sizeof(raw);
  const int tid = threadIdx.x;
  const int l = tid & ((1 << lpr_log2) - 1), q = tid >> lpr_log2;
  const int slots = RUA_BLOCK >> lpr_log2;
  int c;
  int64_t b, k0;
  bool one_block;
  rm_unit(n_chunks, maxblk, c, b, k0, one_block);
  if (b >= S.B) return;
  const int64_t col0 = ((int64_t)c * 8 + l) * EPL;
  const int ne = H - col0 >= EPL ? EPL : (H - col0 > 0 ? (int)(H - col0) : 0);
  if (ne <= 0) return;                                         // (no barrier below)
  const int64_t slen = safe_len(S, b), dlen = safe_len(D, b);
  const int64_t tb = k0 * SEG_BLOCK_TOK;
  const int64_t te = one_block && slen - tb > SEG_BLOCK_TOK ? tb + SEG_BLOCK_TOK : slen;

  struct alignas(16) piece { raw e[EPL]; };
  for (int64_t t = tb + q; t < te; t += slots) {
    const int64_t row = token_to_row(S, b, t, slen);
    if (row < 0 || row >= S.n_rows) continue;
    int64_t f, n;
    if (first) {
      f = first[row];
      n = counts[row];
      if (n < 0 || n > RP_MAX_COUNT) n = 0;                    // as the plan took it
    } else {
      f = t * uniform;
      n = uniform;
    }
    if (f < 0) n = 0;
    int64_t end = f + n;
    if (end > dlen) end = dlen;
    acc a[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) a[e] = (acc)0;
    for (int64_t u = f; u < end; ++u) {
      const int64_t drow = token_to_row(D, b, u, dlen);
      if (drow < 0 || drow >= D.n_rows) continue;
      const raw* p = gdst + drow * H + col0;
      piece x;
      if (vec) {
        x = *(const piece*)p;
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) if (e < ne) x.e[e] = p[e];
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) if (e < ne) a[e] += E::up(x.e[e]);
    }
    piece y;
#pragma unroll
    for (int e = 0; e < EPL; ++e) y.e[e] = E::down(a[e]);
    raw* o = gsrc + row * H + col0;
    if (vec) {
      *(piece*)o = y;
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) if (e < ne) o[e] = y.e[e];
    }
  }

  if (k0 == 0 && (S.kind == RUA_LEFT || S.kind == RUA_RIGHT)) {
    for (int64_t j = q; j < S.T_phys; j += slots) {
      if (!is_pad(S, j, slen)) continue;
      const int64_t row = b * S.T_phys + j;
      if (row >= S.n_rows) continue;
      raw* o = gsrc + row * H + col0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) if (e < ne) o[e] = E::down((acc)0);
    }
  }
}

// ---------------------------------------------------------------- host side
static int rm_launch_move(const rua_layout& D, const rua_layout& S, const int64_t* first, int64_t uniform, char* dst,
                          const char* src, int64_t rb, hipStream_t s) {
  const int W = seg_access_width(rb, (uint64_t)(uintptr_t)dst | (uint64_t)(uintptr_t)src);
  const rp_walk w = rp_make_walk(D, rb);
  if (!w.grid) return RUA_ERANGE;
  if (g_trace_on.load(std::memory_order_relaxed) != 0) {
    char rec[200];
    snprintf(rec, sizeof rec, "seg_repeat_move_kernel form=%s W=%d row_bytes=%lld table=%d dst=%d src=%d cut=%d blocks=%d chunks=%d",
             w.lpr_log2 ? "rows" : "lanes", W, (long long)rb, (int)(first != nullptr), D.kind, S.kind, (int)(w.maxblk > 0),
             w.maxblk, w.n_chunks);
    trace_add(rec);
  }
#define RUA_RM_MOVE(WV)                                                                                                \
  hipLaunchKernelGGL((seg_repeat_move_kernel<WV>), dim3((unsigned)w.grid), dim3(RUA_BLOCK), 0, s, D, S, first, uniform,  \
                     dst, src, rb, w.n_chunks, w.lpr_log2, w.maxblk)
  RUA_DISPATCH_W(W, RUA_RM_MOVE)
#undef RUA_RM_MOVE
  return (int)hipGetLastError();
}

template <typename E>
static int rs_launch_sum(const rua_layout& S, const rua_layout& D, const int64_t* first, const int64_t* counts,
                         int64_t uniform, void* gsrc, const void* gdst, int64_t H, hipStream_t s) {
  using raw = typename E::raw;
  const int64_t rb = H * (int64_t)sizeof(raw);
  const rp_walk w = rp_make_walk(S, rb);
  if (!w.grid) return RUA_ERANGE;
  const int vec = ((uint64_t)rb | (uint64_t)(uintptr_t)gsrc | (uint64_t)(uintptr_t)gdst) % 16 == 0;
  if (g_trace_on.load(std::memory_order_relaxed) != 0) {
    char rec[200];
    snprintf(rec, sizeof rec, "seg_repeat_sum_kernel form=%s dtype=%s H=%lld vec=%d table=%d src=%d dst=%d cut=%d blocks=%d chunks=%d",
             w.lpr_log2 ? "rows" : "lanes", E::name(), (long long)H, vec, (int)(first != nullptr), S.kind, D.kind,
             (int)(w.maxblk > 0), w.maxblk, w.n_chunks);
    trace_add(rec);
  }
  hipLaunchKernelGGL((seg_repeat_sum_kernel<E>), dim3((unsigned)w.grid), dim3(RUA_BLOCK), 0, s, S, D, first, counts,
                     uniform, (raw*)gsrc, (const raw*)gdst, H, w.n_chunks, w.lpr_log2, w.maxblk, vec);
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int64_t rua_repeat_ws_bytes(const rua_layout* lay) {
  using namespace rua;
  if (seg_check_entry(lay, 1, 1) != 0) return 0;
  return seg_make_scan_plan(*lay, RP_WS_ELEM_BYTES).ws_bytes;
}

extern "C" int rua_segment_repeat_plan(const rua_layout* lay, const int64_t* counts, int64_t* first, int64_t* new_lens,
                                       void* ws, void* stream) {
  using namespace rua;
  int e;
  if ((e = seg_check_entry(lay, 1, 1)) != 0) return e;
  if (lay->B == 0) return 0;
  if (!new_lens || (lay->n_rows > 0 && (!counts || !first))) return RUA_EINVAL;
  if ((const void*)first == (const void*)counts || (const void*)new_lens == (const void*)counts ||
      (const void*)new_lens == (const void*)first)
    return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)counts % 8 || (uint64_t)(uintptr_t)first % 8 || (uint64_t)(uintptr_t)new_lens % 8 ||
      (uint64_t)(uintptr_t)ws % 8)
    return RUA_EALIGN;
  seg_scan_plan p = seg_make_scan_plan(*lay, RP_WS_ELEM_BYTES);
  if (p.form == SEG_SCAN_CUT && !ws) {                         // ws == NULL: do not cut
    p.form = SEG_SCAN_LONG;
    p.maxblk = 0;
    p.grid = lay->B;
  }
  if (p.grid <= 0 || p.grid > 0x7fffffffLL) return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  if ((e = (int)hipMemsetAsync(new_lens + lay->B, 0, sizeof(int64_t), s)) != 0) return e;    // the invalid-count word
  return seg_launch_offsets<rp_scan>(p, *lay, counts, first, new_lens, ws, s);
}

extern "C" int rua_segment_repeat_move(const rua_layout* dst, const rua_layout* src, const int64_t* first,
                                       int64_t uniform, void* dst_data, const void* src_data, int64_t row_bytes,
                                       void* stream) {
  using namespace rua;
  int e;
  if ((e = seg_check_entry(src, row_bytes, 1)) != 0) return e;
  if ((e = seg_check_entry(dst, row_bytes, 1)) != 0) return e;
  if (dst->B != src->B || (!first && uniform < 0)) return RUA_EINVAL;
  if (dst->B == 0 || row_bytes == 0 || dst->n_rows == 0) return 0;
  if (!dst_data || dst_data == src_data || (src->n_rows > 0 && !src_data)) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)first % 8) return RUA_EALIGN;
  if (seg_too_large(src, row_bytes, 1) || seg_too_large(dst, row_bytes, 1)) return RUA_ERANGE;
  return rm_launch_move(*dst, *src, first, uniform, (char*)dst_data, (const char*)src_data, row_bytes,
                        (hipStream_t)stream);
}

extern "C" int rua_segment_repeat_sum(const rua_layout* src, const rua_layout* dst, const int64_t* first,
                                      const int64_t* counts, int64_t uniform, void* grad_src, const void* grad_dst,
                                      int64_t H, int32_t dtype, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = seg_check_entry(src, H, es)) != 0) return e;
  if ((e = seg_check_entry(dst, H, es)) != 0) return e;
  if (dst->B != src->B || (!first && uniform < 0) || (first && !counts)) return RUA_EINVAL;
  if (src->B == 0 || H == 0 || src->n_rows == 0) return 0;
  if (!grad_src || grad_src == grad_dst || (dst->n_rows > 0 && !grad_dst)) return RUA_EINVAL;
  if ((const void*)grad_src == (const void*)first || (const void*)grad_src == (const void*)counts) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)first % 8 || (uint64_t)(uintptr_t)counts % 8 || (uint64_t)(uintptr_t)grad_src % es ||
      (uint64_t)(uintptr_t)grad_dst % es)
    return RUA_EALIGN;
  if (seg_too_large(src, H, es) || seg_too_large(dst, H, es)) return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case RUA_F32:  return rs_launch_sum<sm_f32>(*src, *dst, first, counts, uniform, grad_src, grad_dst, H, s);
    case RUA_F64:  return rs_launch_sum<sm_f64>(*src, *dst, first, counts, uniform, grad_src, grad_dst, H, s);
    case RUA_BF16: return rs_launch_sum<sm_bf16>(*src, *dst, first, counts, uniform, grad_src, grad_dst, H, s);
    case RUA_F16:  return rs_launch_sum<sm_f16>(*src, *dst, first, counts, uniform, grad_src, grad_dst, H, s);
  }
  return RUA_EINVAL;
}
