// rua_sort.hip — per-sequence STABLE sort / argsort of a C / L / P / R container, per column, and the per-sequence
// permutation that goes with it (rua_segment_sort, rua_segment_reorder; include/rua.h).  An extension.
//
// An element is (key image, position): the key an order-preserving unsigned image of the value (sign flip for floats,
// every NaN one maximum, -0 -> +0, a bias for int64; inverted for `descending`), the position the token's place in its
// sequence.  Elements are sorted ASCENDING as a whole, so equal keys keep ascending position in both directions and no
// form needs stability logic; the order is total, so every form and every layout gives the same bits.  The values are
// gathered from the input by position afterwards: a NaN keeps its payload, -0.0 stays -0.0.
//   lanes  bound <= 64: a sequence (and column) on G = 8 .. 64 lanes, 64 / G sequences per wave, a bitonic network of
//          cross-lane exchanges; no LDS
//   block  a workgroup per (block of 2 048 tokens of a sequence, column): a bitonic network over an LDS slab of the
//          block's elements (the next power of two above its length); sequences that fit a block are finished here
//   merge  longer sequences: ceil(log2(blocks)) rank-merge passes over a FLAT grid of storage elements through a
//          ping-pong workspace (rua_sort_plan.h: pairing, destination, parity); the last pass of a sequence writes the
//          caller's outputs.  No synchronisation between workgroups inside a launch; a pass no sequence needs returns
//          at its first load (the block sort leaves the passes needed in the workspace's first word).
// All address tokens through token_to_row / row_to_token, so the four layouts share every kernel.
#include <stdint.h>
#include "rua_seg_launch.h"
#include "rua_sort_plan.h"

namespace rua {

static_assert(RUA_WAVE == 64 && RUA_BLOCK == 256, "four waves of 64 lanes per workgroup");

// ---------------------------------------------------------------- elements
// 2- and 4-byte values: the image in the high word, the position in the low one — one 64-bit compare
struct el32 {
  uint64_t c;
  static constexpr bool WIDE = false;
  static __device__ __forceinline__ el32 make(uint32_t k, uint32_t p) { return {((uint64_t)k << 32) | p}; }
  static __device__ __forceinline__ el32 pad() { return {~0ull}; }     // after every element: positions are 31 bits
  __device__ __forceinline__ uint32_t pos() const { return (uint32_t)c; }
  __device__ __forceinline__ bool less(const el32& o) const { return c < o.c; }
  __device__ __forceinline__ el32 xchg(int m) const { return {(uint64_t)__shfl_xor((long long)c, m, RUA_WAVE)}; }
};
// 8-byte values: 64 bits of image and the position beside them
struct el64 {
  uint64_t k;
  uint32_t p;
  static constexpr bool WIDE = true;
  static __device__ __forceinline__ el64 make(uint64_t k, uint32_t p) { return {k, p}; }
  static __device__ __forceinline__ el64 pad() { return {~0ull, ~0u}; }
  __device__ __forceinline__ uint32_t pos() const { return p; }
  __device__ __forceinline__ bool less(const el64& o) const { return k < o.k || (k == o.k && p < o.p); }
  __device__ __forceinline__ el64 xchg(int m) const {
    return {(uint64_t)__shfl_xor((long long)k, m, RUA_WAVE), (uint32_t)__shfl_xor((int)p, m, RUA_WAVE)};
  }
};

// an array of elements (LDS slab or ping-pong buffer): `a` the 64-bit words, `b` the positions of the wide elements
struct el_array {
  uint64_t* a;
  uint32_t* b;
};
__device__ __forceinline__ el32 el_ld(const el_array& s, int64_t i, el32*) { return {s.a[i]}; }
__device__ __forceinline__ el64 el_ld(const el_array& s, int64_t i, el64*) { return {s.a[i], s.b[i]}; }
__device__ __forceinline__ void el_st(const el_array& s, int64_t i, const el32& e) { s.a[i] = e.c; }
__device__ __forceinline__ void el_st(const el_array& s, int64_t i, const el64& e) { s.a[i] = e.k; s.b[i] = e.p; }

// ---------------------------------------------------------------- key images, by dtype
struct sk_f32 {
  using raw = uint32_t; using el = el32;
  static const char* name() { return "f32"; }
  static __device__ __forceinline__ uint32_t image(raw u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0;
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  }
};
template <uint16_t INF> struct sk_half {
  using raw = uint16_t; using el = el32;
  static __device__ __forceinline__ uint32_t image(raw u) {
    if ((u & 0x7fffu) > INF) return 0xffffu;
    if (u == 0x8000u) u = 0;
    return (uint32_t)(uint16_t)(u ^ ((u >> 15) ? 0xffffu : 0x8000u));
  }
};
struct sk_bf16 : sk_half<0x7f80> { static const char* name() { return "bf16"; } };
struct sk_f16 : sk_half<0x7c00> { static const char* name() { return "f16"; } };
struct sk_f64 {
  using raw = uint64_t; using el = el64;
  static const char* name() { return "f64"; }
  static __device__ __forceinline__ uint64_t image(raw u) {
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;
    if (u == 0x8000000000000000ull) u = 0;
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  }
};
struct sk_i64 {
  using raw = uint64_t; using el = el64;
  static const char* name() { return "i64"; }
  static __device__ __forceinline__ uint64_t image(raw u) { return u ^ 0x8000000000000000ull; }
};

// the element of token (b, t), column h; a token whose row is not in the storage sorts behind everything
template <typename D>
__device__ __forceinline__ typename D::el sk_load(const rua_layout& L, const typename D::raw* __restrict__ data,
                                                  int64_t H, int64_t h, int64_t b, int64_t t, int64_t slen, int desc) {
  using el = typename D::el;
  const int64_t row = token_to_row(L, b, t, slen);
  if (row < 0 || row >= L.n_rows) return el::pad();
  auto k = D::image(data[row * H + h]);
  if (desc) k = ~k;
  return el::make(k, (uint32_t)t);
}

// rank t of (b, h) is the token at position p: both outputs of that place.  A pad (p out of range) leaves zeros
template <typename D>
__device__ __forceinline__ void sk_emit(const rua_layout& L, const typename D::raw* __restrict__ data,
                                        typename D::raw* __restrict__ values, int64_t* __restrict__ indices, int64_t H,
                                        int64_t h, int64_t b, int64_t t, uint32_t p, int64_t slen) {
  const int64_t drow = token_to_row(L, b, t, slen);
  if (drow < 0 || drow >= L.n_rows) return;
  typename D::raw v = 0;
  int64_t at = 0;
  if ((int64_t)p < slen) {
    const int64_t srow = token_to_row(L, b, (int64_t)p, slen);
    if (srow >= 0 && srow < L.n_rows) { v = data[srow * H + h]; at = (int64_t)p; }
  }
  indices[drow * H + h] = at;
  if (values) values[drow * H + h] = v;
}

// ---------------------------------------------------------------- lanes form
template <typename D, int G>
__global__ __launch_bounds__(RUA_BLOCK) void seg_sort_lanes_kernel(rua_layout L, const typename D::raw* __restrict__ data,
                                                                   typename D::raw* __restrict__ values,
                                                                   int64_t* __restrict__ indices, int64_t H,
                                                                   int64_t units, int desc) {
  using el = typename D::el;
  constexpr int PER_WAVE = RUA_WAVE / G;
  const int lane = threadIdx.x & (RUA_WAVE - 1), wave = threadIdx.x >> 6;
  const int g = lane / G, i = lane & (G - 1);
  const int64_t unit = ((int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + wave) * PER_WAVE + g;
  const bool live = unit < units;                              // (every lane takes part in the exchanges below)
  int64_t b = 0, h = 0, slen = 0;
  if (live) {
    b = div_rows(unit, H);
    h = unit - b * H;
    slen = safe_len(L, b);
  }
  const int n = slen < G ? (int)slen : G;                      // (a bound that understates: the first G tokens)
  el e = el::pad();
  if (i < n) e = sk_load<D>(L, data, H, h, b, i, slen, desc);
#pragma unroll
  for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const el o = e.xchg(j);
      const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
      if (keep_min ? o.less(e) : e.less(o)) e = o;
    }
  }
  if (i < n) sk_emit<D>(L, data, values, indices, H, h, b, i, e.pos(), slen);
  if (live)
    seg_fill_padding(L, b, slen, i, G, [&](int64_t row) {
      indices[row * H + h] = 0;
      if (values) values[row * H + h] = 0;
    });
}

// ---------------------------------------------------------------- block form
// the unit of a block-sort workgroup: (sequence b, block blk).  CAT: block 0 of sequence u for u < B; unit B + w takes the
// one later block that STARTS inside the storage rows [w * 2 048, (w + 1) * 2 048) — it belongs to the sequence that
// holds the window's first row (a sequence that begins inside the window has its block 1 beyond it; blocks of one
// sequence start 2 048 rows apart).  Other layouts: u = b * maxblk + blk.  false: nothing to do
__device__ __forceinline__ bool sort_unit(const rua_layout& L, int64_t u, int maxblk, int64_t& b, int64_t& blk) {
  if (L.kind != RUA_CAT) {
    b = u / maxblk;
    blk = u - b * maxblk;
    return b < L.B;
  }
  if (u < L.B) { b = u; blk = 0; return true; }
  const int64_t r0 = (u - L.B) << SORT_BLOCK_LOG2;
  if (r0 >= L.n_rows || cat_off(L, 0) > r0) return false;
  b = search_cat(L, r0);
  const int64_t d = r0 - cat_off(L, b);
  if (d <= 0) return false;                                    // the window starts with the sequence: its block 0
  blk = (d + SEG_BLOCK_TOK - 1) >> SORT_BLOCK_LOG2;
  return (blk << SORT_BLOCK_LOG2) - d < SEG_BLOCK_TOK;
}

template <typename D>
__global__ __launch_bounds__(RUA_BLOCK) void seg_sort_block_kernel(rua_layout L, const typename D::raw* __restrict__ data,
                                                                   typename D::raw* __restrict__ values,
                                                                   int64_t* __restrict__ indices, int64_t H, int maxblk,
                                                                   int planned, int desc, el_array buf, int* need) {
  using el = typename D::el;
  __shared__ uint64_t s_a[SEG_BLOCK_TOK];
  __shared__ uint32_t s_b[el::WIDE ? SEG_BLOCK_TOK : 1];
  const el_array slab = {s_a, s_b};
  const int tid = threadIdx.x;
  const int64_t u = (int64_t)(blockIdx.x / (uint64_t)H), h = (int64_t)(blockIdx.x % (uint64_t)H);
  int64_t b, blk;
  if (!sort_unit(L, u, maxblk, b, blk)) return;                // (workgroup-uniform, as every return before a barrier)
  const int64_t slen = safe_len(L, b);
  if (blk == 0)
    seg_fill_padding(L, b, slen, tid, RUA_BLOCK, [&](int64_t row) {
      indices[row * H + h] = 0;
      if (values) values[row * H + h] = 0;
    });
  const int64_t t0 = blk << SORT_BLOCK_LOG2;
  if (t0 >= slen) return;
  const int n = slen - t0 < SEG_BLOCK_TOK ? (int)(slen - t0) : SEG_BLOCK_TOK;
  int n2 = 2;
  while (n2 < n) n2 <<= 1;                                     // n2 <= SEG_BLOCK_TOK: the slab holds it
  for (int i = tid; i < n2; i += RUA_BLOCK)
    el_st(slab, i, i < n ? sk_load<D>(L, data, H, h, b, t0 + i, slen, desc) : el::pad());
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = tid; x < (n2 >> 1); x += RUA_BLOCK) {
        const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
        const el a = el_ld(slab, lo, (el*)nullptr), c = el_ld(slab, hi, (el*)nullptr);
        if ((lo & k) == 0 ? c.less(a) : a.less(c)) {
          el_st(slab, lo, c);
          el_st(slab, hi, a);
        }
      }
      __syncthreads();
    }
  }
  int mine = sort_passes(slen, SORT_BLOCK_LOG2);
  if (mine > planned) mine = planned;                          // (a bound that understates: the blocks stay apart)
  if (mine == 0) {
    for (int i = tid; i < n; i += RUA_BLOCK)
      sk_emit<D>(L, data, values, indices, H, h, b, t0 + i, el_ld(slab, i, (el*)nullptr).pos(), slen);
    return;
  }
  for (int i = tid; i < n; i += RUA_BLOCK) {
    const int64_t row = token_to_row(L, b, t0 + i, slen);
    if (row >= 0 && row < L.n_rows) el_st(buf, row * H + h, el_ld(slab, i, (el*)nullptr));
  }
  if (tid == 0 && blk == 0 && h == 0) atomicMax(need, mine);
}

// ---------------------------------------------------------------- merge pass
// a thread per storage element: its element of the source buffer goes to base + (own offset) + (rank in the other run)
template <typename D>
__global__ __launch_bounds__(RUA_BLOCK) void seg_sort_merge_kernel(rua_layout L, const typename D::raw* __restrict__ data,
                                                                   typename D::raw* __restrict__ values,
                                                                   int64_t* __restrict__ indices, int64_t H,
                                                                   int64_t n_elems, int pass, int planned, el_array src,
                                                                   el_array dst, const int* __restrict__ need) {
  using el = typename D::el;
  if (pass >= *need) return;                                   // a surplus pass: nothing is walked
  const int64_t e = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (e >= n_elems) return;
  const int64_t row = div_rows(e, H), h = e - row * H;
  int64_t b, t;
  if (!row_to_token(L, row, b, t)) return;
  const int64_t slen = safe_len(L, b);
  if (t < 0 || t >= slen || token_to_row(L, b, t, slen) != row) return;
  int mine = sort_passes(slen, SORT_BLOCK_LOG2);
  if (mine > planned) mine = planned;
  if (pass >= mine) return;
  const el me = el_ld(src, e, (el*)nullptr);
  auto at = [&](int64_t m) {
    const int64_t r = token_to_row(L, b, m, slen);
    return r >= 0 && r < L.n_rows ? el_ld(src, r * H + h, (el*)nullptr) : el::pad();
  };
  int64_t base, mid, end;
  sort_pairing(t, slen, SORT_BLOCK_LOG2 + pass, base, mid, end);
  int64_t dest = t;
  if (mid < end) {
    int64_t lo, hi;
    if (t < mid) {                                             // lower bound in the right run
      lo = mid; hi = end;
      while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (at(m).less(me)) lo = m + 1; else hi = m;
      }
      dest = sort_dest(base, mid, t, lo - mid);
    } else {                                                   // upper bound in the left run
      lo = base; hi = mid;
      while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (me.less(at(m))) hi = m; else lo = m + 1;
      }
      dest = sort_dest(base, mid, t, lo - base);
    }
  }
  if (dest < 0 || dest >= slen) return;
  if (pass == mine - 1) {
    sk_emit<D>(L, data, values, indices, H, h, b, dest, me.pos(), slen);
  } else {
    const int64_t r = token_to_row(L, b, dest, slen);
    if (r >= 0 && r < L.n_rows) el_st(dst, r * H + h, me);
  }
}

// ---------------------------------------------------------------- reorder
// per row: a thread group (one lane for rows of one vector, eight otherwise) owns the row `row` of the storage; its
// partner row is the token index[row] of the same sequence.  gather: out[row] = in[partner] (zeros where there is
// none: a padding row, a position outside the sequence); scatter: out[partner] = in[row] (out was zeroed)
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_reorder_rows_kernel(rua_layout L, const char* __restrict__ src,
                                                                     const int64_t* __restrict__ index,
                                                                     char* __restrict__ dst, int64_t rb, int lpr_log2,
                                                                     int inverse) {
  const int l = threadIdx.x & ((1 << lpr_log2) - 1), q = threadIdx.x >> lpr_log2;
  const int64_t row = (int64_t)blockIdx.x * (RUA_BLOCK >> lpr_log2) + q;
  if (row >= L.n_rows) return;
  int64_t b, t, partner = -1;
  if (row_to_token(L, row, b, t)) {
    const int64_t slen = safe_len(L, b);
    if (t >= 0 && t < slen) {
      const int64_t i = index[row];
      if (i >= 0 && i < slen) {
        const int64_t r = token_to_row(L, b, i, slen);
        if (r >= 0 && r < L.n_rows) partner = r;
      }
    }
  }
  if (inverse && partner < 0) return;
  const int64_t srow = inverse ? row : partner, drow = inverse ? partner : row;
  for (int64_t c0 = (int64_t)l * 16; c0 < rb; c0 += (int64_t)16 << lpr_log2) {
    const int nb = rb - c0 >= 16 ? 16 : (int)(rb - c0);
    row_vec v;
    row_zero(v);
    if (srow >= 0) row_ld<W>(src + srow * rb + c0, nb, v);
    row_st<W>(dst + drow * rb + c0, nb, v);
  }
}

// per element: a thread per storage element (row, h); its partner is (token index[row, h] of the same sequence, h)
template <typename U>
__global__ __launch_bounds__(RUA_BLOCK) void seg_reorder_elems_kernel(rua_layout L, const U* __restrict__ src,
                                                                      const int64_t* __restrict__ index,
                                                                      U* __restrict__ dst, int64_t H, int64_t n_elems,
                                                                      int inverse) {
  const int64_t e = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (e >= n_elems) return;
  const int64_t row = div_rows(e, H), h = e - row * H;
  int64_t b, t, partner = -1;
  if (row_to_token(L, row, b, t)) {
    const int64_t slen = safe_len(L, b);
    if (t >= 0 && t < slen) {
      const int64_t i = index[e];
      if (i >= 0 && i < slen) {
        const int64_t r = token_to_row(L, b, i, slen);
        if (r >= 0 && r < L.n_rows) partner = r * H + h;
      }
    }
  }
  if (inverse) {
    if (partner >= 0) dst[partner] = src[e];
  } else {
    dst[e] = partner >= 0 ? src[partner] : (U)0;
  }
}

// ---------------------------------------------------------------- host side
static el_array sort_buffer(char* ws, const sort_plan& p, int which, bool wide) {
  char* a = ws + SORT_WS_HEADER + (int64_t)which * sort_pad256(p.buf_elems * 8);
  char* b = ws + SORT_WS_HEADER + 2 * sort_pad256(p.buf_elems * 8) + (int64_t)which * sort_pad256(p.buf_elems * 4);
  return {(uint64_t*)a, wide ? (uint32_t*)b : nullptr};
}

template <typename D>
static int sort_launch(const sort_plan& p, const rua_layout& L, const void* data, void* values, int64_t* indices,
                       int64_t H, int desc, void* ws, hipStream_t s) {
  using raw = typename D::raw;
  const raw* in = (const raw*)data;
  raw* out = (raw*)values;
  seg_trace("seg_sort_%s_kernel dtype=%s H=%lld G=%d kind=%d values=%d desc=%d passes=%d",
            p.form == SORT_LANES ? "lanes" : "block", D::name(), (long long)H, p.G, L.kind, (int)(values != nullptr), desc,
            p.passes);
  if (p.form == SORT_LANES) {
    const int64_t units = L.B * H;
#define RUA_SORT_LANES(GV)                                                                                             \
  hipLaunchKernelGGL((seg_sort_lanes_kernel<D, GV>), dim3((unsigned)p.grid), dim3(RUA_BLOCK), 0, s, L, in, out, indices, \
                     H, units, desc)
    switch (p.G) {
      case 8:  RUA_SORT_LANES(8); break;
      case 16: RUA_SORT_LANES(16); break;
      case 32: RUA_SORT_LANES(32); break;
      default: RUA_SORT_LANES(64); break;
    }
#undef RUA_SORT_LANES
    return (int)hipGetLastError();
  }
  el_array b0 = {nullptr, nullptr}, b1 = {nullptr, nullptr};
  int* need = nullptr;
  if (p.form == SORT_MERGE) {
    need = (int*)ws;
    b0 = sort_buffer((char*)ws, p, 0, D::el::WIDE);
    b1 = sort_buffer((char*)ws, p, 1, D::el::WIDE);
    const int e = (int)hipMemsetAsync(ws, 0, SORT_WS_HEADER, s);
    if (e != 0) return e;
  }
  hipLaunchKernelGGL((seg_sort_block_kernel<D>), dim3((unsigned)p.grid), dim3(RUA_BLOCK), 0, s, L, in, out, indices, H,
                     p.maxblk > 0 ? p.maxblk : 1, p.passes, desc, b0, need);
  int e = (int)hipGetLastError();
  for (int pass = 0; pass < p.passes && e == 0; ++pass) {
    const bool from0 = sort_src_buffer(pass) == 0;
    seg_trace("seg_sort_merge_kernel pass=%d of=%d run=%lld", pass, p.passes, (long long)SEG_BLOCK_TOK << pass);
    hipLaunchKernelGGL((seg_sort_merge_kernel<D>), dim3((unsigned)p.merge_grid), dim3(RUA_BLOCK), 0, s, L, in, out,
                       indices, H, p.buf_elems, pass, p.passes, from0 ? b0 : b1, from0 ? b1 : b0, (const int*)need);
    e = (int)hipGetLastError();
  }
  return e;
}

}  // namespace rua

extern "C" int64_t rua_sort_block_len(void) { return rua::SEG_BLOCK_TOK; }

extern "C" int64_t rua_sort_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  using namespace rua;
  const int es = seg_esize(dtype, true);
  if (seg_check_entry(lay, H, es) != 0) return 0;
  return sort_make_plan(*lay, H, es).ws_bytes;
}

extern "C" int rua_segment_sort(const rua_layout* lay, const void* data, void* values, int64_t* indices, int64_t H,
                                int32_t dtype, int32_t descending, void* ws, void* stream) {
  using namespace rua;
  const int es = seg_esize(dtype, true);
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (sm_len_bound(*lay) > SORT_MAX_LEN) return RUA_ERANGE;
  if (lay->B == 0 || H == 0 || lay->n_rows == 0) return 0;
  if (!data || !indices || data == values || data == (const void*)indices || values == (void*)indices) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)data % es || (uint64_t)(uintptr_t)values % es || (uint64_t)(uintptr_t)indices % 8 ||
      (uint64_t)(uintptr_t)ws % 256)
    return RUA_EALIGN;
  if (seg_too_large(lay, H, 24)) return RUA_ERANGE;
  const sort_plan p = sort_make_plan(*lay, H, es);
  if (p.form < 0) return RUA_ERANGE;
  if (p.form == SORT_MERGE && !ws) return RUA_EINVAL;          // sequences longer than a block need the workspace
  hipStream_t s = (hipStream_t)stream;
  const int desc = descending != 0;
  switch (dtype) {
    case RUA_F32:  return sort_launch<sk_f32>(p, *lay, data, values, indices, H, desc, ws, s);
    case RUA_BF16: return sort_launch<sk_bf16>(p, *lay, data, values, indices, H, desc, ws, s);
    case RUA_F16:  return sort_launch<sk_f16>(p, *lay, data, values, indices, H, desc, ws, s);
    case RUA_F64:  return sort_launch<sk_f64>(p, *lay, data, values, indices, H, desc, ws, s);
    case RUA_I64:  return sort_launch<sk_i64>(p, *lay, data, values, indices, H, desc, ws, s);
  }
  return RUA_EINVAL;
}

extern "C" int rua_segment_reorder(const rua_layout* lay, const void* data, const int64_t* index, void* out, int64_t H,
                                   int32_t elem_bytes, int32_t per_row, int32_t inverse, void* stream) {
  using namespace rua;
  const int es = elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8 ? elem_bytes : 0;
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || H == 0 || lay->n_rows == 0) return 0;
  if (!data || !index || !out || data == out || (const void*)index == data || (const void*)index == (const void*)out)
    return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)index % 8 || (uint64_t)(uintptr_t)data % es || (uint64_t)(uintptr_t)out % es) return RUA_EALIGN;
  if (seg_too_large(lay, H, 8)) return RUA_ERANGE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rb = H * es;
  if (inverse && (e = (int)hipMemsetAsync(out, 0, (size_t)(lay->n_rows * rb), s)) != 0) return e;
  if (per_row) {
    const int lpr_log2 = rb <= 16 ? 0 : 3;
    const int64_t slots = RUA_BLOCK >> lpr_log2, grid = (lay->n_rows - 1) / slots + 1;
    if (grid > 0x7fffffffLL) return RUA_ERANGE;
    const int W = seg_access_width(rb, (uint64_t)(uintptr_t)data | (uint64_t)(uintptr_t)out);
    seg_trace("seg_reorder_rows_kernel form=%s W=%d row_bytes=%lld kind=%d inverse=%d", lpr_log2 ? "rows" : "lanes", W,
              (long long)rb, lay->kind, (int)(inverse != 0));
#define RUA_REORDER_ROWS(WV)                                                                                           \
  hipLaunchKernelGGL((seg_reorder_rows_kernel<WV>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, *lay,                 \
                     (const char*)data, index, (char*)out, rb, lpr_log2, (int)(inverse != 0))
    RUA_DISPATCH_W(W, RUA_REORDER_ROWS)
#undef RUA_REORDER_ROWS
    return (int)hipGetLastError();
  }
  const int64_t n_elems = lay->n_rows * H, grid = (n_elems - 1) / RUA_BLOCK + 1;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_reorder_elems_kernel elem_bytes=%d H=%lld kind=%d inverse=%d", es, (long long)H, lay->kind,
            (int)(inverse != 0));
#define RUA_REORDER_ELEMS(U)                                                                                           \
  hipLaunchKernelGGL((seg_reorder_elems_kernel<U>), dim3((unsigned)grid), dim3(RUA_BLOCK), 0, s, *lay, (const U*)data,  \
                     index, (U*)out, H, n_elems, (int)(inverse != 0))
  switch (es) {
    case 1: RUA_REORDER_ELEMS(uint8_t); break;
    case 2: RUA_REORDER_ELEMS(uint16_t); break;
    case 4: RUA_REORDER_ELEMS(uint32_t); break;
    default: RUA_REORDER_ELEMS(uint64_t); break;
  }
#undef RUA_REORDER_ELEMS
  return (int)hipGetLastError();
}
