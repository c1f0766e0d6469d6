// rua_attention_paged.hip — the forward of attention over a PAGED KV cache for ANY number of queries per sequence: a
// prompt, or a chunk of one, against the pool the decode steps read (rua_segment_attention_paged_forward; include/rua.h;
// DESIGN 3.2v).  K and V live in a pool [num_pages][page_size][heads_kv][D] (q's dtype, or OCP e4m3 codes with one fp32
// scale per kv head), a block table [B][max_pages] of int32 names the pages of every sequence, and the kv rua_layout
// supplies only the LENGTHS — the arguments of rua_attention_decode_paged.hip, whose row rule (pg_entry / pg_row) this
// file shares.  The result is the band forward of rua_attention.hip over the rows the table names, BIT FOR BIT.
//
// GEOMETRY: THE FORWARD'S WALK ON THE DECODE KERNELS' COLUMNS.  For sequence b and kv head hk the matrix columns are the
// packed pairs c = t G + gi — query position t, head hk G + gi, G = heads / heads_kv — for c < T_b G.  A work item is
// (sequence, kv head, block of 128 columns), items = B x heads_kv x ceil(T_max G / 128), and at most 2 048 workgroups
// stride over them in the closed form of attn_items.  A workgroup is 4 waves and wave w owns the columns 32 w .. 32 w +
// 31 of the block.  The KEYS are not divided between the waves: every wave walks all the visible keys of the block in
// tiles of 64 cut by position from 0, staged in LDS ONCE per workgroup for all G heads — the band forward stages the
// same tile once per query head — so there is no split, no workspace, no combine: ONE launch.  With G = 4 a block
// covers 32 query positions; a sequence of a few dozen queries fills its columns instead of a quarter of them.
//
// PER COLUMN THE ARITHMETIC IS THE BAND FORWARD'S, expression for expression: the transposed score tile K Q^T with the
// staged K as the A operand and q (loaded once per item) as B, the select to -inf, m_use / alpha, l from the unrounded
// p, P rounded once (bf16: hi + lo), the O^T accumulator, attn_store_row.  A column of an MFMA result depends on its own
// B column alone, a skipped sub-tile and a wholly masked one leave (m, l, acc) untouched alike, and sub-tiles are met in
// ascending order of position in both kernels: the bits of a (query, head) do not depend on which other columns share
// its wave.  The lane's own query t = c / G gives the visible keys as one interval [see_lo, see_hi) of positions, cut
// per sub-tile into the offsets [vlo, vhi) as the decode kernels do.
//
// THE WALK.  kbeg = attn_band_lo(first query of the block) rounded down to 64, kend = attn_band_hi(last query of the
// block that exists).  A wave skips a 32-key sub-tile wholly right (break) or left (continue) of the band of ITS OWN
// columns' queries; a wave whose columns are all past T_b G skips its MFMAs and still stages.  Block 0 of every
// (sequence, kv head) writes the padding zeros of an L / R result for its G heads.  Columns are cut by position and
// head, never by storage row: all four q layouts give the same bits.
//
// STAGING.  LDS is the forward's: K plain [64][D + 8], V transposed [D][64 + 8], 16-bit elements.  Thread i owns key row
// i / 4 of the tile and the 8-element chunks i % 4, i % 4 + 4, .. of that row, for K and for V: ONE table entry and ONE
// pool row per thread and tile.  A table entry is read only for a column < max_pages and a key < S_b; a page id outside
// [0, num_pages) and the rows of a last page past S_b are never dereferenced and stage as ZERO rows.  e4m3 codes are
// loaded 8 bytes at a time, converted exactly in registers (dec8_up) and stored as 16-bit elements: the tiles, the
// operand order and the bank layout stay the forward's, no d permutation.  k's scale goes once per item into the
// softmax scale, v's multiplies the fp32 accumulator once before the store.
//
// THE TABLE AND HBM ARE KEPT OUT OF THE TILE LOOP.  The global loads of tile k0 + 64 are issued into registers after the
// barrier that publishes tile k0 and before its MFMAs; they are written to LDS after the barrier that ends tile k0.  The
// table entry they need was loaded one tile earlier still and waits in one register.  Cost: D / 4 VGPRs per thread with a
// 16-bit pool (32 at D = 128), half of that with codes.  One instantiation stages in place instead (pgf_ahead below).
//
// THE BUILD FLAGS ARE rua_attention.o's, not the decode objects': with packed fp32 operations switched off the compiler
// rounds f16 results with v_fma_mixlo_f16 — the exact product acc x 1 / l rounded ONCE — where the band forward's object
// multiplies in fp32 and then converts.  The two differ by one f16 ulp in about one element of 8 000 (measured), which is
// all that "the bits of attention" would then lack.
//
// REGISTERS: profiles/attention_paged_registers.txt (no scratch in any of the 12 instantiations).
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include "rua_attention_paged_dev.h"

namespace rua {

// 8 elements of a pool row as they lie in memory: 16 bytes of 16-bit elements, or 8 bytes of codes (in .x, .y)
template <bool F8> __device__ __forceinline__ uint4 pgf_load(const uint8_t* __restrict__ p) {
  if constexpr (F8) {
    const uint2 c = *(const uint2*)p;
    return make_uint4(c.x, c.y, 0u, 0u);
  } else {
    return *(const uint4*)p;
  }
}

// the chunks q4, q4 + 4, .. of kv head hk of pool row `row` of K and of V; row < 0: zeros (for codes 0x00 = +0)
template <int NCH, int D, bool F8>
__device__ __forceinline__ void pgf_fetch(int64_t row, int hk, int hkv, int q4, const uint8_t* __restrict__ k,
                                          const uint8_t* __restrict__ v, uint4* kr, uint4* vr) {
  constexpr int ES = F8 ? 1 : 2;
  const int64_t at = ((row * hkv + hk) * (int64_t)D + 8 * q4) * ES;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    kr[i] = vr[i] = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) {
      kr[i] = pgf_load<F8>(k + at + 32 * i * ES);
      vr[i] = pgf_load<F8>(v + at + 32 * i * ES);
    }
  }
}

// the fetched chunks of key row r of the tile into LDS as 16-bit elements: K plain [64][D + 8], V transposed [D][64 + 8]
template <typename X, int NCH, int D, bool F8>
__device__ __forceinline__ void pgf_put(const uint4* kr, const uint4* vr, int r, int q4, uint16_t* sK, uint16_t* sVt) {
  constexpr int PS = D + 8, TS = ATTN_KB + 8;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int d0 = 8 * (q4 + 4 * i);
    const uint4 kx = F8 ? dec8_up<X>(kr[i].x, kr[i].y) : kr[i], vx = F8 ? dec8_up<X>(vr[i].x, vr[i].y) : vr[i];
    *(uint4*)(sK + r * PS + d0) = kx;
#pragma unroll
    for (int e = 0; e < 8; ++e) sVt[(d0 + e) * TS + r] = attn_elem(vx, e);
  }
}

// whether an instantiation keeps the next tile in registers over the MFMAs of the current one.  One does not: f16 D = 128
// with codes would lose a wave per SIMD to those registers (2 -> 1; profiles/attention_paged_registers.txt has both
// builds); it fetches and stages in place, the table entry still a tile ahead.  Wherever else the occupancy is below the
// band forward's it is so in both builds.
template <typename X, int D, bool F8> constexpr bool pgf_ahead() { return X::SPLIT || !(D == 128 && F8); }

// ---------------------------------------------------------------- the walk: one (sequence, kv head, block of 128 columns)
template <typename X, int D, bool F8>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_paged_forward_kernel(
    rua_layout LQ, rua_layout LK, dec_pages pt, const uint16_t* __restrict__ q, const uint8_t* __restrict__ k,
    const uint8_t* __restrict__ v, const float* __restrict__ k_scale, const float* __restrict__ v_scale, float k_mul,
    float v_mul, uint16_t* __restrict__ out, float* __restrict__ lse, int heads, float scale, int64_t ncb, int64_t items,
    attn_band bd) {
  constexpr int PS = D + 8, TS = ATTN_KB + 8, NS = D / 16, ND = D / 32, NCH = D / 32;
  constexpr bool AHEAD = pgf_ahead<X, D, F8>();
  __shared__ __attribute__((aligned(16))) uint16_t sK[ATTN_KB * PS];
  __shared__ __attribute__((aligned(16))) uint16_t sVt[D * TS];
  const int tid = (int)threadIdx.x, lane = tid & (RUA_WAVE - 1), j = lane & 31, g = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sr = tid >> 2, q4 = tid & 3;                        // the key row of a tile this thread stages; its chunks
  const float NEG_INF = -__builtin_inff();
  const int hkv = bd.heads_kv, G = heads / hkv;

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t cb = item % ncb, bh = item / ncb;
    const int hk = (int)(bh % hkv);
    const int64_t b = bh / hkv;
    const int64_t T = safe_len(LQ, b);
    if (cb == 0)
      for (int gi = 0; gi < G; ++gi) attn_zero_padding<D>(LQ, b, T, hk * G + gi, heads, out, nullptr, lse, tid);
    const int64_t c0 = cb * ATTN_BLOCK_TOK, cols = T * G;
    if (c0 >= cols) continue;
    const int64_t S = safe_len(LK, b);

    // the scales of this kv head (codes only): k's goes into the softmax scale, v's waits for the accumulator
    float sc = scale, vs = 1.f;
    if constexpr (F8) {
      sc = scale * ((k_scale ? k_scale[hk] : 1.f) * k_mul);
      vs = (v_scale ? v_scale[hk] : 1.f) * v_mul;
    }

    // the keys that the block's queries t_lo .. t_hi may see, walked in tiles cut by position from 0 (an empty band: no
    // tile, and the zero rows and lse = -inf below)
    const int64_t shift = bd.align_end ? S - T : 0;
    const int64_t t_lo = c0 / G, t_top = (c0 + ATTN_BLOCK_TOK - 1) / G, t_hi = t_top < T ? t_top : T - 1;
    const int64_t kbeg = attn_band_lo(t_lo + shift, bd.left) / ATTN_KB * ATTN_KB;
    const int64_t kend = attn_band_hi(t_hi + shift, bd.right, S);

    // the table entries of the first two tiles, ahead of everything else the work item loads
    const int32_t* __restrict__ tb = pt.table + b * pt.max_pages;
    int32_t pg_cur = pg_entry(pt, tb, S, kbeg, kbeg < kend, sr);
    int32_t pg_next = pg_entry(pt, tb, S, kbeg + ATTN_KB, kbeg + ATTN_KB < kend, sr);

    // the wave's columns and the queries they hold; the lane's column: query position t, head h; its q operand
    const int64_t wc0 = c0 + 32 * wv, c = wc0 + j, t = c / G;
    const bool live = wc0 < cols;
    const int64_t w_lo = wc0 / G, w_top = (wc0 + 31) / G, w_hi = w_top < T ? w_top : T - 1;
    const int h = hk * G + (int)(c % G);
    const int64_t qrow = t < T ? attn_row(LQ, b, t, T) : (int64_t)-1;
    uint4 qf[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      qf[st] = make_uint4(0u, 0u, 0u, 0u);
      if (qrow >= 0) qf[st] = *(const uint4*)(q + (qrow * heads + h) * (int64_t)D + 16 * st + 8 * g);
    }
    // the keys [see_lo, see_hi) that the lane's own query sees (the band and the end of the sequence, as positions)
    const int64_t see_lo = attn_band_lo(t + shift, bd.left), see_hi = attn_band_hi(t + shift, bd.right, S);
    attn_f32x16 acc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
    float m = NEG_INF, l = 0.f;

    uint4 kr[NCH], vr[NCH];
    if constexpr (AHEAD)
      pgf_fetch<NCH, D, F8>(kbeg < kend ? pg_row(pt, pg_cur, S, kbeg, sr) : (int64_t)-1, hk, hkv, q4, k, v, kr, vr);
    for (int64_t k0 = kbeg; k0 < kend; k0 += ATTN_KB) {
      const int64_t kn = k0 + ATTN_KB;
      if constexpr (!AHEAD) pgf_fetch<NCH, D, F8>(pg_row(pt, pg_cur, S, k0, sr), hk, hkv, q4, k, v, kr, vr);
      pgf_put<X, NCH, D, F8>(kr, vr, sr, q4, sK, sVt);
      __syncthreads();
      // AHEAD: the next tile's K / V set out now, from the entry that has waited a tile, and land in LDS after the
      // barrier below; either way the entry of the tile after the next sets out now
      if constexpr (AHEAD)
        pgf_fetch<NCH, D, F8>(kn < kend ? pg_row(pt, pg_next, S, kn, sr) : (int64_t)-1, hk, hkv, q4, k, v, kr, vr);
      pg_cur = pg_next;
      pg_next = pg_entry(pt, tb, S, kn + ATTN_KB, kn + ATTN_KB < kend, sr);
      if (live) {
#pragma unroll
        for (int sub = 0; sub < ATTN_KB / 32; ++sub) {
          const int64_t ks = k0 + 32 * sub;
          if (ks >= kend) break;                                // past the end
          // wholly right / left of the band of the wave's queries
          if (bd.right >= 0 && ks - (w_hi + shift) > bd.right) break;
          if (bd.left >= 0 && ks + 31 - (w_lo + shift) < -bd.left) continue;
          attn_f32x16 s;
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
          for (int st = 0; st < NS; ++st)
            s = X::mfma(*(const uint4*)(sK + (32 * sub + j) * PS + 16 * st + 8 * g), qf[st], s);
          // the online softmax on the accumulator layout: the lane is the column, its registers are keys; the keys of
          // the sub-tile that the lane's query sees are the offsets [vlo, vhi)
          const int64_t dlo = see_lo - ks, dhi = see_hi - ks;
          const int vlo = dlo < 0 ? 0 : dlo > 32 ? 32 : (int)dlo, vhi = dhi < 0 ? 0 : dhi > 32 ? 32 : (int)dhi;
          float sv[16], mx = NEG_INF;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int off = 8 * (r >> 2) + 4 * g + (r & 3);     // key ks + off
            sv[r] = (off >= vlo && off < vhi) ? s[r] * sc : NEG_INF;
            mx = fmaxf(mx, sv[r]);
          }
          mx = fmaxf(mx, __shfl_xor(mx, 32, RUA_WAVE));
          const float m_new = fmaxf(m, mx);
          const float m_use = m_new == NEG_INF ? 0.f : m_new;
          const float alpha = expf(m - m_use);
          float psum = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            sv[r] = expf(sv[r] - m_use);
            psum += sv[r];                                      // l is summed from the unrounded p
          }
          psum += __shfl_xor(psum, 32, RUA_WAVE);
          l = l * alpha + psum;
          m = m_new;
          const uint4 pb0 = attn_pack8<X>(sv), pb1 = attn_pack8<X>(sv + 8);
          uint4 pl0 = pb0, pl1 = pb1;
          if constexpr (X::SPLIT) {
            pl0 = attn_pack8_lo<X>(sv);
            pl1 = attn_pack8_lo<X>(sv + 8);
          }
#pragma unroll
          for (int dt = 0; dt < ND; ++dt) {
            const uint4 a0 = attn_ld_t<TS>(sVt, 32 * dt + j, 32 * sub, 0, g), a1 = attn_ld_t<TS>(sVt, 32 * dt + j, 32 * sub, 1, g);
            acc[dt] = acc[dt] * alpha;
            acc[dt] = X::mfma(a0, pb0, acc[dt]);
            acc[dt] = X::mfma(a1, pb1, acc[dt]);
            if constexpr (X::SPLIT) {
              acc[dt] = X::mfma(a0, pl0, acc[dt]);
              acc[dt] = X::mfma(a1, pl1, acc[dt]);
            }
          }
        }
      }
      __syncthreads();                                          // the tile is consumed (the next item's too starts here)
    }

    if (qrow >= 0) {                                            // a query without a visible key: zeros and lse = -inf
      if constexpr (F8) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) acc[dt] = acc[dt] * vs; // v's scale, once
      }
      attn_store_row<X, D>(acc, l > 0.f ? 1.f / l : 0.f, out + (qrow * heads + h) * (int64_t)D, g);
      if (g == 0) lse[qrow * heads + h] = l > 0.f ? m + logf(l) : NEG_INF;
    }
  }
}

}  // namespace rua

extern "C" int rua_segment_attention_paged_forward(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                                   const void* k_ptr, const void* v_ptr, void* out, void* lse,
                                                   int32_t heads, int32_t D, int32_t dtype, int32_t heads_kv,
                                                   int64_t left, int64_t right, int32_t align_end, double scale,
                                                   int64_t T_max, int64_t S_max, int32_t kv_dtype, const float* k_scale,
                                                   const float* v_scale, double k_scale_by_value,
                                                   double v_scale_by_value, const int32_t* page_table, int64_t max_pages,
                                                   int32_t page_size, int64_t num_pages, void* stream) {
  using namespace rua;
  int e;
  bool f8;
  dec_pages pt;
  if ((e = attn_check_entry(q, kv, heads, heads_kv, D, dtype, scale, T_max)) != 0) return e;
  if (S_max < 0) return RUA_EINVAL;
  if ((e = pg_check_cache(kv_dtype, k_scale, v_scale, k_scale_by_value, v_scale_by_value, f8)) != 0) return e;
  if ((e = pg_check(q, heads_kv, D, f8 ? 1 : 2, k_ptr, v_ptr, page_table, max_pages, page_size, num_pages, S_max,
                    pt.lg)) != 0)
    return e;
  if (q->B == 0 || T_max == 0) return 0;
  if (q->n_rows > 0 && (!q_ptr || !out || !lse)) return RUA_EINVAL;
  if (attn_misaligned(q_ptr) || attn_misaligned(k_ptr) || attn_misaligned(v_ptr) || attn_misaligned(out) ||
      ((uintptr_t)lse & 3) || ((uintptr_t)k_scale & 3) || ((uintptr_t)v_scale & 3))
    return RUA_EALIGN;
  if (seg_too_large(q, (int64_t)heads * D, 2)) return RUA_ERANGE;
  const int32_t G = heads / heads_kv;
  if ((double)T_max * (double)G >= 4.0e18) return RUA_ERANGE;
  int64_t ncb, items;
  unsigned grid;
  if (!attn_items(q->B, heads_kv, T_max * G, ncb, items, grid)) return RUA_ERANGE;
  pt.table = page_table;
  pt.max_pages = max_pages;
  pt.num_pages = num_pages;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = {left < 0 ? -1 : left, right < 0 ? -1 : right, heads_kv, align_end != 0};
  seg_trace("seg_attn_paged_forward_kernel D=%d heads=%d kvheads=%d left=%lld right=%lld end=%d cols=%lld kind=%d fp8=%d "
            "page=%d pages=%lld table=%lld grid=%u", D, heads, heads_kv, (long long)bd.left, (long long)bd.right,
            bd.align_end, (long long)(T_max * G), LQ.kind, (int)f8, page_size, (long long)num_pages, (long long)max_pages,
            grid);
#define RUA_ATTN_PAGED(XX, DD, FF)                                                                                     \
  hipLaunchKernelGGL((seg_attn_paged_forward_kernel<XX, DD, FF>), dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK, pt,       \
                     (const uint16_t*)q_ptr, (const uint8_t*)k_ptr, (const uint8_t*)v_ptr, k_scale, v_scale,           \
                     (float)k_scale_by_value, (float)v_scale_by_value, (uint16_t*)out, (float*)lse, (int)heads,        \
                     (float)scale, ncb, items, bd)
#define RUA_ATTN_PAGED_16(XX, DD) RUA_ATTN_PAGED(XX, DD, false)
#define RUA_ATTN_PAGED_8(XX, DD) RUA_ATTN_PAGED(XX, DD, true)
  if (f8)
    RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_PAGED_8);
  else
    RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_PAGED_16);
#undef RUA_ATTN_PAGED_8
#undef RUA_ATTN_PAGED_16
#undef RUA_ATTN_PAGED
  return (int)hipGetLastError();
}
