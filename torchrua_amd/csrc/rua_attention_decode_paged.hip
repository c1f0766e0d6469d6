// rua_attention_decode_paged.hip — attention for decode steps over a PAGED KV cache (rua_segment_attention_decode_paged;
// include/rua.h).  K and V live in a pool [num_pages][page_size][heads_kv][D] (q's dtype, or OCP e4m3 codes
// with one fp32 scale per kv head) and a block table [B][max_pages] of int32 names the pages of every sequence: key s of
// sequence b is row  page_table[b][s >> lg] << lg | s & (page_size - 1)  of the pool, lg = log2 page_size.  The walks
// here are the siblings of seg_attn_decode_kernel and seg_attn_decode_fp8_kernel: the work item (sequence, kv head,
// column block, split), the packed columns, the four waves that divide every 128-key step, the band skip, the online
// softmax on the accumulator layout, hi + lo P for bf16, the transposed per-wave V tile ([D][40]; [D][36] for codes),
// the e4m3 converts and the d permutation of the fp8 walk, the scale folds, the fixed-order merge, the partial format
// and the combine kernel are theirs, and steps, sub-tiles and splits are cut by key POSITION from 0 as there — so for
// one kv_chunk the bits are those of the contiguous walk over the gathered cache.  The kv rua_layout supplies only the
// LENGTHS; what follows is what differs: how a key position becomes an address.
//
// ONE TEMPLATE, TWO WALKS.  A kv-head row is 32 NL bytes (NL = D / 16 for 16-bit elements, D / 32 for codes) and lane
// (j, g) takes the 16 bytes 32 st + 16 g .. + 15 of key ks + j in BOTH walks — for 16-bit elements these are the
// elements 16 st + 8 g .. + 7 of k-step st, for codes the 16 d of the fp8 walk's two k-steps — so one loader serves both;
// `F8` selects the convert, the q order, the V tile and the scales.
//
// ROW LOOKUP.  Lane (j, g) owns key ks + j of its sub-tile and reads ITS OWN 4-byte table entry, column (ks + j) >> lg,
// for every page size.  For page_size >= 32 the 32 keys of a sub-tile lie in one page and the entry is uniform over the
// wave; a scalar load at a readfirstlane'd index was built first and MEASURED SLOWER (page 128: 1.04 - 1.14 x the
// contiguous walk, against 0.87 - 1.00 x for the per-lane load; profiles/attention_decode_paged_probe.txt holds the
// latter).  Supposed cause, not verified: a scalar load is waited for on the counter the LDS accesses share, so the wait
// also drains the V tile's stores and reads; a vector load waits on the counter of the K / V loads it precedes anyway.
// The 64 lanes of the per-lane load hit one or two words of one cache line.
//
// THE TABLE IS KEPT OUT OF THE LOAD CHAIN.  The contiguous walks hide latency in one place: the K / V loads of the next
// sub-tile are issued right after the score MFMAs.  A table load in front of them would serialise two trips to memory
// per step.  So the entry of sub-tile ks + 2 x 128 is loaded when the K / V loads of ks + 128 are issued, and waits in
// ONE register (`pg_next`) for a whole step; the first two entries of a work item are loaded before the q operand.
//
// MEMORY SAFETY DOES NOT REST ON THE CALLER.  A table entry is read only for a column < max_pages and a key < S_b (so
// never at or past ceil(S_b / page_size)); a page id outside [0, num_pages) is never dereferenced: its keys and values
// are zero rows, like the keys past the end of a sequence.  The rows of a last page past S_b are not read either: V
// there must be zeros, not what the pool holds (a masked weight of exactly 0 times a NaN is a NaN).
//
// REGISTERS: profiles/attention_decode_paged_registers.txt (no scratch in any instantiation; D = 128 one wave per SIMD).
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include "rua_attention_paged_dev.h"

namespace rua {

// K and V of one key row: lane (j, g) takes the 16 bytes 32 st + 16 g .. + 15 of kv head hk, st = 0 .. NL - 1; row < 0:
// zeros (for codes 0x00 = +0)
template <int NL>
__device__ __forceinline__ void pg_load(int64_t row, int hk, int hkv, const uint8_t* __restrict__ k,
                                        const uint8_t* __restrict__ v, int g, uint4* kf, uint4* vf) {
  const int64_t at = (row * hkv + hk) * (int64_t)(32 * NL) + 16 * g;
#pragma unroll
  for (int st = 0; st < NL; ++st) {
    kf[st] = vf[st] = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) {
      kf[st] = *(const uint4*)(k + at + 32 * st);
      vf[st] = *(const uint4*)(v + at + 32 * st);
    }
  }
}

// ---------------------------------------------------------------- the walk: one (sequence, kv head, column block, split)
template <typename X, int D, bool F8>
__global__ __launch_bounds__(RUA_BLOCK) __attribute__((amdgpu_waves_per_eu(D <= 64 ? 2 : 1)))  // D = 128 would spill
void seg_attn_decode_paged_kernel(rua_layout LQ, rua_layout LK, dec_pages pt, const uint16_t* __restrict__ q,
                                  const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
                                  const float* __restrict__ k_scale, const float* __restrict__ v_scale, float k_mul,
                                  float v_mul, uint16_t* __restrict__ out, float* __restrict__ lse,
                                  float* __restrict__ ws, int heads, float scale, int64_t ncb, int64_t kv_chunk,
                                  int64_t n_split, int64_t items, attn_band bd) {
  constexpr int TS = F8 ? DEC8_TS : DEC_TS, NS = D / 16, ND = D / 32, NR = ND * 16, NL = F8 ? ND : NS;
  constexpr int V_BYTES = RUA_WAVES_PER_BLOCK * D * TS * 2, M_BYTES = (RUA_WAVES_PER_BLOCK - 1) * NR * RUA_WAVE * 4;
  __shared__ __attribute__((aligned(16))) uint8_t smem[V_BYTES > M_BYTES ? V_BYTES : M_BYTES];
  __shared__ float sM[RUA_WAVES_PER_BLOCK][DEC_COLS], sL[RUA_WAVES_PER_BLOCK][DEC_COLS];
  const int tid = (int)threadIdx.x, lane = tid & (RUA_WAVE - 1), j = lane & 31, g = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float NEG_INF = -__builtin_inff();
  uint16_t* sVt = (uint16_t*)smem + wv * (D * TS);             // this wave's transposed V tile
  float* sAcc = (float*)smem;                                  // after the walk: the states of the waves 1 .. 3
  const int hkv = bd.heads_kv, G = heads / hkv;

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t sp = item % n_split, i1 = item / n_split;
    const int64_t cb = i1 % ncb, i2 = i1 / ncb;
    const int hk = (int)(i2 % hkv);
    const int64_t b = i2 / hkv;
    const int64_t T = safe_len(LQ, b);
    if (cb == 0 && sp == 0)
      for (int gi = 0; gi < G; ++gi) attn_zero_padding<D>(LQ, b, T, hk * G + gi, heads, out, nullptr, lse, tid);
    if (cb * DEC_COLS >= T * G) continue;
    const int64_t S = safe_len(LK, b);
    const int64_t kbeg = sp * kv_chunk;
    if (n_split > 1 && kbeg >= S) continue;                     // (one split: it goes on and writes the zero rows)

    // the scales of this kv head (codes only): k's goes into the softmax scale, v's waits for the merged accumulator
    float sc = scale, vs = 1.f;
    if constexpr (F8) {
      sc = scale * ((k_scale ? k_scale[hk] : 1.f) * k_mul);
      vs = (v_scale ? v_scale[hk] : 1.f) * v_mul;
    }

    // the keys of the split that the block's queries t_lo .. t_hi may see, walked in steps cut by position from 0
    const int64_t c = cb * DEC_COLS + j, t = c / G;
    const int64_t shift = bd.align_end ? S - T : 0;
    const int64_t t_lo = cb * DEC_COLS / G, t_top = (cb * DEC_COLS + DEC_COLS - 1) / G, t_hi = t_top < T ? t_top : T - 1;
    const int64_t lo = attn_band_lo(t_lo + shift, bd.left), hi = attn_band_hi(t_hi + shift, bd.right, S);
    // the keys [see_lo, see_hi) that the lane's own query sees (the band and the end of the sequence, as positions)
    const int64_t see_lo = attn_band_lo(t + shift, bd.left), see_hi = attn_band_hi(t + shift, bd.right, S);
    int64_t kend = kbeg + kv_chunk < S ? kbeg + kv_chunk : S;
    if (hi < kend) kend = hi;
    const int64_t lo_step = lo / DEC_STEP * DEC_STEP;
    int64_t ks = (kbeg > lo_step ? kbeg : lo_step) + 32 * wv;   // this wave's first sub-tile ...
    if (ks + 31 < lo) ks += DEC_STEP;                           // ... that is not wholly left of the band

    // the table entries of the first two sub-tiles, ahead of everything else the work item loads
    const int32_t* __restrict__ tb = pt.table + b * pt.max_pages;
    const int32_t pg_first = pg_entry(pt, tb, S, ks, ks < kend, j);
    int32_t pg_next = pg_entry(pt, tb, S, ks + DEC_STEP, ks + DEC_STEP < kend, j);

    // the lane's column: query position t, head h; its q operand (codes: in the d order of the K loads), once per item
    const int h = hk * G + (int)(c % G);
    const int64_t qrow = t < T ? attn_row(LQ, b, t, T) : (int64_t)-1;
    uint4 qf[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      qf[st] = make_uint4(0u, 0u, 0u, 0u);
      const int d0 = F8 ? 32 * (st >> 1) + 16 * g + 8 * (st & 1) : 16 * st + 8 * g;
      if (qrow >= 0) qf[st] = *(const uint4*)(q + (qrow * heads + h) * (int64_t)D + d0);
    }
    attn_f32x16 acc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
    float m = NEG_INF, l = 0.f;

    uint4 kf[NL], vf[NL];
    pg_load<NL>(ks < kend ? pg_row(pt, pg_first, S, ks, j) : (int64_t)-1, hk, hkv, k, v, g, kf, vf);
    __syncthreads();                                            // the merge buffer of the item before is consumed
    while (ks < kend) {
      // V of this sub-tile, transposed (codes: converted first): token j of the rows this lane loaded
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if constexpr (F8) {
#pragma unroll
        for (int s = 0; s < ND; ++s) {
          const uint4 v0 = dec8_up<X>(vf[s].x, vf[s].y), v1 = dec8_up<X>(vf[s].z, vf[s].w);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            sVt[(32 * s + 16 * g + i) * TS + j] = attn_elem(v0, i);
            sVt[(32 * s + 16 * g + 8 + i) * TS + j] = attn_elem(v1, i);
          }
        }
      } else {
#pragma unroll
        for (int st = 0; st < NS; ++st)
#pragma unroll
          for (int i = 0; i < 8; ++i) sVt[(16 * st + 8 * g + i) * TS + j] = attn_elem(vf[st], i);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      attn_f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      if constexpr (F8) {
#pragma unroll
        for (int st = 0; st < ND; ++st) {
          s = X::mfma(dec8_up<X>(kf[st].x, kf[st].y), qf[2 * st], s);
          s = X::mfma(dec8_up<X>(kf[st].z, kf[st].w), qf[2 * st + 1], s);
        }
      } else {
#pragma unroll
        for (int st = 0; st < NS; ++st) s = X::mfma(kf[st], qf[st], s);
      }
      // the next sub-tile's K / V from the entry that has waited a step; the entry of the one after it sets out now
      const int64_t ksn = ks + DEC_STEP;
      pg_load<NL>(ksn < kend ? pg_row(pt, pg_next, S, ksn, j) : (int64_t)-1, hk, hkv, k, v, g, kf, vf);
      pg_next = pg_entry(pt, tb, S, ksn + DEC_STEP, ksn + DEC_STEP < kend, j);
      // the online softmax on the accumulator layout: the lane is the column, its registers are keys; the keys of the
      // sub-tile that the lane's query sees are the offsets [vlo, vhi)
      const int64_t dlo = see_lo - ks, dhi = see_hi - ks;
      const int vlo = dlo < 0 ? 0 : dlo > 32 ? 32 : (int)dlo, vhi = dhi < 0 ? 0 : dhi > 32 ? 32 : (int)dhi;
      float sv[16], mx = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = 8 * (r >> 2) + 4 * g + (r & 3);         // key ks + off
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
        psum += sv[r];                                          // l is summed from the unrounded p
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
        const uint4 a0 = attn_ld_t<TS>(sVt, 32 * dt + j, 0, 0, g), a1 = attn_ld_t<TS>(sVt, 32 * dt + j, 0, 1, g);
        acc[dt] = acc[dt] * alpha;
        acc[dt] = X::mfma(a0, pb0, acc[dt]);
        acc[dt] = X::mfma(a1, pb1, acc[dt]);
        if constexpr (X::SPLIT) {
          acc[dt] = X::mfma(a0, pl0, acc[dt]);
          acc[dt] = X::mfma(a1, pl1, acc[dt]);
        }
      }
      ks = ksn;
    }

    // the merge of the four waves, in the fixed order 0, 1, 2, 3 (m and l are the same in both halves of a column)
    if (g == 0) {
      sM[wv][j] = m;
      sL[wv][j] = l;
    }
    __syncthreads();                                            // every wave has left its V tile: smem is sAcc now
    float mstar = sM[0][j];
#pragma unroll
    for (int w = 1; w < RUA_WAVES_PER_BLOCK; ++w) mstar = fmaxf(mstar, sM[w][j]);
    const float f = dec_factor(m, mstar);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc[dt] = acc[dt] * f;
    if (wv > 0) {
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) sAcc[((wv - 1) * NR + dt * 16 + r) * RUA_WAVE + lane] = acc[dt][r];
    }
    __syncthreads();
    if (wv != 0 || qrow < 0) continue;
    float lstar = sL[0][j] * f;
#pragma unroll
    for (int w = 1; w < RUA_WAVES_PER_BLOCK; ++w) {
      lstar += sL[w][j] * dec_factor(sM[w][j], mstar);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] += sAcc[((w - 1) * NR + dt * 16 + r) * RUA_WAVE + lane];
    }
    if constexpr (F8) {
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) acc[dt] = acc[dt] * vs;   // v's scale, once, for the finish and the partial alike
    }
    if (n_split == 1) {                                         // a query without a visible key: zeros and lse = -inf
      attn_store_row<X, D>(acc, lstar > 0.f ? 1.f / lstar : 0.f, out + (qrow * heads + h) * (int64_t)D, g);
      if (g == 0) lse[qrow * heads + h] = lstar > 0.f ? mstar + logf(lstar) : NEG_INF;
    } else {                                                    // the unnormalised state of this column, to its slot
      float* slot = ws + item * (int64_t)(DEC_COLS * (D + 2));
      if (g == 0) {
        slot[j] = mstar;
        slot[DEC_COLS + j] = lstar;
      }
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          *(float4*)(slot + DEC_SLOT_HEAD + j * D + 32 * dt + 8 * r4 + 4 * g) =
              make_float4(acc[dt][4 * r4], acc[dt][4 * r4 + 1], acc[dt][4 * r4 + 2], acc[dt][4 * r4 + 3]);
    }
  }
}

}  // namespace rua

extern "C" int rua_segment_attention_decode_paged(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                                  const void* k_ptr, const void* v_ptr, void* out, void* lse, void* ws,
                                                  int64_t ws_bytes, int32_t heads, int32_t D, int32_t dtype,
                                                  int32_t heads_kv, int64_t left, int64_t right, int32_t align_end,
                                                  double scale, int64_t T_max, int64_t S_max, int64_t kv_chunk,
                                                  int32_t kv_dtype, const float* k_scale, const float* v_scale,
                                                  double k_scale_by_value, double v_scale_by_value,
                                                  const int32_t* page_table, int64_t max_pages, int32_t page_size,
                                                  int64_t num_pages, void* stream) {
  using namespace rua;
  int e;
  dec_launch L;
  dec_pages pt;
  bool f8;
  if ((e = pg_check_cache(kv_dtype, k_scale, v_scale, k_scale_by_value, v_scale_by_value, f8)) != 0) return e;
  if ((e = pg_check(q, heads_kv, D, f8 ? 1 : 2, k_ptr, v_ptr, page_table, max_pages, page_size, num_pages, S_max,
                    pt.lg)) != 0)
    return e;
  if ((e = dec_prepare(q, kv, q_ptr, k_ptr, v_ptr, out, lse, ws, ws_bytes, heads, D, dtype, heads_kv, left, right,
                       align_end, scale, T_max, S_max, kv_chunk, f8 ? 1 : 2, L)) != 0)
    return e;
  if (((uintptr_t)k_scale & 3) || ((uintptr_t)v_scale & 3)) return RUA_EALIGN;
  if (!L.run) return 0;
  pt.table = page_table;
  pt.max_pages = max_pages;
  pt.num_pages = num_pages;
  const dec_plan& p = L.p;
  const unsigned grid = L.grid;
  const int64_t items = L.items;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = L.bd;
  seg_trace("seg_attn_decode_paged_kernel D=%d heads=%d kvheads=%d left=%lld right=%lld end=%d cols=%lld chunk=%lld "
            "splits=%lld kind=%d fp8=%d page=%d pages=%lld table=%lld grid=%u", D, heads, heads_kv, (long long)bd.left,
            (long long)bd.right, bd.align_end, (long long)(T_max * (heads / heads_kv)), (long long)p.kv_chunk,
            (long long)p.n_split, LQ.kind, (int)f8, page_size, (long long)num_pages, (long long)max_pages, grid);
#define RUA_ATTN_DECODE_PAGED(XX, DD, FF)                                                                              \
  hipLaunchKernelGGL((seg_attn_decode_paged_kernel<XX, DD, FF>), dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK, pt,        \
                     (const uint16_t*)q_ptr, (const uint8_t*)k_ptr, (const uint8_t*)v_ptr, k_scale, v_scale,           \
                     (float)k_scale_by_value, (float)v_scale_by_value, (uint16_t*)out, (float*)lse, (float*)ws,        \
                     (int)heads, (float)scale, p.ncb, p.kv_chunk, p.n_split, items, bd)
#define RUA_ATTN_DECODE_PAGED_16(XX, DD) RUA_ATTN_DECODE_PAGED(XX, DD, false)
#define RUA_ATTN_DECODE_PAGED_8(XX, DD) RUA_ATTN_DECODE_PAGED(XX, DD, true)
  if (f8)
    RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DECODE_PAGED_8);
  else
    RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DECODE_PAGED_16);
#undef RUA_ATTN_DECODE_PAGED_8
#undef RUA_ATTN_DECODE_PAGED_16
#undef RUA_ATTN_DECODE_PAGED
  if ((e = (int)hipGetLastError()) != 0 || p.n_split == 1) return e;
  return dec_combine(q, kv, L, ws, out, lse, heads, D, dtype, heads_kv, T_max, s);
}
