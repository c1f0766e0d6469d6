// rua_attention_decode.hip — attention for DECODE steps over a ragged KV cache (rua_attention_decode_plan,
// rua_segment_attention_decode; include/rua.h).  An extension: the forward of rua_attention.hip's band form
// for sequences of at most 32 queries, forward only, as a split-KV kernel that packs the query heads of a kv group into
// the matrix columns.  A decode step reads every K / V byte once and does about 2 x heads x D MACs per key row; the
// flash-style forward reads the bytes G = heads / heads_kv times and ties its parallelism to B x heads.
//
// COLUMNS.  For sequence b and kv head hk the matrix columns are the pairs (query position t, head in group gi): column
// c = t G + gi is query head hk G + gi, for c < T_b G.  A column block is 32 consecutive columns, ncb = ceil(T_max G /
// 32) of them.  With T = 1 and G <= 32, or T = 4 and G = 8, the whole group is ONE block: its K / V rows are read once
// for all its heads.  Columns are cut by position and head, never by storage row: the bits do not depend on the layouts.
//
// WORK ITEM = (sequence, kv head, column block, split), the closed form item = ((b hkv + hk) ncb + cb) n_split + sp; a
// grid capped at DEC_MAX_GRID strides over the items.  Split sp owns the keys [sp kv_chunk, (sp + 1) kv_chunk) by
// POSITION from 0; a split that starts at or past S_b leaves at once, so does a column block at or past T_b G (after
// block 0 / split 0 wrote the zeros of the padding rows of an L / R result).
//
// INSIDE A WORKGROUP THE KEYS ARE DIVIDED, NOT THE QUERIES.  In each step of 128 keys wave w owns the 32 keys k0 + 32 w
// .. + 31 and keeps its own (m, l, acc[D / 32]) for the block's 32 columns.  The score tile is K Q^T as in the forward —
// K is the A operand, the packed q columns the B operand, loaded once per work item into registers — so the accumulator
// layout, the select-to--inf masking, m_use / alpha, hi + lo P for bf16 and the O^T accumulator are the forward's
// (rua_attention_dev.h); the band compare uses t = c / G per lane; a sub-tile wholly outside the band of the block's
// queries is skipped (the same bits as a wholly masked one).
//
// DATA MOVEMENT.  A K row is consumed by exactly one wave exactly once: the A operand goes straight from global memory
// into registers, 16 bytes per lane, token_to_row per key row, zeros past the end.  V arrives the same way — the same
// row, the same 16 bytes per lane — and is written TRANSPOSED into a per-wave LDS tile [D][32 + 8] with 2-byte stores:
// lane (j, g) owns token j, so the 32 lanes of a half write 32 consecutive tokens of one d (16 banks) and the two halves
// sit 8 d = 160 words apart (32 banks): no bank conflict, unlike attn_stage's (row, chunk) order.  The loads of the next
// sub-tile are issued once the score MFMAs have consumed the K registers, ahead of the softmax and the P V MFMAs of the
// current one.  Per-wave tiles: no __syncthreads() in the key loop; LDS serves a wave's accesses in order, a
// wavefront-scope fence keeps the compiler from reordering them.
//
// MERGE.  After the walk the four waves' (m, l, acc) are merged through LDS in the FIXED order wave 0, 1, 2, 3:
// m* = max m_i, f_i = exp(m_i - m*) (m* == -inf: f_i = 0 is SELECTED, never computed), l* = ((f_0 l_0 + f_1 l_1) +
// f_2 l_2) + f_3 l_3 and acc* likewise.  n_split == 1: wave 0 finishes in place — out = acc* / l* rounded once, lse = m*
// + log l*, zeros and -inf when l* == 0 — ONE launch.  n_split > 1: the unnormalised fp32 state of every LIVE column
// goes to its workspace slot (m[32], l[32], acc[32][D]), also when the band showed the split nothing (m = -inf, l = 0,
// zeros), and seg_attn_decode_combine_kernel — four d per lane — reads the splits sp = 0 .. ceil(S_b / kv_chunk) - 1 of
// its (query row, head) in ascending order, applies the same rule, rounds once and writes out and lse.  Every partial it
// reads was written in this call; no atomics, no tickets: bitwise reproducible.
//
// KNOWN LIMITS: V is transposed with 2-byte LDS stores (gfx950's transposing LDS read would take 16-byte stores; its lane
// mapping was not pinned down); with few live columns (T = 1, G = 4: 4 of 32) the matrix unit does mostly idle work —
// the kernel is bound by its K / V bytes; the merge buffer makes the LDS footprint 384 D bytes where the V tiles alone
// take 320 D.
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include "rua_attention_decode_dev.h"

namespace rua {

static_assert(DEC_STEP == 32 * RUA_WAVES_PER_BLOCK && DEC_COLS == 32, "a wave owns 32 keys of a step; a tile is 32 x 32");

// K (the A operand of the scores) and V (staged transposed below) of the 32 keys [ks, ks + 32): lane (j, g) takes the 16
// bytes 16 st + 8 g .. + 7 of key ks + j, st = 0 .. D / 16 - 1; zeros when the key is past the end or `on` is false
template <int D>
__device__ __forceinline__ void dec_load(const rua_layout& LK, int64_t b, int64_t S, int64_t ks, bool on, int hk, int hkv,
                                         const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int j, int g,
                                         uint4* kf, uint4* vf) {
  const int64_t row = on ? attn_row(LK, b, ks + j, S) : (int64_t)-1;
  const int64_t at = (row * hkv + hk) * (int64_t)D + 8 * g;
#pragma unroll
  for (int st = 0; st < D / 16; ++st) {
    kf[st] = vf[st] = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) {
      kf[st] = *(const uint4*)(k + at + 16 * st);
      vf[st] = *(const uint4*)(v + at + 16 * st);
    }
  }
}

// ---------------------------------------------------------------- the walk: one (sequence, kv head, column block, split)
template <typename X, int D>
__global__ __launch_bounds__(RUA_BLOCK) __attribute__((amdgpu_waves_per_eu(D <= 64 ? 2 : 1)))  // D = 128 would spill
void seg_attn_decode_kernel(rua_layout LQ, rua_layout LK,
                                                                    const uint16_t* __restrict__ q,
                                                                    const uint16_t* __restrict__ k,
                                                                    const uint16_t* __restrict__ v,
                                                                    uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                    float* __restrict__ ws, int heads, float scale,
                                                                    int64_t ncb, int64_t kv_chunk, int64_t n_split,
                                                                    int64_t items, attn_band bd) {
  constexpr int TS = DEC_TS, NS = D / 16, ND = D / 32, NR = ND * 16;
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

    // the lane's column: query position t, head h; its q operand, once per work item
    const int64_t c = cb * DEC_COLS + j, t = c / G;
    const int h = hk * G + (int)(c % G);
    const int64_t qrow = t < T ? attn_row(LQ, b, t, T) : (int64_t)-1;
    uint4 qf[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      qf[st] = make_uint4(0u, 0u, 0u, 0u);
      if (qrow >= 0) qf[st] = *(const uint4*)(q + (qrow * heads + h) * (int64_t)D + 16 * st + 8 * g);
    }
    attn_f32x16 acc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
    float m = NEG_INF, l = 0.f;

    // the keys of the split that the block's queries t_lo .. t_hi may see, walked in steps cut by position from 0
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

    uint4 kf[NS], vf[NS];
    dec_load<D>(LK, b, S, ks, ks < kend, hk, hkv, k, v, j, g, kf, vf);
    __syncthreads();                                            // the merge buffer of the item before is consumed
    while (ks < kend) {
      // V of this sub-tile, transposed: token j of row d
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int st = 0; st < NS; ++st)
#pragma unroll
        for (int i = 0; i < 8; ++i) sVt[(16 * st + 8 * g + i) * TS + j] = attn_elem(vf[st], i);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      attn_f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int st = 0; st < NS; ++st) s = X::mfma(kf[st], qf[st], s);
      const int64_t ksn = ks + DEC_STEP;
      dec_load<D>(LK, b, S, ksn, ksn < kend, hk, hkv, k, v, j, g, kf, vf);
      // the online softmax on the accumulator layout: the lane is the column, its registers are keys; the keys of the
      // sub-tile that the lane's query sees are the offsets [vlo, vhi)
      const int64_t dlo = see_lo - ks, dhi = see_hi - ks;
      const int vlo = dlo < 0 ? 0 : dlo > 32 ? 32 : (int)dlo, vhi = dhi < 0 ? 0 : dhi > 32 ? 32 : (int)dhi;
      float sv[16], mx = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = 8 * (r >> 2) + 4 * g + (r & 3);         // key ks + off
        sv[r] = (off >= vlo && off < vhi) ? s[r] * scale : NEG_INF;
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

// ---------------------------------------------------------------- the combine: a (query row, head) per D / 4 lanes
template <typename X, int D>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_decode_combine_kernel(rua_layout LQ, rua_layout LK,
                                                                            const float* __restrict__ ws,
                                                                            uint16_t* __restrict__ out,
                                                                            float* __restrict__ lse, int heads, int hkv,
                                                                            int64_t T_max, int64_t ncb, int64_t kv_chunk,
                                                                            int64_t n_split, int64_t pairs) {
  constexpr int LPP = D / 4, SLOT = DEC_COLS * (D + 2);
  const int64_t idx = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x, pair = idx / LPP;
  const int dl = (int)(idx % LPP);
  if (pair >= pairs) return;
  const int h = (int)(pair % heads);
  const int64_t t = pair / heads % T_max, b = pair / heads / T_max;
  const int64_t T = safe_len(LQ, b);
  if (t >= T) return;
  const int64_t row = attn_row(LQ, b, t, T);
  const int G = heads / hkv;
  const int64_t c = t * G + h % G, cb = c / DEC_COLS;
  if (row < 0 || cb >= ncb) return;
  const int j = (int)(c % DEC_COLS);
  const int64_t S = safe_len(LK, b);
  int64_t nsp = S > 0 ? (S - 1) / kv_chunk + 1 : 0;             // the splits that wrote: sp kv_chunk < S
  if (nsp > n_split) nsp = n_split;
  const float* slot = ws + (((b * hkv + h / G) * ncb + cb) * n_split) * (int64_t)SLOT;
  const float NEG_INF = -__builtin_inff();

  float mstar = NEG_INF;
  for (int64_t sp = 0; sp < nsp; ++sp) mstar = fmaxf(mstar, slot[sp * SLOT + j]);
  float lstar = 0.f, a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t sp = 0; sp < nsp; ++sp) {
    const float* p = slot + sp * SLOT;
    const float f = dec_factor(p[j], mstar);
    const float4 x = *(const float4*)(p + DEC_SLOT_HEAD + j * D + 4 * dl);
    lstar += p[DEC_COLS + j] * f;
    a[0] += x.x * f;
    a[1] += x.y * f;
    a[2] += x.z * f;
    a[3] += x.w * f;
  }
  const float inv = lstar > 0.f ? 1.f / lstar : 0.f;
  const uint32_t w0 = (uint32_t)X::down(a[0] * inv) | ((uint32_t)X::down(a[1] * inv) << 16);
  const uint32_t w1 = (uint32_t)X::down(a[2] * inv) | ((uint32_t)X::down(a[3] * inv) << 16);
  *(uint2*)(out + (row * heads + h) * (int64_t)D + 4 * dl) = make_uint2(w0, w1);
  if (dl == 0) lse[row * heads + h] = lstar > 0.f ? mstar + logf(lstar) : NEG_INF;
}

int dec_prepare(const rua_layout* q, const rua_layout* kv, const void* q_ptr, const void* k_ptr, const void* v_ptr,
                const void* out, const void* lse, const void* ws, int64_t ws_bytes, int32_t heads, int32_t D,
                int32_t dtype, int32_t heads_kv, int64_t left, int64_t right, int32_t align_end, double scale,
                int64_t T_max, int64_t S_max, int64_t kv_chunk, int kv_es, dec_launch& L) {
  int e;
  dec_plan& p = L.p;
  L.run = false;
  if ((e = attn_check_entry(q, kv, heads, heads_kv, D, dtype, scale, T_max)) != 0) return e;
  if (S_max < 0 || T_max > DEC_MAX_T || kv_chunk <= 0 || kv_chunk % DEC_STEP != 0) return RUA_EINVAL;
  if ((e = dec_make_plan(q->B, heads, heads_kv, D, T_max, S_max, kv_chunk, p)) != 0) return e;
  if (ws_bytes < p.ws_bytes || (p.ws_bytes > 0 && !ws)) return RUA_EINVAL;
  if (q->B == 0) return 0;
  const bool padded = q->kind == RUA_LEFT || q->kind == RUA_RIGHT;
  if (T_max == 0) {                                             // nothing but the padding zeros of an L / R result
    if (!padded || q->n_rows == 0) return 0;
    p.ncb = 1;
    p.n_split = 1;
  }
  if ((q->n_rows > 0 && (!q_ptr || !out || !lse)) || (kv->n_rows > 0 && (!k_ptr || !v_ptr))) return RUA_EINVAL;
  if (attn_misaligned(q_ptr) || attn_misaligned(k_ptr) || attn_misaligned(v_ptr) || attn_misaligned(out) ||
      attn_misaligned(ws) || ((uintptr_t)lse & 3))
    return RUA_EALIGN;
  if (seg_too_large(q, (int64_t)heads * D, 2) || seg_too_large(kv, (int64_t)heads_kv * D, kv_es)) return RUA_ERANGE;
  if ((double)q->B * (double)heads_kv * (double)p.ncb * (double)p.n_split >= 4.0e18) return RUA_ERANGE;
  L.items = q->B * heads_kv * p.ncb * p.n_split;
  L.grid = (unsigned)(L.items < DEC_MAX_GRID ? L.items : DEC_MAX_GRID);
  L.pairs = q->B * T_max * heads;
  L.cgrid = (L.pairs * (D / 4) + RUA_BLOCK - 1) / RUA_BLOCK;
  if (p.n_split > 1 && L.cgrid > 0x7fffffffLL) return RUA_ERANGE;
  L.bd = {left < 0 ? -1 : left, right < 0 ? -1 : right, heads_kv, align_end != 0};
  L.run = true;
  return 0;
}

int dec_combine(const rua_layout* q, const rua_layout* kv, const dec_launch& L, const void* ws, void* out, void* lse,
                int32_t heads, int32_t D, int32_t dtype, int32_t heads_kv, int64_t T_max, hipStream_t s) {
  const rua_layout LQ = *q, LK = *kv;
  const dec_plan& p = L.p;
  seg_trace("seg_attn_decode_combine_kernel D=%d heads=%d kvheads=%d chunk=%lld splits=%lld grid=%lld", D, heads, heads_kv,
            (long long)p.kv_chunk, (long long)p.n_split, (long long)L.cgrid);
#define RUA_ATTN_COMBINE(XX, DD)                                                                                       \
  hipLaunchKernelGGL((seg_attn_decode_combine_kernel<XX, DD>), dim3((unsigned)L.cgrid), dim3(RUA_BLOCK), 0, s, LQ, LK, \
                     (const float*)ws, (uint16_t*)out, (float*)lse, (int)heads, (int)heads_kv, T_max, p.ncb,           \
                     p.kv_chunk, p.n_split, L.pairs)
  RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_COMBINE);
#undef RUA_ATTN_COMBINE
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int rua_attention_decode_plan(int64_t B, int32_t heads, int32_t heads_kv, int32_t D, int64_t T_max,
                                         int64_t S_max, int64_t kv_chunk_in, int64_t* kv_chunk, int64_t* n_split,
                                         int64_t* ws_bytes) {
  rua::dec_plan p;
  const int e = rua::dec_make_plan(B, heads, heads_kv, D, T_max, S_max, kv_chunk_in, p);
  if (e != 0) return e;
  if (kv_chunk) *kv_chunk = p.kv_chunk;
  if (n_split) *n_split = p.n_split;
  if (ws_bytes) *ws_bytes = p.ws_bytes;
  return 0;
}

extern "C" int rua_segment_attention_decode(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                            const void* k_ptr, const void* v_ptr, void* out, void* lse, void* ws,
                                            int64_t ws_bytes, int32_t heads, int32_t D, int32_t dtype, int32_t heads_kv,
                                            int64_t left, int64_t right, int32_t align_end, double scale, int64_t T_max,
                                            int64_t S_max, int64_t kv_chunk, void* stream) {
  using namespace rua;
  int e;
  dec_launch L;
  if ((e = dec_prepare(q, kv, q_ptr, k_ptr, v_ptr, out, lse, ws, ws_bytes, heads, D, dtype, heads_kv, left, right,
                       align_end, scale, T_max, S_max, kv_chunk, 2, L)) != 0 || !L.run)
    return e;
  const dec_plan& p = L.p;
  const unsigned grid = L.grid;
  const int64_t items = L.items;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = L.bd;
  seg_trace("seg_attn_decode_kernel D=%d heads=%d kvheads=%d left=%lld right=%lld end=%d cols=%lld chunk=%lld splits=%lld "
            "kind=%d kvkind=%d grid=%u", D, heads, heads_kv, (long long)bd.left, (long long)bd.right, bd.align_end,
            (long long)(T_max * (heads / heads_kv)), (long long)p.kv_chunk, (long long)p.n_split, LQ.kind, LK.kind, grid);
#define RUA_ATTN_DECODE(XX, DD)                                                                                        \
  hipLaunchKernelGGL((seg_attn_decode_kernel<XX, DD>), dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK,                      \
                     (const uint16_t*)q_ptr, (const uint16_t*)k_ptr, (const uint16_t*)v_ptr, (uint16_t*)out,           \
                     (float*)lse, (float*)ws, (int)heads, (float)scale, p.ncb, p.kv_chunk, p.n_split, items, bd)
  RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DECODE);
#undef RUA_ATTN_DECODE
  if ((e = (int)hipGetLastError()) != 0 || p.n_split == 1) return e;
  return dec_combine(q, kv, L, ws, out, lse, heads, D, dtype, heads_kv, T_max, s);
}
