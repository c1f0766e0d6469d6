// rua_attention.hip — attention inside every sequence of a ragged batch, over unpadded storage (rua_segment_attention_forward,
// rua_segment_attention_backward; include/rua.h).  An extension, and the first contraction of the library:
//
//   out[t, h, :] = sum_s softmax_s(scale * q[t, h, :] . k[s, h, :]) * v[s, h, :]      over the kv tokens of the SAME sequence
//
// `q` lives in one C / L / P / R layout, `k` and `v` in another; both layouts travel by value and sequence b is the same
// sequence in both (token_to_row resolves a P through `unsorted`).  bf16 / f16 payloads, D = 32 / 64 / 128, fp32
// accumulation on the gfx950 matrix unit (v_mfma_f32_32x32x16_bf16 / _f16).
//
// Tiles are cut by token POSITION inside the sequence, counted from 0, never by storage row: the bits of every result are
// the same for all 4 x 4 pairs of layouts.
//
// THE TRANSPOSED SCORE TILE.  Every kernel computes its 32 x 32 score tile with the STAGED side as the A operand and the
// side the wave owns as the B operand, so that the accumulator layout (lane = column, 16 registers = rows
// 8 (r / 4) + 4 (lane / 32) + r % 4) puts the wave's own token on the LANE: in the forward and the dQ kernel a lane is a
// query and its 16 registers are keys, in the dK / dV kernel a lane is a key and its registers are queries.  Then
//   - the softmax of a query is a fold over the lane's own registers and ONE exchange with lane ^ 32;
//   - the running max, the running sum, lse and delta of the wave's own token are one register each;
//   - the rounded tile (P, dS) is ALREADY the B operand of the second contraction: its 8 k-entries per lane are the
//     registers 8 c .. 8 c + 7 — the rows 16 c + 8 (e / 4) + 4 (lane / 32) + e % 4 — and because a contraction does not
//     care in which order it meets k, the A operand is simply read in the same order: two 8-byte LDS reads per lane from a
//     tile that was staged TRANSPOSED ([d][token], tokens contiguous).  No cross-lane shuffle of P exists.
//   - the output accumulator (O^T, dQ^T, dK^T, dV^T: rows d, column = the wave's token) is rescaled by a per-lane scalar
//     and written as 4 consecutive d (8 bytes) per register quad.
//
// Geometry.  A workgroup is 4 waves; a wave owns 32 consecutive positions of the 128 of its work item (sequence, head,
// block).  The other side is walked in tiles staged in LDS once per workgroup, every row gathered through token_to_row,
// rows past the end staged as zeros.  LDS rows are padded by 16 bytes (plain: D + 8 elements; transposed: tokens + 8), so
// that the 16-byte and 8-byte operand reads of a wave fall on distinct banks.  Work items come from the closed form
// (b, h, block) = unflatten(item; B, heads, ceil(max / 128)); a capped grid strides over them; a block past its
// sequence's end leaves at once (after block 0 wrote the zeros of the padding rows of an L / R result).
//
// Ragged edges.  Keys past the end, queries past the end and keys above the causal diagonal are SELECTED away (-inf
// before the max in the forward, 0 in place of exp in the backward), never multiplied by zero.  Causal tiles wholly above
// the diagonal of the block are not visited, tiles wholly above the diagonal of a wave are skipped by that wave.  Waves
// whose 32 positions lie past the end skip their MFMAs and still help to stage.
//
// Backward: delta[t, h] = sum_d dO * O (fp32, from the SAVED rounded output), then P is recomputed from lse:
//   dK / dV kernel   (sequence, head, key block) walks the query tiles:  dV += P~^T dO,  dS = P o (dO V^T - delta) rounded
//                    once,  dK += dS^T Q,  times scale at the end;
//   dQ kernel        (sequence, head, query block) walks the key tiles:  dQ += dS K,  times scale at the end.
// Every gradient row is written exactly once, no atomics: bitwise reproducible.
//
// bf16 ONLY: P meets V (forward) and dO (dV) as hi + lo — P rounded once, and what that rounding left behind, exact in
// fp32, rounded again — through two MFMAs on the same A operand.  bf16 keeps 8 significant bits, so a weight rounded to
// it alone is off by up to 2^-8, as much as the rounding of the result itself; at rows with few keys the two together
// exceed one ulp of the result.  f16 (11 bits) takes the single MFMA.  dS is rounded once in both types.
//
// THE BAND FORM (rua_segment_attention_band_*; the BAND switch of the same three templates).  Query t sees key s iff
// -left <= s - (t + shift) <= right, shift = S - T under end alignment, and query head h reads kv head h / G, G = heads /
// heads_kv.  It parametrises the walk and nothing else: the forward and the dQ kernel visit only the key tiles between
// the band edges of their block of 128 queries, the first rounded down to a multiple of 64 so that tiles stay cut by
// position from 0; a wave skips a 32-key sub-tile wholly outside the band of its own 32 queries, on either side; every
// other key outside the band is selected away like the causal diagonal.  A skipped tile and a wholly masked tile give the
// same bits (m_use / alpha below), so the plain form's bits come out wherever the masks coincide.  K / V rows are staged
// from head h / G with row stride heads_kv x D.  The dK / dV kernel works over (sequence, KV head, key block): its
// accumulators stay in registers over the G query heads of the group in ascending order, and for each over the query
// tiles that can see the block in ascending order; every dK / dV row is stored once — no atomics, no workspace, a fixed
// order of adds.  A query without a visible key (an empty band) gets zeros, lse = -inf and zero gradients.
//
// KNOWN LIMITS: the transposed tiles are written to LDS with 2-byte stores.  One workgroup walks all the visible keys of
// a (sequence, head, query block), the query heads of a group stage the same K / V tile once each in the forward, and a
// sequence with a handful of queries still fills a 128-query block: decode steps (at most 32 queries per sequence) have
// a kernel of their own that splits the keys and packs a group's heads into the matrix columns —
// rua_attention_decode.hip, rua_segment_attention_decode; these kernels never dispatch to it.
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include "rua_attention_dev.h"

namespace rua {

// ---------------------------------------------------------------- forward: one flash-style pass
template <typename X, int D, bool CAUSAL, bool BAND = false>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_forward_kernel(rua_layout LQ, rua_layout LK,
                                                                     const uint16_t* __restrict__ q,
                                                                     const uint16_t* __restrict__ k,
                                                                     const uint16_t* __restrict__ v,
                                                                     uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                     int heads, float scale, int64_t nblk, int64_t items,
                                                                     attn_band bd) {
  constexpr int PS = D + 8, TS = ATTN_KB + 8, NS = D / 16, ND = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t sK[ATTN_KB * PS];
  __shared__ __attribute__((aligned(16))) uint16_t sVt[D * TS];
  const int tid = (int)threadIdx.x, lane = tid & (RUA_WAVE - 1), j = lane & 31, g = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float NEG_INF = -__builtin_inff();

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t blk = item % nblk, bh = item / nblk;
    const int h = (int)(bh % heads);
    const int64_t b = bh / heads;
    const int64_t T = safe_len(LQ, b);
    if (blk == 0) attn_zero_padding<D>(LQ, b, T, h, heads, out, nullptr, lse, tid);
    const int64_t q0 = blk * ATTN_BLOCK_TOK;
    if (q0 >= T) continue;
    const int64_t S = safe_len(LK, b);
    const int64_t w0 = q0 + wv * 32, tq = w0 + j;
    const bool live = w0 < T;
    const int64_t qrow = attn_row(LQ, b, tq, T);

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

    // the kv head and the heads of a kv row; the keys the block may see, walked in tiles cut by position from 0 (an
    // empty band: no tile, and the zero rows and lse = -inf below)
    const int hkv = BAND ? bd.heads_kv : heads, hk = BAND ? h / (heads / hkv) : h;
    const int64_t shift = (BAND && bd.align_end) ? S - T : 0;
    const int64_t kbeg = BAND ? attn_band_lo(q0 + shift, bd.left) / ATTN_KB * ATTN_KB : 0;
    const int64_t kend = BAND ? attn_band_hi(q0 + ATTN_BLOCK_TOK - 1 + shift, bd.right, S) : attn_key_end<CAUSAL>(S, q0);
    for (int64_t k0 = kbeg; k0 < kend; k0 += ATTN_KB) {
      __syncthreads();                                          // the tile before is consumed
      attn_stage<D, ATTN_KB, true, false>(LK, b, S, k0, hk, hkv, k, sK, nullptr, tid);
      attn_stage<D, ATTN_KB, false, true>(LK, b, S, k0, hk, hkv, v, nullptr, sVt, tid);
      __syncthreads();
      if (!live) continue;
#pragma unroll
      for (int sub = 0; sub < ATTN_KB / 32; ++sub) {
        const int64_t ks = k0 + 32 * sub;
        if (ks >= kend || (CAUSAL && ks > w0 + 31)) break;      // past the end, or wholly above the wave's diagonal
        if constexpr (BAND) {                                   // wholly right / left of the band of the wave's queries
          if (bd.right >= 0 && ks - (w0 + 31 + shift) > bd.right) break;
          if (bd.left >= 0 && ks + 31 - (w0 + shift) < -bd.left) continue;
        }
        attn_f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int st = 0; st < NS; ++st)
          s = X::mfma(*(const uint4*)(sK + (32 * sub + j) * PS + 16 * st + 8 * g), qf[st], s);
        // the online softmax on the accumulator layout: the lane is the query, its registers are keys
        float sv[16], mx = NEG_INF;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t key = ks + 8 * (r >> 2) + 4 * g + (r & 3);
          const bool ok = key < S && (!CAUSAL || key <= tq) && (!BAND || attn_band_sees(bd, key - (tq + shift)));
          sv[r] = ok ? s[r] * scale : NEG_INF;
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
          psum += sv[r];                                        // l is summed from the unrounded p
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

    if (qrow >= 0) {                                            // a query without a visible key: zeros and lse = -inf
      attn_store_row<X, D>(acc, l > 0.f ? 1.f / l : 0.f, out + (qrow * heads + h) * (int64_t)D, g);
      if (g == 0) lse[qrow * heads + h] = l > 0.f ? m + logf(l) : NEG_INF;
    }
  }
}

// ---------------------------------------------------------------- backward 1: delta = sum_d dO * O, a thread per (row, head)
template <typename X, int D>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_delta_kernel(const uint16_t* __restrict__ o,
                                                                   const uint16_t* __restrict__ go,
                                                                   float* __restrict__ delta, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const uint4 a = *(const uint4*)(o + i * D + 8 * c), bq = *(const uint4*)(go + i * D + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += X::up(attn_elem(a, e)) * X::up(attn_elem(bq, e));
  }
  delta[i] = acc;
}

// ---------------------------------------------------------------- backward 2: dK and dV, a lane is a key
// BAND: the work item is (sequence, KV head, key block).  The accumulators stay in registers across the whole group: the
// query heads hk G .. hk G + G - 1 of the kv head in ASCENDING order, and for each the query tiles that can see the block
// in ascending order — a fixed order of fp32 adds, so the sum over the group is reproducible and is rounded once.
template <typename X, int D, bool CAUSAL, bool BAND = false>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_dkdv_kernel(rua_layout LQ, rua_layout LK,
                                                                  const uint16_t* __restrict__ q,
                                                                  const uint16_t* __restrict__ k,
                                                                  const uint16_t* __restrict__ v,
                                                                  const uint16_t* __restrict__ go,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ delta,
                                                                  uint16_t* __restrict__ gk, uint16_t* __restrict__ gv,
                                                                  int heads, float scale, int64_t nblk, int64_t items,
                                                                  attn_band bd) {
  constexpr int PS = D + 8, TS = ATTN_QB + 8, NS = D / 16, ND = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t sQ[ATTN_QB * PS];
  __shared__ __attribute__((aligned(16))) uint16_t sQt[D * TS];
  __shared__ __attribute__((aligned(16))) uint16_t sG[ATTN_QB * PS];
  __shared__ __attribute__((aligned(16))) uint16_t sGt[D * TS];
  __shared__ float sLse[ATTN_QB], sDelta[ATTN_QB];
  const int tid = (int)threadIdx.x, lane = tid & (RUA_WAVE - 1), j = lane & 31, g = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int hkv = BAND ? bd.heads_kv : heads, G = BAND ? heads / hkv : 1;   // the heads of a kv row; the group
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t blk = item % nblk, bh = item / nblk;
    const int hk = (int)(bh % hkv);
    const int64_t b = bh / hkv;
    const int64_t S = safe_len(LK, b);
    if (blk == 0) attn_zero_padding<D>(LK, b, S, hk, hkv, gk, gv, nullptr, tid);
    const int64_t k0 = blk * ATTN_BLOCK_TOK;
    if (k0 >= S) continue;
    const int64_t T = safe_len(LQ, b);
    const int64_t w0 = k0 + wv * 32, key = w0 + j;
    const bool live = w0 < S;
    const int64_t krow = attn_row(LK, b, key, S);

    uint4 kf[NS], vf[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      kf[st] = vf[st] = make_uint4(0u, 0u, 0u, 0u);
      if (krow >= 0) {
        kf[st] = *(const uint4*)(k + (krow * hkv + hk) * (int64_t)D + 16 * st + 8 * g);
        vf[st] = *(const uint4*)(v + (krow * hkv + hk) * (int64_t)D + 16 * st + 8 * g);
      }
    }
    attn_f32x16 dk[ND], dv[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;

    // the queries that can see the block (under `causal` those below its first key see none of its keys), in tiles cut
    // by position from 0
    const int64_t shift = (BAND && bd.align_end) ? S - T : 0;
    const int64_t tbeg = BAND ? attn_band_lo(k0 - shift, bd.right) / ATTN_QB * ATTN_QB : (CAUSAL ? k0 : 0);
    const int64_t tend = BAND ? attn_band_hi(k0 + ATTN_BLOCK_TOK - 1 - shift, bd.left, T) : T;
    for (int gi = 0; gi < G; ++gi) {
      const int h = hk * G + gi;
      for (int64_t t0 = tbeg; t0 < tend; t0 += ATTN_QB) {
        __syncthreads();
        attn_stage<D, ATTN_QB, true, true>(LQ, b, T, t0, h, heads, q, sQ, sQt, tid);
        attn_stage<D, ATTN_QB, true, true>(LQ, b, T, t0, h, heads, go, sG, sGt, tid);
        if (tid < ATTN_QB) {
          const int64_t row = attn_row(LQ, b, t0 + tid, T);
          sLse[tid] = row >= 0 ? lse[row * heads + h] : 0.f;
          sDelta[tid] = row >= 0 ? delta[row * heads + h] : 0.f;
        }
        __syncthreads();
        if (!live || (CAUSAL && t0 + ATTN_QB - 1 < w0)) continue;  // wholly above the wave's diagonal
        if constexpr (BAND) {                                     // wholly outside the band of the wave's keys
          if (bd.right >= 0 && w0 - (t0 + ATTN_QB - 1 + shift) > bd.right) continue;
          if (bd.left >= 0 && w0 + 31 - (t0 + shift) < -bd.left) continue;
        }
        attn_f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
          s = X::mfma(*(const uint4*)(sQ + j * PS + 16 * st + 8 * g), kf[st], s);
          dp = X::mfma(*(const uint4*)(sG + j * PS + 16 * st + 8 * g), vf[st], dp);
        }
        float p[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 8 * (r >> 2) + 4 * g + (r & 3);           // the query of this register
          const int64_t t = t0 + i;
          const bool ok = t < T && key < S && (!CAUSAL || key <= t) && (!BAND || attn_band_sees(bd, key - (t + shift)));
          p[r] = ok ? expf(s[r] * scale - sLse[i]) : 0.f;
          ds[r] = ok ? p[r] * (dp[r] - sDelta[i]) : 0.f;
        }
        const uint4 db0 = attn_pack8<X>(ds), db1 = attn_pack8<X>(ds + 8);
        const uint4 pb0 = attn_pack8<X>(p), pb1 = attn_pack8<X>(p + 8);
        uint4 pl0 = pb0, pl1 = pb1;
        if constexpr (X::SPLIT) {
          pl0 = attn_pack8_lo<X>(p);
          pl1 = attn_pack8_lo<X>(p + 8);
        }
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const uint4 g0 = attn_ld_t<TS>(sGt, 32 * dt + j, 0, 0, g), g1 = attn_ld_t<TS>(sGt, 32 * dt + j, 0, 1, g);
          dv[dt] = X::mfma(g0, pb0, dv[dt]);
          dv[dt] = X::mfma(g1, pb1, dv[dt]);
          if constexpr (X::SPLIT) {
            dv[dt] = X::mfma(g0, pl0, dv[dt]);
            dv[dt] = X::mfma(g1, pl1, dv[dt]);
          }
          dk[dt] = X::mfma(attn_ld_t<TS>(sQt, 32 * dt + j, 0, 0, g), db0, dk[dt]);
          dk[dt] = X::mfma(attn_ld_t<TS>(sQt, 32 * dt + j, 0, 1, g), db1, dk[dt]);
        }
      }
    }

    if (krow >= 0) {
      attn_store_row<X, D>(dk, scale, gk + (krow * hkv + hk) * (int64_t)D, g);
      attn_store_row<X, D>(dv, 1.f, gv + (krow * hkv + hk) * (int64_t)D, g);
    }
  }
}

// ---------------------------------------------------------------- backward 3: dQ, a lane is a query
template <typename X, int D, bool CAUSAL, bool BAND = false>
__global__ __launch_bounds__(RUA_BLOCK) void seg_attn_dq_kernel(rua_layout LQ, rua_layout LK,
                                                                const uint16_t* __restrict__ q,
                                                                const uint16_t* __restrict__ k,
                                                                const uint16_t* __restrict__ v,
                                                                const uint16_t* __restrict__ go,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ delta,
                                                                uint16_t* __restrict__ gq, int heads, float scale,
                                                                int64_t nblk, int64_t items, attn_band bd) {
  constexpr int PS = D + 8, TS = ATTN_KB + 8, NS = D / 16, ND = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t sK[ATTN_KB * PS];
  __shared__ __attribute__((aligned(16))) uint16_t sKt[D * TS];
  __shared__ __attribute__((aligned(16))) uint16_t sV[ATTN_KB * PS];
  const int tid = (int)threadIdx.x, lane = tid & (RUA_WAVE - 1), j = lane & 31, g = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t blk = item % nblk, bh = item / nblk;
    const int h = (int)(bh % heads);
    const int64_t b = bh / heads;
    const int64_t T = safe_len(LQ, b);
    if (blk == 0) attn_zero_padding<D>(LQ, b, T, h, heads, gq, nullptr, nullptr, tid);
    const int64_t q0 = blk * ATTN_BLOCK_TOK;
    if (q0 >= T) continue;
    const int64_t S = safe_len(LK, b);
    const int64_t w0 = q0 + wv * 32, tq = w0 + j;
    const bool live = w0 < T;
    const int64_t qrow = attn_row(LQ, b, tq, T);

    uint4 qf[NS], gf[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      qf[st] = gf[st] = make_uint4(0u, 0u, 0u, 0u);
      if (qrow >= 0) {
        qf[st] = *(const uint4*)(q + (qrow * heads + h) * (int64_t)D + 16 * st + 8 * g);
        gf[st] = *(const uint4*)(go + (qrow * heads + h) * (int64_t)D + 16 * st + 8 * g);
      }
    }
    const float my_lse = qrow >= 0 ? lse[qrow * heads + h] : 0.f;
    const float my_delta = qrow >= 0 ? delta[qrow * heads + h] : 0.f;
    attn_f32x16 dq[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;

    // the same walk as the forward's
    const int hkv = BAND ? bd.heads_kv : heads, hk = BAND ? h / (heads / hkv) : h;
    const int64_t shift = (BAND && bd.align_end) ? S - T : 0;
    const int64_t kbeg = BAND ? attn_band_lo(q0 + shift, bd.left) / ATTN_KB * ATTN_KB : 0;
    const int64_t kend = BAND ? attn_band_hi(q0 + ATTN_BLOCK_TOK - 1 + shift, bd.right, S) : attn_key_end<CAUSAL>(S, q0);
    for (int64_t k0 = kbeg; k0 < kend; k0 += ATTN_KB) {
      __syncthreads();
      attn_stage<D, ATTN_KB, true, true>(LK, b, S, k0, hk, hkv, k, sK, sKt, tid);
      attn_stage<D, ATTN_KB, true, false>(LK, b, S, k0, hk, hkv, v, sV, nullptr, tid);
      __syncthreads();
      if (!live) continue;
#pragma unroll
      for (int sub = 0; sub < ATTN_KB / 32; ++sub) {
        const int64_t ks = k0 + 32 * sub;
        if (ks >= kend || (CAUSAL && ks > w0 + 31)) break;
        if constexpr (BAND) {
          if (bd.right >= 0 && ks - (w0 + 31 + shift) > bd.right) break;
          if (bd.left >= 0 && ks + 31 - (w0 + shift) < -bd.left) continue;
        }
        attn_f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
          s = X::mfma(*(const uint4*)(sK + (32 * sub + j) * PS + 16 * st + 8 * g), qf[st], s);
          dp = X::mfma(*(const uint4*)(sV + (32 * sub + j) * PS + 16 * st + 8 * g), gf[st], dp);
        }
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t key = ks + 8 * (r >> 2) + 4 * g + (r & 3);
          const bool ok = qrow >= 0 && key < S && (!CAUSAL || key <= tq) && (!BAND || attn_band_sees(bd, key - (tq + shift)));
          ds[r] = ok ? expf(s[r] * scale - my_lse) * (dp[r] - my_delta) : 0.f;
        }
        const uint4 db0 = attn_pack8<X>(ds), db1 = attn_pack8<X>(ds + 8);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          dq[dt] = X::mfma(attn_ld_t<TS>(sKt, 32 * dt + j, 32 * sub, 0, g), db0, dq[dt]);
          dq[dt] = X::mfma(attn_ld_t<TS>(sKt, 32 * dt + j, 32 * sub, 1, g), db1, dq[dt]);
        }
      }
    }

    if (qrow >= 0) attn_store_row<X, D>(dq, scale, gq + (qrow * heads + h) * (int64_t)D, g);
  }
}

// ---------------------------------------------------------------- host side
// LAUNCH(payload type, D, causal) by (dtype, D, causal)
#define RUA_ATTN_DISPATCH(dtype, D, causal, LAUNCH)                                                                    \
  do {                                                                                                                 \
    if ((dtype) == RUA_BF16) {                                                                                         \
      if ((D) == 32) { if (causal) LAUNCH(at_bf16, 32, true); else LAUNCH(at_bf16, 32, false); }                       \
      else if ((D) == 64) { if (causal) LAUNCH(at_bf16, 64, true); else LAUNCH(at_bf16, 64, false); }                  \
      else { if (causal) LAUNCH(at_bf16, 128, true); else LAUNCH(at_bf16, 128, false); }                               \
    } else {                                                                                                           \
      if ((D) == 32) { if (causal) LAUNCH(at_f16, 32, true); else LAUNCH(at_f16, 32, false); }                         \
      else if ((D) == 64) { if (causal) LAUNCH(at_f16, 64, true); else LAUNCH(at_f16, 64, false); }                    \
      else { if (causal) LAUNCH(at_f16, 128, true); else LAUNCH(at_f16, 128, false); }                                 \
    }                                                                                                                  \
  } while (0)

// the trace line of one of the three walks: the plain form names `causal`, the band form its four words
static void attn_trace(const char* role, const attn_band* band, int32_t D, int32_t heads, bool causal, const rua_layout& LQ,
                       const rua_layout& LK, unsigned grid) {
  if (band)
    seg_trace("seg_attn_band_%s_kernel D=%d heads=%d kvheads=%d left=%lld right=%lld end=%d kind=%d kvkind=%d grid=%u", role,
              D, heads, band->heads_kv, (long long)band->left, (long long)band->right, band->align_end, LQ.kind, LK.kind,
              grid);
  else
    seg_trace("seg_attn_%s_kernel D=%d heads=%d causal=%d kind=%d kvkind=%d grid=%u", role, D, heads, (int)causal, LQ.kind,
              LK.kind, grid);
}

// both forward entry points; `band` is null for the plain form, which launches the <X, D, CAUSAL> instantiations
static int attn_forward(const rua_layout* q, const rua_layout* kv, const void* q_ptr, const void* k_ptr,
                        const void* v_ptr, void* out, void* lse, int32_t heads, int32_t D, int32_t dtype, bool causal,
                        double scale, int64_t T_max, void* stream, const attn_band* band) {
  const int32_t heads_kv = band ? band->heads_kv : heads;
  int e;
  if ((e = attn_check_entry(q, kv, heads, heads_kv, D, dtype, scale, T_max)) != 0) return e;
  if (q->B == 0 || T_max == 0) return 0;
  if ((q->n_rows > 0 && (!q_ptr || !out || !lse)) || (kv->n_rows > 0 && (!k_ptr || !v_ptr))) return RUA_EINVAL;
  if (attn_misaligned(q_ptr) || attn_misaligned(k_ptr) || attn_misaligned(v_ptr) || attn_misaligned(out) ||
      ((uintptr_t)lse & 3))
    return RUA_EALIGN;
  if (seg_too_large(q, (int64_t)heads * D, 2) || seg_too_large(kv, (int64_t)heads_kv * D, 2)) return RUA_ERANGE;
  int64_t nblk, items;
  unsigned grid;
  if (!attn_items(q->B, heads, T_max, nblk, items, grid)) return RUA_ERANGE;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = band ? *band : attn_band{-1, -1, heads, 0};
  attn_trace("forward", band, D, heads, causal, LQ, LK, grid);
#define RUA_ATTN_FWD_ARGS                                                                                              \
  dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK, (const uint16_t*)q_ptr, (const uint16_t*)k_ptr, (const uint16_t*)v_ptr,   \
      (uint16_t*)out, (float*)lse, (int)heads, (float)scale, nblk, items, bd
#define RUA_ATTN_FWD(XX, DD, CC) hipLaunchKernelGGL((seg_attn_forward_kernel<XX, DD, CC>), RUA_ATTN_FWD_ARGS)
#define RUA_ATTN_FWD_BAND(XX, DD) hipLaunchKernelGGL((seg_attn_forward_kernel<XX, DD, false, true>), RUA_ATTN_FWD_ARGS)
  if (band)
    RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_FWD_BAND);
  else
    RUA_ATTN_DISPATCH(dtype, D, causal, RUA_ATTN_FWD);
#undef RUA_ATTN_FWD_BAND
#undef RUA_ATTN_FWD
#undef RUA_ATTN_FWD_ARGS
  return (int)hipGetLastError();
}

// both backward entry points: delta, then dK / dV (over the kv heads in the band form), then dQ
static int attn_backward(const rua_layout* q, const rua_layout* kv, const void* q_ptr, const void* k_ptr,
                         const void* v_ptr, const void* out, const void* lse, const void* grad_out, void* grad_q,
                         void* grad_k, void* grad_v, void* ws, int32_t heads, int32_t D, int32_t dtype, bool c,
                         double scale, int64_t T_max, int64_t S_max, void* stream, const attn_band* band) {
  const int32_t heads_kv = band ? band->heads_kv : heads;
  int e;
  if ((e = attn_check_entry(q, kv, heads, heads_kv, D, dtype, scale, T_max)) != 0) return e;
  if (S_max < 0) return RUA_EINVAL;
  if (q->B == 0) return 0;
  if (q->n_rows > 0 && (!q_ptr || !out || !lse || !grad_out || !grad_q || !ws)) return RUA_EINVAL;
  if (kv->n_rows > 0 && (!k_ptr || !v_ptr || !grad_k || !grad_v)) return RUA_EINVAL;
  // a gradient that aliases what the walks read, or another gradient
  if (grad_q && (grad_q == grad_out || grad_q == q_ptr || grad_q == out)) return RUA_EINVAL;
  if (grad_k && (grad_k == k_ptr || grad_k == v_ptr || grad_k == grad_v || grad_k == grad_q)) return RUA_EINVAL;
  if (grad_v && (grad_v == k_ptr || grad_v == v_ptr || grad_v == grad_q)) return RUA_EINVAL;
  const void* ptrs[] = {q_ptr, k_ptr, v_ptr, out, grad_out, grad_q, grad_k, grad_v};
  for (const void* p : ptrs)
    if (attn_misaligned(p)) return RUA_EALIGN;
  if (((uintptr_t)lse & 3) || ((uintptr_t)ws & 3)) return RUA_EALIGN;
  if (seg_too_large(q, (int64_t)heads * D, 2) || seg_too_large(kv, (int64_t)heads_kv * D, 2)) return RUA_ERANGE;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = band ? *band : attn_band{-1, -1, heads, 0};
  float* delta = (float*)ws;

  if (T_max > 0 && q->n_rows > 0) {
    const int64_t n = q->n_rows * heads, dgrid = (n + RUA_BLOCK - 1) / RUA_BLOCK;
    if (dgrid > 0x7fffffffLL) return RUA_ERANGE;
    seg_trace("seg_attn_delta_kernel D=%d heads=%d grid=%lld", D, heads, (long long)dgrid);
#define RUA_ATTN_DELTA(XX, DD, CC)                                                                                     \
  hipLaunchKernelGGL((seg_attn_delta_kernel<XX, DD>), dim3((unsigned)dgrid), dim3(RUA_BLOCK), 0, s,                    \
                     (const uint16_t*)out, (const uint16_t*)grad_out, delta, n)
    RUA_ATTN_DISPATCH(dtype, D, false, RUA_ATTN_DELTA);
#undef RUA_ATTN_DELTA
    if ((e = (int)hipGetLastError()) != 0) return e;
  }
  int64_t nblk, items;
  unsigned grid;
  if (S_max > 0) {
    if (!attn_items(q->B, heads_kv, S_max, nblk, items, grid)) return RUA_ERANGE;
    attn_trace("dkdv", band, D, heads, c, LQ, LK, grid);
#define RUA_ATTN_DKDV_ARGS                                                                                             \
  dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK, (const uint16_t*)q_ptr, (const uint16_t*)k_ptr, (const uint16_t*)v_ptr,   \
      (const uint16_t*)grad_out, (const float*)lse, (const float*)delta, (uint16_t*)grad_k, (uint16_t*)grad_v,         \
      (int)heads, (float)scale, nblk, items, bd
#define RUA_ATTN_DKDV(XX, DD, CC) hipLaunchKernelGGL((seg_attn_dkdv_kernel<XX, DD, CC>), RUA_ATTN_DKDV_ARGS)
#define RUA_ATTN_DKDV_BAND(XX, DD) hipLaunchKernelGGL((seg_attn_dkdv_kernel<XX, DD, false, true>), RUA_ATTN_DKDV_ARGS)
    if (band)
      RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DKDV_BAND);
    else
      RUA_ATTN_DISPATCH(dtype, D, c, RUA_ATTN_DKDV);
#undef RUA_ATTN_DKDV_BAND
#undef RUA_ATTN_DKDV
#undef RUA_ATTN_DKDV_ARGS
    if ((e = (int)hipGetLastError()) != 0) return e;
  }
  if (T_max > 0) {
    if (!attn_items(q->B, heads, T_max, nblk, items, grid)) return RUA_ERANGE;
    attn_trace("dq", band, D, heads, c, LQ, LK, grid);
#define RUA_ATTN_DQ_ARGS                                                                                               \
  dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK, (const uint16_t*)q_ptr, (const uint16_t*)k_ptr, (const uint16_t*)v_ptr,   \
      (const uint16_t*)grad_out, (const float*)lse, (const float*)delta, (uint16_t*)grad_q, (int)heads, (float)scale,  \
      nblk, items, bd
#define RUA_ATTN_DQ(XX, DD, CC) hipLaunchKernelGGL((seg_attn_dq_kernel<XX, DD, CC>), RUA_ATTN_DQ_ARGS)
#define RUA_ATTN_DQ_BAND(XX, DD) hipLaunchKernelGGL((seg_attn_dq_kernel<XX, DD, false, true>), RUA_ATTN_DQ_ARGS)
    if (band)
      RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DQ_BAND);
    else
      RUA_ATTN_DISPATCH(dtype, D, c, RUA_ATTN_DQ);
#undef RUA_ATTN_DQ_BAND
#undef RUA_ATTN_DQ
#undef RUA_ATTN_DQ_ARGS
  }
  return (int)hipGetLastError();
}

}  // namespace rua

extern "C" int rua_segment_attention_forward(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                             const void* k_ptr, const void* v_ptr, void* out, void* lse, int32_t heads,
                                             int32_t D, int32_t dtype, int32_t causal, double scale, int64_t T_max,
                                             void* stream) {
  return rua::attn_forward(q, kv, q_ptr, k_ptr, v_ptr, out, lse, heads, D, dtype, causal != 0, scale, T_max, stream,
                           nullptr);
}

extern "C" int rua_segment_attention_backward(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                              const void* k_ptr, const void* v_ptr, const void* out, const void* lse,
                                              const void* grad_out, void* grad_q, void* grad_k, void* grad_v, void* ws,
                                              int32_t heads, int32_t D, int32_t dtype, int32_t causal, double scale,
                                              int64_t T_max, int64_t S_max, void* stream) {
  return rua::attn_backward(q, kv, q_ptr, k_ptr, v_ptr, out, lse, grad_out, grad_q, grad_k, grad_v, ws, heads, D, dtype,
                            causal != 0, scale, T_max, S_max, stream, nullptr);
}

extern "C" int rua_segment_attention_band_forward(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                                  const void* k_ptr, const void* v_ptr, void* out, void* lse,
                                                  int32_t heads, int32_t D, int32_t dtype, int32_t heads_kv, int64_t left,
                                                  int64_t right, int32_t align_end, double scale, int64_t T_max,
                                                  void* stream) {
  const rua::attn_band bd = {left < 0 ? -1 : left, right < 0 ? -1 : right, heads_kv, align_end != 0};
  return rua::attn_forward(q, kv, q_ptr, k_ptr, v_ptr, out, lse, heads, D, dtype, false, scale, T_max, stream, &bd);
}

extern "C" int rua_segment_attention_band_backward(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                                   const void* k_ptr, const void* v_ptr, const void* out,
                                                   const void* lse, const void* grad_out, void* grad_q, void* grad_k,
                                                   void* grad_v, void* ws, int32_t heads, int32_t D, int32_t dtype,
                                                   int32_t heads_kv, int64_t left, int64_t right, int32_t align_end,
                                                   double scale, int64_t T_max, int64_t S_max, void* stream) {
  const rua::attn_band bd = {left < 0 ? -1 : left, right < 0 ? -1 : right, heads_kv, align_end != 0};
  return rua::attn_backward(q, kv, q_ptr, k_ptr, v_ptr, out, lse, grad_out, grad_q, grad_k, grad_v, ws, heads, D, dtype,
                            false, scale, T_max, S_max, stream, &bd);
}
