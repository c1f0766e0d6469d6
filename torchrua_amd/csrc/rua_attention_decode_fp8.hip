// rua_attention_decode_fp8.hip — attention for decode steps over an fp8 KV cache (rua_segment_attention_decode_fp8;
// include/rua.h).  The sibling of rua_attention_decode.hip's walk for K and V stored as OCP e4m3 codes with
// one fp32 scale per kv head: the value of a cache element is float(code) * scale[hk].  q, the output and all the
// arithmetic stay in q's dtype (bf16 / f16) and fp32; the kernel reads HALF the K / V bytes, which is what a decode step
// costs.  The work item (sequence, kv head, column block, split), the packed columns c = t G + gi, the four waves that
// divide every 128-key step without a __syncthreads(), the band skip, the fixed-order merge, the partial format and
// the combine kernel are rua_attention_decode.hip's; what follows is what differs.
//
// DEQUANTISATION IS EXACT AND HAPPENS IN REGISTERS.  Every finite e4m3 value (3 significant bits, exponents -9 .. 8) is a
// bf16 and an f16 value, so v_cvt_scalef32_pk_bf16_fp8 / _pk_f16_fp8 with the scale operand 1.0 turn two codes into the
// two 16-bit elements of a matrix operand without rounding: one instruction per pair, no fp32 detour.  After it the
// MFMAs (32x32x16 in q's dtype — not the fp8 MFMA, which would quantise q and P), the online softmax and the bf16 hi + lo
// P are the forward's.  The scale operand of the convert is NOT used for the cache scales (it would round):
//   k_scale[hk]  is folded ONCE per work item into the softmax scale:  sc = scale * (k_scale[hk] * k_scale_by_value);
//   v_scale[hk]  multiplies the merged fp32 accumulator once, right after the four-wave merge and before either the
//                in-place finish (n_split == 1) or the write of the partial to ws: one rule for both paths.
// Power-of-two scales make both folds exact; others add two roundings to the score scale and one to the accumulator.
//
// THE d PERMUTATION.  A kv-head row is D BYTES, so a 16-byte load holds 16 elements — two k-steps of the MFMA.  Lane
// (j, g) takes the bytes 32 s + 16 g .. + 15 of key ks + j (s = 0 .. D / 32 - 1) and feeds its low 8 to k-step 2 s and its
// high 8 to k-step 2 s + 1: within k-step 2 s + e the lane of half g holds d = 32 s + 16 g + 8 e + i, i = 0 .. 7.  A
// contraction does not care in which order d is walked as long as both operands agree, so the packed q columns are
// loaded once per work item in the same order (two 16-byte loads of the 32 bytes 32 s + 16 g .. of the q row).  K costs
// D / 32 load instructions per sub-tile — half the bf16 kernel's, ONE at D = 32 — and goes from global memory straight
// to the converter and the A operand.  Keys past S_b (and rows outside the storage) are zeros by predicate on the key
// index: code 0x00 is +0.  The loads of the next sub-tile are issued once the score MFMAs have consumed the K registers.
//
// V: THE SAME LOAD, CONVERTED, STAGED TRANSPOSED.  Lane (j, g) now owns 16 consecutive d of token j (not 8) and writes
// them with 2-byte stores into the per-wave tile sVt[D][TS].  BANKS (64 banks of 4 bytes; a 2-byte store instruction
// serves its 64 lanes at once, an 8-byte read 32 lanes at a time):
//   stores  one instruction is one (s, i): half g writes the 32 consecutive tokens of row d = 32 s + 16 g + i — 16
//           consecutive words, two lanes per word — and the two halves sit 16 d = 8 TS words apart.  TS = 32 + 8 (the
//           bf16 kernel's, whose halves sit 8 d = 160 = 2 x 64 + 32 words apart) gives 320 = 5 x 64 words: BOTH HALVES IN
//           THE SAME 16 BANKS, a two-way conflict on every store.  TS = 32 + 4 gives 288 = 4 x 64 + 32: banks 0 .. 15
//           and 32 .. 47, no conflict.
//   reads   attn_ld_t: lane (j, g) reads 2 x 8 bytes of row 32 dt + j at token 16 c + 4 g (+ 8); the 32 lanes of a half
//           sit TS / 2 = 18 words apart: 18 j mod 64 over j = 0 .. 31 are the 32 even residues, each lane takes that
//           word and the next: all 64 banks once.  (TS = 40: 20 j mod 64 repeats from j = 16 — a two-way conflict the
//           bf16 kernel lives with.)  8-byte alignment holds: a row is 72 bytes.
// So the tile is [D][32 + 4]: 288 D bytes for four waves, below the merge buffer's 384 D as before.
//
// REGISTERS (hipcc's resource report for gfx950; bf16 q / f16 q; no scratch, no spill as built):
//   D = 32    185 / 139 VGPRs   waves_per_eu 2 (f16: 3 fit)
//   D = 64    236 / 197 VGPRs   waves_per_eu 2
//   D = 128   256 VGPRs + 141 / 102 AGPRs   waves_per_eu 1
// K and V in flight take D / 8 VGPRs each instead of D / 4.  That does NOT lift D = 128 to two waves per SIMD: asked for
// two, the compiler spills 76 / 36 registers (300 / 148 bytes of scratch per lane), so it stays at one like the bf16 kernel.
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#include "rua_attention_decode_dev.h"

namespace rua {

// K and V codes of the 32 keys [ks, ks + 32): lane (j, g) takes the 16 bytes 32 s + 16 g .. + 15 of key ks + j, s = 0 ..
// D / 32 - 1; zeros (code 0x00 = +0) when the key is past the end or `on` is false
template <int D>
__device__ __forceinline__ void dec8_load(const rua_layout& LK, int64_t b, int64_t S, int64_t ks, bool on, int hk, int hkv,
                                          const uint8_t* __restrict__ k, const uint8_t* __restrict__ v, int j, int g,
                                          uint4* kf, uint4* vf) {
  const int64_t row = on ? attn_row(LK, b, ks + j, S) : (int64_t)-1;
  const int64_t at = (row * hkv + hk) * (int64_t)D + 16 * g;
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    kf[s] = vf[s] = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) {
      kf[s] = *(const uint4*)(k + at + 32 * s);
      vf[s] = *(const uint4*)(v + at + 32 * s);
    }
  }
}

// ---------------------------------------------------------------- the walk: one (sequence, kv head, column block, split)
template <typename X, int D>
__global__ __launch_bounds__(RUA_BLOCK) __attribute__((amdgpu_waves_per_eu(D <= 64 ? 2 : 1)))  // see REGISTERS
void seg_attn_decode_fp8_kernel(rua_layout LQ, rua_layout LK, const uint16_t* __restrict__ q,
                                const uint8_t* __restrict__ k, const uint8_t* __restrict__ v,
                                const float* __restrict__ k_scale, const float* __restrict__ v_scale, float k_mul,
                                float v_mul, uint16_t* __restrict__ out, float* __restrict__ lse,
                                float* __restrict__ ws, int heads, float scale, int64_t ncb, int64_t kv_chunk,
                                int64_t n_split, int64_t items, attn_band bd) {
  constexpr int TS = DEC8_TS, ND = D / 32, NR = ND * 16;
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

    // the scales of this kv head: k's goes into the softmax scale, v's waits for the merged accumulator
    const float sc = scale * ((k_scale ? k_scale[hk] : 1.f) * k_mul);
    const float vs = (v_scale ? v_scale[hk] : 1.f) * v_mul;

    // the lane's column: query position t, head h; its q operand in the d order of the K loads, once per work item
    const int64_t c = cb * DEC_COLS + j, t = c / G;
    const int h = hk * G + (int)(c % G);
    const int64_t qrow = t < T ? attn_row(LQ, b, t, T) : (int64_t)-1;
    uint4 qf[2 * ND];
#pragma unroll
    for (int s = 0; s < ND; ++s) {
      qf[2 * s] = qf[2 * s + 1] = make_uint4(0u, 0u, 0u, 0u);
      if (qrow >= 0) {
        const uint16_t* p = q + (qrow * heads + h) * (int64_t)D + 32 * s + 16 * g;
        qf[2 * s] = *(const uint4*)p;
        qf[2 * s + 1] = *(const uint4*)(p + 8);
      }
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

    uint4 kf[ND], vf[ND];
    dec8_load<D>(LK, b, S, ks, ks < kend, hk, hkv, k, v, j, g, kf, vf);
    __syncthreads();                                            // the merge buffer of the item before is consumed
    while (ks < kend) {
      // V of this sub-tile, converted and transposed: token j of the rows 32 s + 16 g .. + 15
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int s = 0; s < ND; ++s) {
        const uint4 v0 = dec8_up<X>(vf[s].x, vf[s].y), v1 = dec8_up<X>(vf[s].z, vf[s].w);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          sVt[(32 * s + 16 * g + i) * TS + j] = attn_elem(v0, i);
          sVt[(32 * s + 16 * g + 8 + i) * TS + j] = attn_elem(v1, i);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      attn_f32x16 sa;
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[r] = 0.f;
#pragma unroll
      for (int s = 0; s < ND; ++s) {
        sa = X::mfma(dec8_up<X>(kf[s].x, kf[s].y), qf[2 * s], sa);
        sa = X::mfma(dec8_up<X>(kf[s].z, kf[s].w), qf[2 * s + 1], sa);
      }
      const int64_t ksn = ks + DEC_STEP;
      dec8_load<D>(LK, b, S, ksn, ksn < kend, hk, hkv, k, v, j, g, kf, vf);
      // the online softmax on the accumulator layout: the lane is the column, its registers are keys; the keys of the
      // sub-tile that the lane's query sees are the offsets [vlo, vhi)
      const int64_t dlo = see_lo - ks, dhi = see_hi - ks;
      const int vlo = dlo < 0 ? 0 : dlo > 32 ? 32 : (int)dlo, vhi = dhi < 0 ? 0 : dhi > 32 ? 32 : (int)dhi;
      float sv[16], mx = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = 8 * (r >> 2) + 4 * g + (r & 3);         // key ks + off
        sv[r] = (off >= vlo && off < vhi) ? sa[r] * sc : NEG_INF;
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
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc[dt] = acc[dt] * vs;     // v's scale, once, for the finish and the partial alike
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

extern "C" int rua_segment_attention_decode_fp8(const rua_layout* q, const rua_layout* kv, const void* q_ptr,
                                                const void* k_ptr, const void* v_ptr, void* out, void* lse, void* ws,
                                                int64_t ws_bytes, int32_t heads, int32_t D, int32_t dtype,
                                                int32_t heads_kv, int64_t left, int64_t right, int32_t align_end,
                                                double scale, int64_t T_max, int64_t S_max, int64_t kv_chunk,
                                                int32_t kv_dtype, const float* k_scale, const float* v_scale,
                                                double k_scale_by_value, double v_scale_by_value, void* stream) {
  using namespace rua;
  int e;
  dec_launch L;
  if (kv_dtype != RUA_KV_E4M3 || dec8_bad_scale(k_scale_by_value) || dec8_bad_scale(v_scale_by_value)) return RUA_EINVAL;
  if ((e = dec_prepare(q, kv, q_ptr, k_ptr, v_ptr, out, lse, ws, ws_bytes, heads, D, dtype, heads_kv, left, right,
                       align_end, scale, T_max, S_max, kv_chunk, 1, L)) != 0)
    return e;
  if (((uintptr_t)k_scale & 3) || ((uintptr_t)v_scale & 3)) return RUA_EALIGN;
  if (!L.run) return 0;
  const dec_plan& p = L.p;
  const unsigned grid = L.grid;
  const int64_t items = L.items;
  const hipStream_t s = (hipStream_t)stream;
  const rua_layout LQ = *q, LK = *kv;
  const attn_band bd = L.bd;
  seg_trace("seg_attn_decode_fp8_kernel D=%d heads=%d kvheads=%d left=%lld right=%lld end=%d cols=%lld chunk=%lld "
            "splits=%lld kind=%d kvkind=%d grid=%u", D, heads, heads_kv, (long long)bd.left, (long long)bd.right,
            bd.align_end, (long long)(T_max * (heads / heads_kv)), (long long)p.kv_chunk, (long long)p.n_split, LQ.kind,
            LK.kind, grid);
#define RUA_ATTN_DECODE_FP8(XX, DD)                                                                                    \
  hipLaunchKernelGGL((seg_attn_decode_fp8_kernel<XX, DD>), dim3(grid), dim3(RUA_BLOCK), 0, s, LQ, LK,                  \
                     (const uint16_t*)q_ptr, (const uint8_t*)k_ptr, (const uint8_t*)v_ptr, k_scale, v_scale,           \
                     (float)k_scale_by_value, (float)v_scale_by_value, (uint16_t*)out, (float*)lse, (float*)ws,        \
                     (int)heads, (float)scale, p.ncb, p.kv_chunk, p.n_split, items, bd)
  RUA_ATTN_DISPATCH_BAND(dtype, D, RUA_ATTN_DECODE_FP8);
#undef RUA_ATTN_DECODE_FP8
  if ((e = (int)hipGetLastError()) != 0 || p.n_split == 1) return e;
  return dec_combine(q, kv, L, ws, out, lse, heads, D, dtype, heads_kv, T_max, s);
}
