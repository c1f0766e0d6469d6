// rua_softmax.hip — per-sequence softmax / log_softmax over the tokens of a C / L / P / R container, and their backward
// (rua_segment_softmax, rua_segment_softmax_backward; include/rua.h).  An extension: the reference spells it as
// segment_logsumexp + repeat_interleave + sub (+ exp) over [N, H] temporaries, for a CattedSequence only.
//
// ONE fold order per (sequence, column), whatever the layout, the kernel form, the alignment or the launch geometry —
// that is what makes the operator commute with the casts bit for bit (z.softmax().cat() == z.cat().softmax()):
//   - the tokens of a sequence are cut into BLOCKS of SM_BLOCK_TOK = 2 048 consecutive tokens;
//   - inside a block, SLOT r (of SM_SLOTS = 32) folds the tokens t = r (mod 32) in ascending order, starting from the
//     identity (max = -inf, sum = 0), with the one-exp online update `fold` below;
//   - the 32 slots are combined by a butterfly over the slot number (xor 1, 2, 4, 8, 16; `combine` is symmetric in its
//     arguments, and this file is compiled without fp contraction, so both partners compute the same bits);
//   - the block results are combined in ascending block order, starting from the identity.
// The lanes form maps a slot to a lane, the row forms map it to 8 consecutive threads of a workgroup (one 16-byte
// vector each); the cut form hands the blocks of a long sequence to different workgroups and folds their results from
// a small workspace in the same order.  The backward's per-sequence sums follow the same order with `+`.
//
// y = exp(x - max) / sum and y = (x - max) - log(sum) are evaluated in fp32 (fp64 for RUA_F64) and rounded once.  A
// column of a sequence that holds NaN or +inf, or only -inf, is NaN throughout — torch.softmax(seq, dim=0) per sequence.
// Padding rows of a LEFT / RIGHT result are written as zeros in the same pass and are never read.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "rua_seg_launch.h"

#pragma clang fp contract(off)

namespace rua {

constexpr int SM_SLOTS = 32;               // parallel fold chains per (sequence, column)
constexpr int SM_BLOCK_TOK = SEG_BLOCK_TOK; // tokens per block = 64 per slot
constexpr int SM_LPR = 8;                  // row forms: 16-byte lanes per row chunk (128 bytes)
constexpr int SM_ROWS_UNR = 4;             // row forms: rows in flight per thread
constexpr int SM_LANES_UNR = 8;            // lanes form: tokens a lane keeps in registers (sequences up to 256 tokens)
constexpr int SM_CAP_FWD = 512;            // resident rows of a slab: 512 x 128 B = 64 KiB, two workgroups per CU
constexpr int SM_CAP_BWD = 256;            // the backward keeps y AND g

// ---------------------------------------------------------------- the fold
// online (max, sum): one exp per element.  NaN and +inf poison the sum (torch: the whole column of the sequence is NaN);
// -inf adds nothing; the max itself is never NaN.
template <typename A> __device__ __forceinline__ void fold(A& m, A& s, A x) {
  const A inf = seg_inf<A>();
  if (!(x < inf)) {
    s = seg_nan<A>();
  } else if (x > m) {
    s = s * seg_exp(m - x) + (A)1;
    m = x;
  } else if (x > -inf) {
    s = s + seg_exp(x - m);
  }
}

// symmetric: combine(a, b) and combine(b, a) are the same bits
template <typename A> __device__ __forceinline__ void combine(A& m, A& s, A m2, A s2) {
  const A M = m > m2 ? m : m2;
  if (M == -seg_inf<A>()) {
    s = s + s2;
  } else {
    const A a = s * seg_exp(m - M), b = s2 * seg_exp(m2 - M);
    s = a + b;
  }
  m = M;
}

// what walk 2 writes.  forward: (m, s) hold max and 1 / sum (softmax) or log(sum) (log_softmax);
// backward: s is the sequence's sum of g * y (softmax) or of g (log_softmax), v = y
template <bool BWD, typename A> __device__ __forceinline__ A finish(A v, A g, A m, A s, int lg) {
  if constexpr (BWD) {
    return lg ? g - seg_exp(v) * s : v * (g - s);
  } else {
    return lg ? (v - m) - s : seg_exp(v - m) * s;
  }
}

// ---------------------------------------------------------------- lanes along time: rows of one vector (<= 16 bytes)
// A wave takes two sequences, 32 lanes each; lane r of a half is slot r: consecutive lanes take consecutive tokens (one
// contiguous run of whole lines for CAT), the fold goes across lanes by shuffles.  Sequences of up to 256 tokens stay in
// registers between the two walks; longer ones are read again.
template <typename E, bool BWD>
__global__ __launch_bounds__(RUA_BLOCK) void seg_softmax_lanes_kernel(rua_layout L, const char* xin, const char* gin,
                                                                      char* out, int H, int W, int lg) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int UNR = SM_LANES_UNR;
  const int lane = threadIdx.x & (RUA_WAVE - 1);
  const int q = lane & (SM_SLOTS - 1);
  const int64_t wave = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) >> 6;
  const int64_t b = wave * 2 + (lane >> 5);
  const bool have = b < L.B;
  const int64_t len = have ? safe_len(L, b) : 0;
  const int64_t other = __shfl_xor(len, 32, RUA_WAVE);
  const int64_t maxlen = len > other ? len : other;          // wave-uniform
  const int nb = H * (int)sizeof(raw);
  const bool keep = maxlen <= (int64_t)SM_SLOTS * UNR;

  struct alignas(16) Row { raw e[VE]; };
  Row vx[UNR], vg[UNR];
  A M[VE], S[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { M[e] = -seg_inf<A>(); S[e] = (A)0; }

  for (int64_t t0 = 0; t0 < maxlen; t0 += SM_BLOCK_TOK) {
    A m[VE], s[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) { m[e] = -seg_inf<A>(); s[e] = (A)0; }
    const int64_t t1 = len < t0 + SM_BLOCK_TOK ? len : t0 + SM_BLOCK_TOK;
    const int64_t t1w = maxlen < t0 + SM_BLOCK_TOK ? maxlen : t0 + SM_BLOCK_TOK;
    for (int64_t tt = t0; tt < t1w; tt += (int64_t)SM_SLOTS * UNR) {
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t t = tt + (int64_t)u * SM_SLOTS + q;
        ok[u] = false;
        if (t < t1) {
          const int64_t row = token_to_row(L, b, t, len);
          if (row >= 0 && row < L.n_rows) {
            ok[u] = true;
            ld_row_w(xin + row * nb, nb, W, &vx[u]);
            if constexpr (BWD) ld_row_w(gin + row * nb, nb, W, &vg[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if (e >= H) continue;
          if constexpr (BWD) {
            const A y = E::up(vx[u].e[e]), g = E::up(vg[u].e[e]);
            s[e] = s[e] + (lg ? g : g * y);
          } else {
            fold(m[e], s[e], E::up(vx[u].e[e]));
          }
        }
      }
    }
#pragma unroll
    for (int k = 1; k < SM_SLOTS; k <<= 1) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A s2 = seg_shfl_xor(s[e], k);
        if constexpr (BWD) {
          s[e] = s[e] + s2;
        } else {
          const A m2 = seg_shfl_xor(m[e], k);
          combine(m[e], s[e], m2, s2);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if constexpr (BWD) S[e] = S[e] + s[e];
      else combine(M[e], S[e], m[e], s[e]);
    }
  }
  if constexpr (!BWD) {
#pragma unroll
    for (int e = 0; e < VE; ++e) S[e] = lg ? seg_log(S[e]) : (A)1 / S[e];
  }

  // walk 2
  for (int64_t tt = 0; tt < len; tt += (int64_t)SM_SLOTS * UNR) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t t = tt + (int64_t)u * SM_SLOTS + q;
      if (t >= len) continue;
      const int64_t row = token_to_row(L, b, t, len);
      if (row < 0 || row >= L.n_rows) continue;
      if (!keep) {
        ld_row_w(xin + row * nb, nb, W, &vx[u]);
        if constexpr (BWD) ld_row_w(gin + row * nb, nb, W, &vg[u]);
      }
      Row o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A g = BWD ? E::up(vg[u].e[e]) : (A)0;
        o.e[e] = E::down(finish<BWD, A>(E::up(vx[u].e[e]), g, M[e], S[e], lg));
      }
      st_row_w(out + row * nb, nb, W, &o);
    }
  }
  if (have && (L.kind == RUA_LEFT || L.kind == RUA_RIGHT)) {
    Row z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = E::down((A)0);
    for (int64_t j = q; j < L.T_phys; j += SM_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st_row_w(out + row * nb, nb, W, &z);
    }
  }
}

// ---------------------------------------------------------------- rows wider than one vector
// A workgroup takes (sequence x 128-byte column chunk): thread (q, l) = (tid / 8, tid % 8) is slot q and owns the l-th
// 16-byte vector of the chunk.  RESIDENT (len <= cap_rows): walk 1 parks every vector in LDS in the payload dtype —
// each thread reads back exactly what it stored, so the slab needs no barrier — and walk 2 normalises out of LDS: the
// payload crosses HBM once.  Otherwise STREAMING: walk 2 reads global memory again (the same workgroup, so L2 / the
// Infinity Cache may serve it).  mode SEG_PARTIAL / SEG_FINISH: the CUT form — a workgroup per (sequence, block of 2 048
// tokens, chunk) leaves its block's (max, sum) in `ws`, and a second launch folds them in block order and normalises.
// AL = false: rows or bases off 16 bytes — the same geometry with elementwise accesses.
template <typename E, bool BWD, bool AL>
__global__ __launch_bounds__(RUA_BLOCK) void seg_softmax_rows_kernel(rua_layout L, const typename E::raw* xin,
                                                                     const typename E::raw* gin, typename E::raw* out,
                                                                     int64_t H, int n_chunks, int cap_rows, int mode,
                                                                     int maxblk, typename E::acc* ws, int lg) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  constexpr int CW = SM_LPR * VE;
  constexpr int UNR = SM_ROWS_UNR;
  constexpr int XCH_BYTES = RUA_WAVES_PER_BLOCK * SM_LPR * VE * 2 * (int)sizeof(A);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  A* xch = (A*)smem;                                       // [wave][l][e][2]
  struct alignas(16) Vec { raw e[VE]; };
  Vec* slab = (Vec*)(smem + XCH_BYTES);                    // [row][l] (+ the same again for g in the backward)

  const int tid = threadIdx.x;
  const int l = tid & (SM_LPR - 1), q = tid >> 3, w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)n_chunks);
  int64_t b = blockIdx.x / (unsigned)n_chunks;
  int blk = 0;
  if (mode != SEG_FULL) { blk = (int)(b % maxblk); b /= maxblk; }
  if (b >= L.B) return;
  const int64_t len = safe_len(L, b);
  // the cut form sized `ws` and the grid from the host's length bound: a CAT layout whose T_log understates a length
  // must not walk past the maxblk blocks that exist (rua.h: T_log has to be a true bound for a right result)
  const int64_t have_blk = (len + SM_BLOCK_TOK - 1) / SM_BLOCK_TOK;
  const int64_t nblk = mode != SEG_FULL && have_blk > maxblk ? maxblk : have_blk;
  if (mode != SEG_FULL && blk > 0 && blk >= nblk) return;   // workgroup-uniform
  const int64_t col0 = (int64_t)c * CW + (int64_t)l * VE;
  const int nval = H - col0 >= VE ? VE : (H - col0 > 0 ? (int)(H - col0) : 0);
  const bool active = nval > 0;
  int64_t tb = 0, te = len;
  if (mode != SEG_FULL) {
    tb = (int64_t)blk * SM_BLOCK_TOK;
    te = len < tb + SM_BLOCK_TOK ? len : tb + SM_BLOCK_TOK;
    if (tb > te) tb = te;
  }
  const bool resident = mode == SEG_FULL && len <= cap_rows;

  auto ld = [&](const raw* base, int64_t row, Vec& v) {
    const raw* p = base + row * H + col0;
    if constexpr (AL) {
      *(uint4*)&v = *(const uint4*)p;
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v.e[e] = e < nval ? p[e] : E::down((A)0);
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

  A M[VE], S[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) { M[e] = -seg_inf<A>(); S[e] = (A)0; }

  if (mode == SEG_FINISH) {
    for (int64_t k = 0; k < nblk; ++k) {
      const A* p = ws + ((((b * maxblk + k) * n_chunks + c) * SM_LPR + l) * VE) * 2;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if constexpr (BWD) S[e] = S[e] + p[e * 2 + 1];
        else combine(M[e], S[e], p[e * 2], p[e * 2 + 1]);
      }
    }
  } else {
    for (int64_t t0 = tb; t0 < te; t0 += SM_BLOCK_TOK) {
      A m[VE], s[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) { m[e] = -seg_inf<A>(); s[e] = (A)0; }
      const int64_t t1 = te < t0 + SM_BLOCK_TOK ? te : t0 + SM_BLOCK_TOK;
      if (active) {
        for (int64_t tt = t0 + q; tt < t1; tt += (int64_t)SM_SLOTS * UNR) {
          Vec vx[UNR], vg[UNR];
          bool ok[UNR];
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int64_t t = tt + (int64_t)u * SM_SLOTS;
            ok[u] = false;
            if (t < t1) {
              const int64_t row = token_to_row(L, b, t, len);
              if (row >= 0 && row < L.n_rows) {
                ok[u] = true;
                ld(xin, row, vx[u]);
                if constexpr (BWD) ld(gin, row, vg[u]);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int64_t t = tt + (int64_t)u * SM_SLOTS;
            if (!ok[u]) continue;
            if (resident) {
              slab[t * SM_LPR + l] = vx[u];
              if constexpr (BWD) slab[((int64_t)cap_rows + t) * SM_LPR + l] = vg[u];
            }
#pragma unroll
            for (int e = 0; e < VE; ++e) {
              if constexpr (BWD) {
                const A y = E::up(vx[u].e[e]), g = E::up(vg[u].e[e]);
                s[e] = s[e] + (lg ? g : g * y);
              } else {
                fold(m[e], s[e], E::up(vx[u].e[e]));
              }
            }
          }
        }
      }
      // slots 0 .. 7 of a wave: xor 8, 16, 32 of the lane number = xor 1, 2, 4 of the slot number
#pragma unroll
      for (int k = SM_LPR; k < RUA_WAVE; k <<= 1) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const A s2 = seg_shfl_xor(s[e], k);
          if constexpr (BWD) {
            s[e] = s[e] + s2;
          } else {
            const A m2 = seg_shfl_xor(m[e], k);
            combine(m[e], s[e], m2, s2);
          }
        }
      }
      // xor 8, 16 of the slot number = xor 1, 2 of the wave number, through LDS
      __syncthreads();
      if ((tid & (RUA_WAVE - 1)) < SM_LPR) {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          xch[((w * SM_LPR + l) * VE + e) * 2] = m[e];
          xch[((w * SM_LPR + l) * VE + e) * 2 + 1] = s[e];
        }
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        A vm[RUA_WAVES_PER_BLOCK], vs[RUA_WAVES_PER_BLOCK];
#pragma unroll
        for (int k = 0; k < RUA_WAVES_PER_BLOCK; ++k) {
          vm[k] = xch[(((w ^ k) * SM_LPR + l) * VE + e) * 2];
          vs[k] = xch[(((w ^ k) * SM_LPR + l) * VE + e) * 2 + 1];
        }
        if constexpr (BWD) {
          s[e] = (vs[0] + vs[1]) + (vs[2] + vs[3]);
        } else {
          combine(vm[0], vs[0], vm[1], vs[1]);
          combine(vm[2], vs[2], vm[3], vs[3]);
          combine(vm[0], vs[0], vm[2], vs[2]);
          m[e] = vm[0];
          s[e] = vs[0];
        }
      }
      if (mode == SEG_PARTIAL) {
        if (tid < SM_LPR) {
          A* p = ws + ((((b * maxblk + blk) * n_chunks + c) * SM_LPR + l) * VE) * 2;
#pragma unroll
          for (int e = 0; e < VE; ++e) { p[e * 2] = m[e]; p[e * 2 + 1] = s[e]; }
        }
      } else {
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          if constexpr (BWD) S[e] = S[e] + s[e];
          else combine(M[e], S[e], m[e], s[e]);
        }
      }
    }
    if (mode == SEG_PARTIAL) return;
  }
  if (!active) return;
  if constexpr (!BWD) {
#pragma unroll
    for (int e = 0; e < VE; ++e) S[e] = lg ? seg_log(S[e]) : (A)1 / S[e];
  }

  // walk 2
  for (int64_t tt = tb + q; tt < te; tt += (int64_t)SM_SLOTS * UNR) {
    Vec vx[UNR], vg[UNR];
    int64_t rows[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t t = tt + (int64_t)u * SM_SLOTS;
      rows[u] = -1;
      if (t >= te) continue;
      const int64_t row = token_to_row(L, b, t, len);
      if (row < 0 || row >= L.n_rows) continue;
      rows[u] = row;
      if (resident) {
        vx[u] = slab[t * SM_LPR + l];
        if constexpr (BWD) vg[u] = slab[((int64_t)cap_rows + t) * SM_LPR + l];
      } else {
        ld(xin, row, vx[u]);
        if constexpr (BWD) ld(gin, row, vg[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (rows[u] < 0) continue;
      Vec o;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const A g = BWD ? E::up(vg[u].e[e]) : (A)0;
        o.e[e] = E::down(finish<BWD, A>(E::up(vx[u].e[e]), g, M[e], S[e], lg));
      }
      st(rows[u], o);
    }
  }
  if ((L.kind == RUA_LEFT || L.kind == RUA_RIGHT) && blk == 0) {
    Vec z;
#pragma unroll
    for (int e = 0; e < VE; ++e) z.e[e] = E::down((A)0);
    for (int64_t j = q; j < L.T_phys; j += SM_SLOTS) {
      if (!is_pad(L, j, len)) continue;
      const int64_t row = b * L.T_phys + j;
      if (row < L.n_rows) st(row, z);
    }
  }
}

// ---------------------------------------------------------------- host side
// the cut form keeps (max, sum) — the backward: (unused, sum) — per block and (padded) column: two accumulators
static seg_plan sm_make_plan(const rua_layout& L, int64_t H, int32_t dtype) {
  const int es = seg_esize(dtype, false);
  return seg_make_plan(L, H, es, 2 * (es == 8 ? 8 : 4));
}

template <typename E, bool BWD>
static int sm_launch(const rua_layout& L, const void* x, const void* g, void* out, int64_t H, int32_t dtype, int lg,
                     void* ws, hipStream_t s) {
  using raw = typename E::raw;
  using A = typename E::acc;
  constexpr int VE = 16 / (int)sizeof(raw);
  const int64_t row_bytes = H * (int64_t)sizeof(raw);
  const uint64_t bases = (uint64_t)(uintptr_t)x | (uint64_t)(uintptr_t)g | (uint64_t)(uintptr_t)out;
  const char* dir = BWD ? "_backward" : "";
  if (bases % sizeof(raw)) return RUA_EALIGN;                 // (elements themselves are always aligned)

  if (row_bytes <= 16) {
    const seg_lanes ln = seg_lanes_geometry(row_bytes, bases, L.B);
    if (!ln.grid) return RUA_ERANGE;
    seg_trace("seg_softmax%s_lanes_kernel T=%s W=%d H=%d log=%d kind=%d", dir, E::name(), ln.W, (int)H, lg, L.kind);
    hipLaunchKernelGGL((seg_softmax_lanes_kernel<E, BWD>), dim3((unsigned)ln.grid), dim3(RUA_BLOCK), 0, s, L,
                       (const char*)x, (const char*)g, (char*)out, (int)H, ln.W, lg);
    return (int)hipGetLastError();
  }

  const seg_rows r = seg_rows_form(sm_make_plan(L, H, dtype), L, row_bytes, bases, ws != nullptr);
  const seg_plan& p = r.p;
  constexpr int XCH_BYTES = RUA_WAVES_PER_BLOCK * SM_LPR * VE * 2 * (int)sizeof(A);
  int cap = seg_slab_cap(L, r.cut, SM_SLOTS, BWD ? SM_CAP_BWD : SM_CAP_FWD);
  size_t lds = XCH_BYTES + (size_t)cap * 128 * (BWD ? 2 : 1);
  if (!r.grid) return RUA_ERANGE;

  if (lds > 64 * 1024) {
    // more than 64 KiB of dynamic LDS has to be asked for, once per kernel AND DEVICE (the attribute belongs to the
    // device's copy of the function); where the runtime refuses, a smaller slab.  A device number beyond the table
    // asks on every launch.
    constexpr int MAX_DEV = 64;
    static std::atomic<int> big_ok[2][MAX_DEV];                // zero-initialised: 0 = not asked yet, 1 = granted, -1 = refused
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; }
    std::atomic<int> never{0};
    std::atomic<int>& st = dev >= 0 && dev < MAX_DEV ? big_ok[r.al ? 1 : 0][dev] : never;
    int v = st.load(std::memory_order_relaxed);
    if (v == 0) {
      const int want = XCH_BYTES + (BWD ? SM_CAP_BWD * 2 : SM_CAP_FWD) * 128;
      hipError_t e = hipSuccess;
      seg_with_al(r.al, [&](auto AL) {
        e = hipFuncSetAttribute((const void*)seg_softmax_rows_kernel<E, BWD, decltype(AL)::value>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, want);
      });
      v = e == hipSuccess ? 1 : -1;
      if (e != hipSuccess) (void)hipGetLastError();
      st.store(v, std::memory_order_relaxed);
    }
    if (v < 0) {
      cap = (64 * 1024 - XCH_BYTES) / (128 * (BWD ? 2 : 1)) / SM_SLOTS * SM_SLOTS;
      lds = XCH_BYTES + (size_t)cap * 128 * (BWD ? 2 : 1);
    }
  }
  return seg_launch_rows(
      r,
      [&](int mode) {
        seg_with_al(r.al, [&](auto AL) {
          hipLaunchKernelGGL((seg_softmax_rows_kernel<E, BWD, decltype(AL)::value>), dim3((unsigned)r.grid),
                             dim3(RUA_BLOCK), lds, s, L, (const raw*)x, (const raw*)g, (raw*)out, H, p.n_chunks, cap, mode,
                             r.cut ? p.maxblk : 1, (A*)ws, lg);
        });
      },
      [&](const char* phase) {
        if (phase)
          seg_trace("seg_softmax%s_stream_kernel T=%s AL=%d log=%d kind=%d cut=1 phase=%s blocks=%d chunks=%d", dir,
                    E::name(), (int)r.al, lg, L.kind, phase, p.maxblk, p.n_chunks);
        else
          seg_trace("seg_softmax%s_%s_kernel T=%s AL=%d log=%d kind=%d cut=0 cap=%d chunks=%d", dir,
                    cap > 0 ? "resident" : "stream", E::name(), (int)r.al, lg, L.kind, cap, p.n_chunks);
      });
}

template <bool BWD>
static int sm_dispatch(const rua_layout* lay, const void* x, const void* g, void* out, int64_t H, int32_t dtype,
                       int32_t lg, void* ws, void* stream) {
  const int es = seg_esize(dtype, false);
  int e;
  if ((e = seg_check_entry(lay, H, es)) != 0) return e;
  if (lay->B == 0 || lay->n_rows == 0 || H == 0) return 0;
  if (!x || !out || (BWD && !g)) return RUA_EINVAL;
  if (seg_too_large(lay, H, es)) return RUA_ERANGE;
#define RUA_SM(E) sm_launch<E, BWD>(*lay, x, g, out, H, dtype, lg ? 1 : 0, ws, (hipStream_t)stream)
  RUA_DISPATCH_FLOAT(dtype, RUA_SM);
#undef RUA_SM
}

}  // namespace rua

extern "C" int64_t rua_softmax_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype) {
  if (rua::sm_check_layout(lay) != 0) return 0;
  return rua::sm_make_plan(*lay, H, dtype).ws_bytes;
}

extern "C" int rua_segment_softmax(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype,
                                   int32_t log, void* ws, void* stream) {
  return rua::sm_dispatch<false>(lay, data, nullptr, out, H, dtype, log, ws, stream);
}

extern "C" int rua_segment_softmax_backward(const rua_layout* lay, const void* y, const void* grad_out, void* grad_in,
                                            int64_t H, int32_t dtype, int32_t log, void* ws, void* stream) {
  if (y && y == grad_in) return RUA_EINVAL;
  return rua::sm_dispatch<true>(lay, y, grad_out, grad_in, H, dtype, log, ws, stream);
}
