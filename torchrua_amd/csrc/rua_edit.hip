// rua_edit.hip — per-sequence edit distance and alignment of the int64 tokens of a C / L / P / R container of
// hypotheses against the tokens of a SECOND ragged container of references (rua_segment_edit_forward,
// rua_segment_edit_backtrace; include/rua.h).  An extension: the number the ragged speech pipeline reports
// (WER / CER) and its split into substitutions, insertions and deletions.  Both layouts travel by value, sequence b is
// the same sequence in both (token_to_row resolves a P through `unsorted`).  Pure integer arithmetic: every result is
// exact and the same bits for every pair of layouts, every bucket and both forms.
//
//   D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (hyp[i-1] != ref[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
//
// Geometry (that of rua_ctc.hip).  A TEAM walks one pair, hyp token by hyp token, and the teams stride over b:
//   lanes form      a team is one wave (4 per workgroup); thread i keeps the R consecutive columns i R + 1 .. i R + R
//                   and their ref tokens in registers, R = 1 / 2 / 4 / 8 for S_max <= 64 / 128 / 256 / 512;
//   workgroup form  a team is one workgroup of 256 threads with R = 8 (512 < S_max <= 2048).
//
// A row is NOT walked serially along the left neighbour.  With t[j] = min(Dprev[j-1] + neq, Dprev[j] + 1) and t[0] = i,
//   D[j] = j + min_{k <= j} (t[k] - k)
// (unroll D[j] = min(t[j], D[j-1] + 1)).  So a row is an R-long chain in registers, whose running minimum m[r] of
// t - column the thread keeps, and ONE exclusive prefix-min E of the threads' last m across the team, seeded with i for
// column 0: a shuffle scan across the lanes; in the workgroup form each wave scans, lane 63 leaves the wave's minimum in
// LDS (two buffers of four words by the parity of a running row counter, one barrier per row; all four words are read
// by every lane: a broadcast, no bank conflict) and every wave folds the waves below it.  Then D[column] = column +
// min(E, m[r]).  E is also what the next row needs from the thread below: Dprev[i R] = i R + E of the row before, so no
// second cross-lane move exists.  Columns past S compute on a zero token and never reach a column at or below S.
//
// The hyp tokens and their rows are fetched 64 at a time, one per lane (every wave of a workgroup team fetches the same
// 64), and handed out per row by a lane read; the next 64 are requested before the current ones are walked.  The ref
// tokens and their rows are resolved once per pair.  Every row index is range-checked before it is dereferenced and the
// lengths are clamped to what the launch was sized for.
//
// Codes (only when the caller wants the alignment): once the row is final, cell (i, j), 1 <= j <= S, gets 0 / 1 if the
// diagonal candidate equals D[i][j] (0: the tokens are equal, 1: a substitution), else 2 if the up candidate does, else
// 3 (left) — one byte at codes[row of hyp token i - 1][j - 1], the rows S_max apart.  The backtrace (a thread per
// sequence) walks them from (T, S): at j == 0 only up, at i == 0 only left.
//
// KNOWN LIMITS: one long ref sends the whole batch to the workgroup form; one wave / workgroup walks all the tokens of
// a hyp; the code table costs rows x S_max bytes; the backtrace is one thread per sequence.
#include <stdio.h>
#include <stdint.h>
#include "rua_seg_launch.h"

namespace rua {

constexpr int64_t EDIT_MAX_GRID = 1024;
constexpr int EDIT_LANES_MAX_S = 512;                                   // S_max of the lanes form, at most
constexpr int EDIT_INF = 0x7fffffff;
static_assert(RUA_EDIT_MAX_REF <= RUA_BLOCK * 8, "the workgroup form holds 8 columns per thread");
static_assert(RUA_BLOCK == 4 * RUA_WAVE, "the workgroup form folds four waves");

enum : int { EDIT_MATCH = 0, EDIT_SUBST = 1, EDIT_UP = 2, EDIT_LEFT = 3 };

// the number of tokens of ref b, never more than the launch was sized for
__device__ __forceinline__ int edit_ref_len(const rua_layout& LR, int64_t b, int S_max) {
  const int64_t S = safe_len(LR, b);
  return (int)(S < S_max ? S : S_max);
}

// the row of token t of sequence b, range-checked where it is formed; -1: there is none
__device__ __forceinline__ int64_t edit_row(const rua_layout& L, int64_t b, int64_t t, int64_t len) {
  const int64_t r = token_to_row(L, b, t, len);
  return (r >= 0 && r < L.n_rows) ? r : (int64_t)-1;
}

// lane q's 64-bit value for the whole wave (q is the same in every lane)
__device__ __forceinline__ int64_t edit_lane_read(int64_t v, int q) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, q);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), q);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int edit_min(int a, int b) { return a < b ? a : b; }

// ---------------------------------------------------------------- forward: the distance, and the codes if wanted
template <int R, bool WG, bool CODES>
__global__ __launch_bounds__(RUA_BLOCK) void seg_edit_forward_kernel(rua_layout LH, rua_layout LR,
                                                                     const int64_t* __restrict__ hyp,
                                                                     const int64_t* __restrict__ ref,
                                                                     int64_t* __restrict__ dist,
                                                                     uint8_t* __restrict__ codes, int S_max) {
  __shared__ int wave_min[WG ? 2 * 4 : 1];
  const int lane = (int)(threadIdx.x & (RUA_WAVE - 1));
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int tid = WG ? wv * RUA_WAVE + lane : lane;
  const int64_t team = WG ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * RUA_WAVES_PER_BLOCK + wv;
  const int64_t teams = (int64_t)gridDim.x * (WG ? 1 : RUA_WAVES_PER_BLOCK);
  const int j0 = tid * R;                                       // the thread holds the columns j0 + 1 .. j0 + R
  unsigned step = 0;                                            // rows walked so far (the parity of the LDS buffer)

  for (int64_t b = team; b < LH.B; b += teams) {
    const int64_t T = safe_len(LH, b);
    const int S = edit_ref_len(LR, b, S_max);

    int64_t y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = j0 + r;
      const int64_t row = k < S ? edit_row(LR, b, k, S) : (int64_t)-1;
      y[r] = row >= 0 ? ref[row] : (int64_t)0;
    }
    auto fetch = [&](int64_t c0, int64_t& h, int64_t& row) {
      const int64_t t = c0 + lane;
      row = t < T ? edit_row(LH, b, t, T) : (int64_t)-1;
      h = row >= 0 ? hyp[row] : (int64_t)0;
    };

    int d[R];                                                   // row 0
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = j0 + 1 + r;
    int excl = 0;                                               // D[j0] - j0 of the row before

    int64_t h_nxt, row_nxt;
    fetch(0, h_nxt, row_nxt);
    for (int64_t c0 = 0; c0 < T; c0 += RUA_WAVE) {
      const int64_t h_cur = h_nxt, row_cur = row_nxt;
      fetch(c0 + RUA_WAVE, h_nxt, row_nxt);                     // the next 64 are in flight during these
      const int n = (int)(T - c0 < RUA_WAVE ? T - c0 : RUA_WAVE);
      for (int q = 0; q < n; ++q) {
        const int i = (int)(c0 + q) + 1;
        const int64_t h = edit_lane_read(h_cur, q);
        const int64_t row = edit_lane_read(row_cur, q);
        // the chain in registers
        int dg[R], m[R];
        int run = EDIT_INF;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int above_left = r == 0 ? j0 + excl : d[r >= 1 ? r - 1 : 0];
          dg[r] = above_left + (h != y[r] ? 1 : 0);
          run = edit_min(run, edit_min(dg[r], d[r] + 1) - (j0 + 1 + r));
          m[r] = run;
        }
        // the exclusive prefix-min of `run` across the team, seeded with i - 0 for column 0
        int e = __shfl_up(run, 1, RUA_WAVE);
        if (lane == 0) e = (!WG || wv == 0) ? i : EDIT_INF;
#pragma unroll
        for (int s = 1; s < RUA_WAVE; s <<= 1) {
          const int o = __shfl_up(e, s, RUA_WAVE);
          if (lane >= s) e = edit_min(e, o);
        }
        if constexpr (WG) {
          int* buf = wave_min + (step & 1u) * 4;
          if (lane == RUA_WAVE - 1) buf[wv] = edit_min(e, run);
          __syncthreads();
#pragma unroll
          for (int w = 0; w < 3; ++w) {
            if (w < wv) e = edit_min(e, buf[w]);
          }
        }
        ++step;
        excl = e;
        // the row is final
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int v = j0 + 1 + r + edit_min(e, m[r]);
          if constexpr (CODES) {
            if (j0 + r < S && row >= 0) {
              const int code = dg[r] == v ? (h != y[r] ? EDIT_SUBST : EDIT_MATCH) : (d[r] + 1 == v ? EDIT_UP : EDIT_LEFT);
              codes[row * (int64_t)S_max + j0 + r] = (uint8_t)code;
            }
          }
          m[r] = v;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = m[r];
      }
    }

    // D[T][S]: column 0 is T itself
    if (S == 0) {
      if (tid == 0) dist[b] = T;
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (j0 + 1 + r == S) dist[b] = (int64_t)d[r];
      }
    }
  }
}

// ---------------------------------------------------------------- the backtrace: a thread per sequence
__global__ __launch_bounds__(RUA_BLOCK) void seg_edit_backtrace_kernel(rua_layout LH, rua_layout LR,
                                                                       const uint8_t* __restrict__ codes,
                                                                       int64_t* __restrict__ positions,
                                                                       int64_t* __restrict__ subs,
                                                                       int64_t* __restrict__ ins,
                                                                       int64_t* __restrict__ dels, int S_max) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= LH.B) return;
  const int64_t T = safe_len(LH, b);
  int64_t i = T, j = edit_ref_len(LR, b, S_max);
  int64_t n_sub = 0, n_ins = 0, n_del = 0;
  int64_t row = i > 0 ? edit_row(LH, b, i - 1, T) : (int64_t)-1;
  while (i > 0) {
    // at j == 0 only up exists; a row outside the storage has no codes: up, so that the walk ends
    int c = EDIT_UP;
    if (j > 0 && row >= 0) c = codes[row * (int64_t)S_max + (j - 1)] & 3;
    if (c == EDIT_LEFT) {                                       // a deletion: ref token j - 1 has no partner
      ++n_del;
      --j;
      continue;
    }
    int64_t pos = -1;
    if (c == EDIT_UP) {
      ++n_ins;
    } else {
      pos = j - 1;
      n_sub += c;
      --j;
    }
    if (row >= 0) positions[row] = pos;
    --i;
    row = i > 0 ? edit_row(LH, b, i - 1, T) : (int64_t)-1;
  }
  subs[b] = n_sub;
  ins[b] = n_ins;
  dels[b] = n_del + j;                                          // at i == 0 only left exists
  seg_fill_padding(LH, b, T, 0, 1, [&](int64_t r) { positions[r] = 0; });
}

// ---------------------------------------------------------------- host side
static int edit_check_entry(const rua_layout* lh, const rua_layout* lr, int32_t S_max) {
  int e;
  if ((e = sm_check_layout(lh)) != 0) return e;
  if ((e = sm_check_layout(lr)) != 0) return e;
  if (lr->B != lh->B) return RUA_EINVAL;
  if (S_max < 0 || S_max > RUA_EDIT_MAX_REF) return RUA_EINVAL;
  return 0;
}

static int edit_bucket(int S_max) {                                     // R of the lanes form; 0: the workgroup form
  return S_max <= 64 ? 1 : S_max <= 128 ? 2 : S_max <= 256 ? 4 : S_max <= EDIT_LANES_MAX_S ? 8 : 0;
}

static unsigned edit_grid(int64_t B, bool wg) {
  const int64_t teams = wg ? B : (B - 1) / RUA_WAVES_PER_BLOCK + 1;
  return (unsigned)(teams < EDIT_MAX_GRID ? teams : EDIT_MAX_GRID);
}

template <bool CODES>
static void edit_launch(int R, unsigned grid, const rua_layout& LH, const rua_layout& LR, const void* hyp, const void* ref,
                        void* dist, void* codes, int S_max, hipStream_t s) {
#define RUA_EDIT_FWD(RR, WG)                                                                                           \
  hipLaunchKernelGGL((seg_edit_forward_kernel<RR, WG, CODES>), dim3(grid), dim3(RUA_BLOCK), 0, s, LH, LR,              \
                     (const int64_t*)hyp, (const int64_t*)ref, (int64_t*)dist, (uint8_t*)codes, S_max)
  switch (R) {
    case 1: RUA_EDIT_FWD(1, false); break;
    case 2: RUA_EDIT_FWD(2, false); break;
    case 4: RUA_EDIT_FWD(4, false); break;
    case 8: RUA_EDIT_FWD(8, false); break;
    default: RUA_EDIT_FWD(8, true); break;
  }
#undef RUA_EDIT_FWD
}

}  // namespace rua

extern "C" int rua_segment_edit_forward(const rua_layout* hyp, const rua_layout* ref, const void* hyp_tokens,
                                        const void* ref_tokens, void* distance, void* codes, int32_t S_max,
                                        void* stream) {
  using namespace rua;
  int e;
  if ((e = edit_check_entry(hyp, ref, S_max)) != 0) return e;
  if (hyp->B == 0) return 0;
  if (!distance || (hyp->n_rows > 0 && !hyp_tokens) || (ref->n_rows > 0 && !ref_tokens)) return RUA_EINVAL;
  if (hyp->n_rows + (int64_t)S_max >= 0x7fffffffLL) return RUA_ERANGE;
  if ((uintptr_t)hyp_tokens % 8 || (uintptr_t)ref_tokens % 8 || (uintptr_t)distance % 8) return RUA_EALIGN;
  const int R = edit_bucket(S_max);
  const unsigned grid = edit_grid(hyp->B, R == 0);
  seg_trace("seg_edit_forward_kernel S_max=%d form=%s R=%d codes=%d kind=%d rkind=%d grid=%u", S_max,
            R ? "lanes" : "workgroup", R ? R : 8, (int)(codes != nullptr), hyp->kind, ref->kind, grid);
  if (codes)
    edit_launch<true>(R, grid, *hyp, *ref, hyp_tokens, ref_tokens, distance, codes, S_max, (hipStream_t)stream);
  else
    edit_launch<false>(R, grid, *hyp, *ref, hyp_tokens, ref_tokens, distance, nullptr, S_max, (hipStream_t)stream);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_edit_backtrace(const rua_layout* hyp, const rua_layout* ref, const void* codes,
                                          void* positions, void* substitutions, void* insertions, void* deletions,
                                          int32_t S_max, void* stream) {
  using namespace rua;
  int e;
  if ((e = edit_check_entry(hyp, ref, S_max)) != 0) return e;
  if (hyp->B == 0) return 0;
  if (!substitutions || !insertions || !deletions) return RUA_EINVAL;
  if (hyp->n_rows > 0 && (!positions || (S_max > 0 && !codes))) return RUA_EINVAL;
  if (hyp->n_rows + (int64_t)S_max >= 0x7fffffffLL) return RUA_ERANGE;
  if ((uintptr_t)positions % 8 || (uintptr_t)substitutions % 8 || (uintptr_t)insertions % 8 || (uintptr_t)deletions % 8)
    return RUA_EALIGN;
  const int64_t grid = (hyp->B - 1) / RUA_BLOCK + 1;
  if (grid > 0x7fffffffLL) return RUA_ERANGE;
  seg_trace("seg_edit_backtrace_kernel S_max=%d kind=%d rkind=%d", S_max, hyp->kind, ref->kind);
  hipLaunchKernelGGL(seg_edit_backtrace_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *hyp,
                     *ref, (const uint8_t*)codes, (int64_t*)positions, (int64_t*)substitutions, (int64_t*)insertions,
                     (int64_t*)deletions, S_max);
  return (int)hipGetLastError();
}
