// rua_join.hip — per-sequence join and unjoin: glue ragged batches together along time, and cut one at per-sequence
// boundaries (rua_segment_join_lens, rua_segment_unjoin_lens, rua_segment_join; include/rua.h).  An extension: the
// raggedness of the result is the SUM of its parts', and every token's place has a closed form —
//   token (b, u) of the joined side  <->  token (b, u - pre_k[b]) of part k,  pre_k[b] <= u < pre_(k+1)[b],
//   pre_k[b] = the lengths of the parts before k in sequence b (at most 8 loads per sequence)
// — so there is no per-token table of any kind: no rank, no index, no workspace.
// ONE move kernel walks the JOINED side sequence by sequence (token_to_row on both sides, so b is known by construction
// and any two kinds meet); `unjoin` only swaps which side is stored to.  A thread group owns WHOLE rows: the lengths, the
// prefixes and both row formulas are paid once per row, and a row is fetched by one group, not by one workgroup per
// 128-byte chunk.  Rows move as bits: plain vector loads and stores of the widest power of two (up to 16 bytes) that
// divides the row and every base address.
#include <stdio.h>
#include <stdint.h>
#include <atomic>
#include "rua_seg.h"
#include "rua_join_plan.h"

namespace rua {

extern std::atomic<int> g_trace_on;        // the dispatch trace (rua_reduce.hip)
void trace_add(const char* rec);

constexpr int JN_UNR = 4;                  // rows in flight per thread
static_assert(JN_MAX_PARTS == RUA_JOIN_MAX_PARTS, "rua_join_plan.h and rua.h name the same limit");
static_assert(JN_BLOCK == RUA_BLOCK, "rua_join_plan.h sizes its grids by the workgroup");

// the parts, by value in the kernel arguments: every index below is a compile-time constant of an unrolled loop, so a
// field is a scalar load and nothing is ever indexed by a lane's own part number
struct jn_parts {
  rua_layout p[JN_MAX_PARTS];
  char* data[JN_MAX_PARTS];
};
struct jn_sizes {
  const int64_t* sizes[JN_MAX_PARTS];      // [B] or NULL
  int64_t add[JN_MAX_PARTS];               // wanted[k][b] = (sizes[k] ? sizes[k][b] : 0) + add[k]
};

// ---------------------------------------------------------------- the lengths
// a thread per sequence.  out[b] = sum of the parts' clamped lengths; part_out[k * B + b] (optional) = the length of
// part k as its layout GIVES it (what a host mirror of that length vector holds)
__global__ __launch_bounds__(RUA_BLOCK) void seg_join_lens_kernel(jn_parts P, int n, int64_t B, int64_t* __restrict__ out,
                                                                  int64_t* __restrict__ part_out) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= B) return;
  int64_t sum = 0;
#pragma unroll
  for (int k = 0; k < JN_MAX_PARTS; ++k) {
    if (k >= n) continue;
    sum += safe_len(P.p[k], b);
    if (part_out) part_out[(int64_t)k * B + b] = seq_len(P.p[k], b);
  }
  out[b] = sum;
}

// out[k * B + b] = the length of part k of sequence b: what is wanted, clamped to what the parts before left over;
// own_out[b] (optional) = the length of sequence b as the layout GIVES it (what a host mirror of that vector holds)
__global__ __launch_bounds__(RUA_BLOCK) void seg_unjoin_lens_kernel(rua_layout J, jn_sizes S, int n,
                                                                    int64_t* __restrict__ out,
                                                                    int64_t* __restrict__ own_out) {
  const int64_t b = (int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x;
  if (b >= J.B) return;
  int64_t rest = safe_len(J, b);
  if (own_out) own_out[b] = seq_len(J, b);
#pragma unroll
  for (int k = 0; k < JN_MAX_PARTS; ++k) {
    if (k >= n) continue;
    int64_t c = (S.sizes[k] ? S.sizes[k][b] : 0) + S.add[k];
    if (c < 0) c = 0;
    if (c > rest) c = rest;
    out[(int64_t)k * J.B + b] = c;
    rest -= c;
  }
}

// ---------------------------------------------------------------- the move
// padding rows of sequence b of a LEFT / RIGHT side, as zeros: the positions q, q + rs, ... of [0, T_phys), every thread
// its pieces of the row.  A CAT storage that holds more rows than its lengths add up to (a join of device-only lengths
// sizes it by the parts' storages) has spare rows behind its last sequence: the group of that sequence zeroes them.
template <int W>
__device__ __forceinline__ void jn_zero_padding(const rua_layout& D, char* data, int64_t b, int64_t dlen, int64_t rb,
                                                int q, int rs, int64_t col0, int64_t colstep) {
  row_vec z;
  row_zero(z);
  if (D.kind == RUA_CAT && b == D.B - 1) {
    int64_t row = cat_off(D, b);
    if (row < 0) return;                         // (offsets that are no offsets: safe_len gave the sequence no token)
    for (row += dlen + q; row < D.n_rows; row += rs)
      for (int64_t col = col0; col < rb; col += colstep)
        row_st<W>(data + row * rb + col, rb - col >= 16 ? 16 : (int)(rb - col), z);
    return;
  }
  if (D.kind != RUA_LEFT && D.kind != RUA_RIGHT) return;
  for (int64_t j = q; j < D.T_phys; j += rs) {
    if (!is_pad(D, j, dlen)) continue;
    const int64_t row = b * D.T_phys + j;
    if (row >= D.n_rows) continue;
    for (int64_t col = col0; col < rb; col += colstep)
      row_st<W>(data + row * rb + col, rb - col >= 16 ? 16 : (int)(rb - col), z);
  }
}

// A group of 1 << tg_log2 threads walks one unit — sequence b of the joined side J, or (maxblk > 0) block `blk` of
// SEG_BLOCK_TOK of its tokens; 1 << g_log2 threads of the group own one row, 16 bytes each per step, so the group takes
// rs = 1 << (tg_log2 - g_log2) consecutive tokens per step, JN_UNR steps in flight: places first, then the loads, then
// the stores.  unjoin == 0: J is written (a token no part holds, and J's padding, as zeros); unjoin != 0: the parts
// are (a token J does not hold, and every part's padding, as zeros).  No collective: groups need nothing of each other.
template <int W>
__global__ __launch_bounds__(RUA_BLOCK) void seg_join_kernel(rua_layout J, jn_parts P, char* jdata, int64_t rb, int n,
                                                             int tg_log2, int g_log2, int maxblk, int unjoin) {
  const int tid = threadIdx.x;
  const int r = tid & ((1 << tg_log2) - 1);
  const int q = r >> g_log2, l = r & ((1 << g_log2) - 1);
  const int rs = 1 << (tg_log2 - g_log2);
  const int64_t unit = (int64_t)blockIdx.x * (RUA_BLOCK >> tg_log2) + (tid >> tg_log2);
  int64_t b = unit;
  int blk = 0;
  if (maxblk > 0) { blk = (int)(unit % maxblk); b = unit / maxblk; }
  if (b >= J.B) return;

  const int64_t jlen = safe_len(J, b);
  // per part, once per sequence: where it begins in the joined sequence (pre) and — CAT / LEFT / RIGHT, whose tokens
  // are consecutive rows — the row of its token 0 less that beginning (adj), so that token u of the joined sequence is
  // row adj + u of its part.  A PACK part's tokens are strided: its rows come from token_to_row token by token.
  int64_t pre[JN_MAX_PARTS + 1], adj[JN_MAX_PARTS];
  pre[0] = 0;
#pragma unroll
  for (int k = 0; k < JN_MAX_PARTS; ++k) {
    int64_t len = 0;
    adj[k] = 0;
    if (k < n) {
      len = safe_len(P.p[k], b);
      if (P.p[k].kind != RUA_PACK) adj[k] = token_to_row(P.p[k], b, 0, len) - pre[k];
    }
    pre[k + 1] = pre[k] + len;
  }
  const int64_t total = pre[JN_MAX_PARTS];

  // the tokens [tb, te) of the side that is written; the last block takes what a bound that understates left over
  // (seg_block_range, spelled out: through the helper this kernel compiles to another instruction stream)
  int64_t tb = 0, te = unjoin ? total : jlen;
  if (maxblk > 0) {
    tb = (int64_t)blk * SEG_BLOCK_TOK;
    if (blk < maxblk - 1 && te > tb + SEG_BLOCK_TOK) te = tb + SEG_BLOCK_TOK;
    if (tb > te) tb = te;
  }
  const int64_t col0 = (int64_t)l * 16, colstep = (int64_t)16 << g_log2;

  for (int64_t t0 = tb + q; t0 < te; t0 += (int64_t)rs * JN_UNR) {
    const char* src[JN_UNR];
    char* dst[JN_UNR];
#pragma unroll
    for (int i = 0; i < JN_UNR; ++i) {
      const int64_t u = t0 + (int64_t)i * rs;
      char* jp = nullptr;
      char* pp = nullptr;
      if (u < te) {
        if (u < jlen) {
          const int64_t row = token_to_row(J, b, u, jlen);
          if (row >= 0 && row < J.n_rows) jp = jdata + row * rb;
        }
        if (u < total) {
          // the part that holds u: the last one that begins at or before it (at most 8 compares; empty parts fall through)
          int sel = 0;
          int64_t row = adj[0] + u, rows = P.p[0].n_rows;
          char* base = P.data[0];
#pragma unroll
          for (int k = 1; k < JN_MAX_PARTS; ++k) {
            if (k < n && u >= pre[k]) { sel = k; row = adj[k] + u; rows = P.p[k].n_rows; base = P.data[k]; }
          }
#pragma unroll
          for (int k = 0; k < JN_MAX_PARTS; ++k) {
            if (k < n && P.p[k].kind == RUA_PACK && sel == k)
              row = token_to_row(P.p[k], b, u - pre[k], pre[k + 1] - pre[k]);
          }
          if (row >= 0 && row < rows) pp = base + row * rb;
        }
      }
      dst[i] = unjoin ? pp : jp;
      src[i] = unjoin ? jp : pp;
    }
    for (int64_t col = col0; col < rb; col += colstep) {
      const int nb = rb - col >= 16 ? 16 : (int)(rb - col);
      row_vec v[JN_UNR];
#pragma unroll
      for (int i = 0; i < JN_UNR; ++i) {
        row_zero(v[i]);
        if (dst[i] && src[i]) row_ld<W>(src[i] + col, nb, v[i]);
      }
#pragma unroll
      for (int i = 0; i < JN_UNR; ++i)
        if (dst[i]) row_st<W>(dst[i] + col, nb, v[i]);
    }
  }

  if (blk != 0) return;
  if (!unjoin) {
    jn_zero_padding<W>(J, jdata, b, jlen, rb, q, rs, col0, colstep);
  } else {
#pragma unroll
    for (int k = 0; k < JN_MAX_PARTS; ++k)
      if (k < n) jn_zero_padding<W>(P.p[k], P.data[k], b, pre[k + 1] - pre[k], rb, q, rs, col0, colstep);
  }
}

// ---------------------------------------------------------------- host side
static const char* jn_form_name(int form) {
  switch (form) {
    case JN_LANES: return "lanes";
    case JN_WAVE:  return "wave";
    case JN_ROWS:  return "rows";
  }
  return "?";
}

// a null or inconsistent layout, n_parts outside 1 .. 8, a part of another B: RUA_EINVAL (`H` < 0 likewise)
static int jn_check_layouts(const rua_layout* joined, const rua_layout* parts, int32_t n_parts, int64_t H) {
  int e;
  if (joined && (e = seg_check_entry(joined, H, 1)) != 0) return e;
  if (n_parts < 1 || n_parts > JN_MAX_PARTS || !parts) return RUA_EINVAL;
  for (int k = 0; k < n_parts; ++k) {
    if ((e = seg_check_entry(parts + k, H, 1)) != 0) return e;
    if (parts[k].B != (joined ? joined->B : parts[0].B)) return RUA_EINVAL;
  }
  return 0;
}

static int64_t jn_lens_grid(int64_t B) {
  const int64_t grid = (B - 1) / RUA_BLOCK + 1;
  return grid > 0x7fffffffLL ? 0 : grid;
}

static void jn_note_lens(const char* what, int n, int64_t B) {
  if (!g_trace_on.load(std::memory_order_relaxed)) return;
  char rec[120];
  snprintf(rec, sizeof rec, "%s parts=%d B=%lld", what, n, (long long)B);
  trace_add(rec);
}

}  // namespace rua

extern "C" int rua_segment_join_lens(const rua_layout* part_lays, int32_t n_parts, int64_t* out_lens,
                                     int64_t* part_lens, void* stream) {
  using namespace rua;
  int e;
  if ((e = jn_check_layouts(nullptr, part_lays, n_parts, 1)) != 0) return e;
  const int64_t B = part_lays[0].B;
  if (B == 0) return 0;
  if (!out_lens || out_lens == part_lens) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)out_lens % 8 || (uint64_t)(uintptr_t)part_lens % 8) return RUA_EALIGN;
  const int64_t grid = jn_lens_grid(B);
  if (!grid) return RUA_ERANGE;
  jn_parts P = {};
  for (int k = 0; k < n_parts; ++k) P.p[k] = part_lays[k];
  jn_note_lens("seg_join_lens_kernel", n_parts, B);
  hipLaunchKernelGGL(seg_join_lens_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, P,
                     (int)n_parts, B, out_lens, part_lens);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_unjoin_lens(const rua_layout* joined, const int64_t* const* sizes, const int64_t* size_add,
                                       int32_t n_parts, int64_t* out_lens, int64_t* own_lens, void* stream) {
  using namespace rua;
  int e;
  if ((e = seg_check_entry(joined, 1, 1)) != 0) return e;
  if (n_parts < 1 || n_parts > JN_MAX_PARTS || !sizes || !size_add) return RUA_EINVAL;
  if (joined->B == 0) return 0;
  if (!out_lens || out_lens == own_lens) return RUA_EINVAL;
  for (int k = 0; k < n_parts; ++k)
    if (sizes[k] && (sizes[k] == out_lens || sizes[k] == own_lens)) return RUA_EINVAL;
  if ((uint64_t)(uintptr_t)out_lens % 8 || (uint64_t)(uintptr_t)own_lens % 8) return RUA_EALIGN;
  for (int k = 0; k < n_parts; ++k)
    if ((uint64_t)(uintptr_t)sizes[k] % 8) return RUA_EALIGN;
  const int64_t grid = jn_lens_grid(joined->B);
  if (!grid) return RUA_ERANGE;
  jn_sizes S = {};
  for (int k = 0; k < n_parts; ++k) { S.sizes[k] = sizes[k]; S.add[k] = size_add[k]; }
  jn_note_lens("seg_unjoin_lens_kernel", n_parts, joined->B);
  hipLaunchKernelGGL(seg_unjoin_lens_kernel, dim3((unsigned)grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *joined, S,
                     (int)n_parts, out_lens, own_lens);
  return (int)hipGetLastError();
}

extern "C" int rua_segment_join(const rua_layout* joined, const rua_layout* part_lays, int32_t n_parts, void* joined_data,
                                void* const* part_data, int64_t row_bytes, int32_t unjoin, void* stream) {
  using namespace rua;
  int e;
  if (!joined) return RUA_EINVAL;
  if ((e = jn_check_layouts(joined, part_lays, n_parts, row_bytes)) != 0) return e;
  if (joined->B == 0 || row_bytes == 0) return 0;
  int64_t part_rows = 0;
  for (int k = 0; k < n_parts; ++k) part_rows |= part_lays[k].n_rows;
  if ((unjoin ? part_rows : joined->n_rows) == 0) return 0;              // a destination without rows
  if (!part_data || (joined->n_rows > 0 && !joined_data)) return RUA_EINVAL;
  uint64_t bases = (uint64_t)(uintptr_t)joined_data;
  for (int k = 0; k < n_parts; ++k) {
    if (part_lays[k].n_rows > 0 && !part_data[k]) return RUA_EINVAL;
    if (part_data[k] && part_data[k] == joined_data) return RUA_EINVAL;      // the output aliases an input
    if (unjoin)
      for (int i = 0; i < k; ++i)
        if (part_data[k] && part_data[k] == part_data[i]) return RUA_EINVAL;    // two outputs in one place
    bases |= (uint64_t)(uintptr_t)part_data[k];
  }
  if (seg_too_large(joined, row_bytes, 1)) return RUA_ERANGE;
  for (int k = 0; k < n_parts; ++k)
    if (seg_too_large(part_lays + k, row_bytes, 1)) return RUA_ERANGE;

  const jn_plan p = jn_make_plan(*joined, row_bytes, bases);
  if (!p.grid) return RUA_ERANGE;
  jn_parts P = {};
  for (int k = 0; k < n_parts; ++k) { P.p[k] = part_lays[k]; P.data[k] = (char*)part_data[k]; }
  if (g_trace_on.load(std::memory_order_relaxed)) {
    char rec[200];
    snprintf(rec, sizeof rec, "seg_join_kernel form=%s W=%d row_bytes=%lld parts=%d unjoin=%d joined=%d G=%d cut=%d blocks=%d",
             jn_form_name(p.form), p.W, (long long)row_bytes, (int)n_parts, unjoin ? 1 : 0, joined->kind, 1 << p.g_log2,
             (int)(p.maxblk > 0), p.maxblk);
    trace_add(rec);
  }
#define RUA_JN_LAUNCH(WV)                                                                                              \
  hipLaunchKernelGGL((seg_join_kernel<WV>), dim3((unsigned)p.grid), dim3(RUA_BLOCK), 0, (hipStream_t)stream, *joined,  \
                     P, (char*)joined_data, row_bytes, (int)n_parts, p.tg_log2, p.g_log2, p.maxblk, unjoin ? 1 : 0)
  RUA_DISPATCH_W(p.W, RUA_JN_LAUNCH)
#undef RUA_JN_LAUNCH
  return (int)hipGetLastError();
}
