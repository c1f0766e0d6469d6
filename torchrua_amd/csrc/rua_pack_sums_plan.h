// rua_pack_sums_plan.h — what the entry points of pack() that keeps its sums decide BEFORE their first HIP call, as plain
// host C++ (no HIP header): which calls are refused with which code, and the grid of the adjoint kernel.  The forward's
// own launch is planned by plan_reduce (rua_reduce_plan.h: the COPY form), whose answers this file does not touch.
#pragma once
#include <stdint.h>
#include "rua.h"
#include "rua_wave.h"

namespace rua {

// a source the fused walk takes and the PackedSequence it fills; fp32 accumulators only
inline int pack_sums_check(const rua_layout* src, const rua_layout* pack, int64_t H, int32_t dtype) {
  if (!src || !pack || H < 0 || src->B < 0) return RUA_EINVAL;
  if (dtype != RUA_F32 && dtype != RUA_BF16 && dtype != RUA_F16) return RUA_EINVAL;
  if (src->kind != RUA_CAT && src->kind != RUA_LEFT && src->kind != RUA_RIGHT) return RUA_EINVAL;
  if (src->kind == RUA_CAT && src->lens && !src->off) return RUA_EINVAL;
  if (pack->kind != RUA_PACK || pack->B != src->B || (pack->T > 0 && !pack->boff)) return RUA_EINVAL;
  return 0;
}

struct PackSumsBackwardPlan {
  int err, epl, lp_log2;       // epl: elements per 16-byte lane
  int64_t n_chunks;            // 64-lane column chunks per row: one wave per (sequence, chunk)
  unsigned grid;
};
// `ptrs`: the OR of grad_pack, grad_sums and grad_src
inline PackSumsBackwardPlan plan_pack_sums_backward(int64_t B, int64_t H, int esize, uintptr_t ptrs) {
  PackSumsBackwardPlan P = {};
  P.epl = 16 / esize;
  if (H % P.epl != 0 || ptrs % 16 != 0) { P.err = RUA_EALIGN; return P; }
  const int64_t lpr = H / P.epl;
  P.lp_log2 = lanes_log2(lpr);
  P.n_chunks = (lpr + RUA_WAVE - 1) / RUA_WAVE;
  if (B > 0x7fffffffLL / (P.n_chunks > 0 ? P.n_chunks : 1)) { P.err = RUA_ERANGE; return P; }
  P.grid = (unsigned)(B * P.n_chunks);
  return P;
}

}  // namespace rua
