// rua_compress_plan.h — what rua_segment_compress_plan decides BEFORE its first HIP call beyond rua_seg_plan.h, as
// plain host C++ (no HIP header): the length it refuses and the element of its workspace.  The forms of the plan, its
// grid and its workspace are the family's offsets scan (seg_make_scan_plan); layout and entry checks, the length bound,
// the cut rule and the geometry of the move are rua_seg_plan.h too.  tests/c/compress_plan_host.cpp walks this header.
#pragma once
#include "rua_seg_plan.h"

namespace rua {

constexpr int64_t CP_MAX_LEN = 0x7fffffffLL;     // a rank is an int32: sequences of 2^31 tokens or more are refused
constexpr int CP_WS_ELEM_BYTES = 4;              // the cut form keeps one int32 count per (sequence, block)

static bool cp_too_long(const rua_layout& L) { return sm_len_bound(L) > CP_MAX_LEN; }

}  // namespace rua
