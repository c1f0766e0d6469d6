// rua_seg_launch.h — the host side the launchers of the fold operators (rua_softmax.hip, rua_scan.hip,
// rua_argreduce.hip, rua_linear_scan.hip, rua_norm.hip; rua_conv.hip and rua_pool.hip take the small helpers) share
// AFTER the decisions of rua_seg_plan.h: the dispatch trace, the switch over the float element types, AL as a template
// argument and the sequencing of a rows-form launch.  An operator keeps its pointer checks, its *_make_plan, the text
// of its records and its kernel argument list.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <type_traits>
#include "rua_seg.h"

namespace rua {

extern std::atomic<int> g_trace_on;        // the dispatch trace (rua_reduce.hip)
void trace_add(const char* rec);

static bool seg_tracing() { return g_trace_on.load(std::memory_order_relaxed) != 0; }

// one record of the dispatch trace.  seg_trace(fmt, ...) evaluates and formats nothing while the trace is off
__attribute__((format(printf, 1, 2))) static void seg_trace_add(const char* fmt, ...) {
  char rec[240];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(rec, sizeof rec, fmt, ap);
  va_end(ap);
  trace_add(rec);
}
#define seg_trace(...)                                                                                                 \
  do {                                                                                                                 \
    if (seg_tracing()) seg_trace_add(__VA_ARGS__);                                                                     \
  } while (0)

// return LAUNCH(element type) for a float dtype, RUA_EINVAL for any other.  An operator that also takes int64 answers
// RUA_I64 with its own element type before it
#define RUA_DISPATCH_FLOAT(dtype, LAUNCH)                                                                              \
  switch (dtype) {                                                                                                     \
    case RUA_F32:  return LAUNCH(sm_f32);                                                                              \
    case RUA_BF16: return LAUNCH(sm_bf16);                                                                             \
    case RUA_F16:  return LAUNCH(sm_f16);                                                                              \
    case RUA_F64:  return LAUNCH(sm_f64);                                                                              \
  }                                                                                                                    \
  return RUA_EINVAL

// f(std::true_type{}) or f(std::false_type{}): AL stays a template argument of the kernel (decltype(AL)::value)
template <typename F> static void seg_with_al(bool al, F f) {
  if (al) f(std::true_type{}); else f(std::false_type{});
}

// the sequencing of a rows-form launch (r = seg_rows_form, r.grid != 0), and nothing else.  `launch(mode)` is the
// operator's hipLaunchKernelGGL with its own grid; `trace(phase)` its record, phase == nullptr for the uncut form.
// Cut: both records, then SEG_PARTIAL and, unless that failed, SEG_FINISH; else one record and SEG_FULL.
template <typename Launch, typename Trace> static int seg_launch_rows(const seg_rows& r, Launch launch, Trace trace) {
  if (!r.cut) {
    trace(nullptr);
    launch(SEG_FULL);
    return (int)hipGetLastError();
  }
  trace("partial");
  trace("finish");
  launch(SEG_PARTIAL);
  const int e = (int)hipGetLastError();
  if (e) return e;
  launch(SEG_FINISH);
  return (int)hipGetLastError();
}

}  // namespace rua
