// rua_reduce.hip — extern "C" entry points of the reductions; the kernels live in rua_reduce_impl.h and are
// instantiated per element type in rua_reduce_{f32,bf16,f16,f64}.hip.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <deque>
#include <mutex>
#include <string>
#include "rua_reduce_impl.h"
#include "rua_pack_sums_plan.h"

namespace rua {
// the dispatch trace (rua_debug_trace): process-global — autograd runs the backward on a thread of its own — and
// bounded, oldest record dropped first.  Off: one relaxed load per dispatch, nothing formatted, nothing allocated.
std::atomic<int> g_trace_on{0};            // (read by the softmax, scan and mover dispatchers too)
static std::mutex g_trace_mu;
static std::deque<std::string> g_trace_log;
constexpr size_t TRACE_CAP = 512;
static inline bool tracing() { return g_trace_on.load(std::memory_order_relaxed) != 0; }
void trace_add(const char* rec) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  if (g_trace_log.size() >= TRACE_CAP) g_trace_log.pop_front();
  g_trace_log.emplace_back(rec);
}
__attribute__((format(printf, 1, 2))) static std::string fmt(const char* f, ...) {
  char buf[320];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
// the OP template argument a launcher picks (max / min count their ties when `ties` is given)
static const char* op_name(int op, bool ties) {
  switch (op) {
    case RUA_SUM: return "sum";
    case RUA_MEAN: return "mean";
    case RUA_MAX: return ties ? "max_t" : "max";
    case RUA_MIN: return ties ? "min_t" : "min";
    case RUA_PROD: return "prod";
    case RUA_LOGSUMEXP: return "logsumexp";
  }
  return "?";
}
// ---- the records of a plan: one line per launch, the kernel template named as in rua_reduce_impl.h.  The trace and
// rua_debug_reduce_plan both print through these two, so a record cannot drift from what the launcher is handed.
template <typename Emit>
static void trace_reduce(const ReducePlan& P, const char* tname, Emit&& emit) {
  static const char* const kern[] = {"seg_reduce_ranks_kernel", "seg_reduce_team_kernel", "seg_reduce_kernel"};
  auto rec = [&](const char* k, bool nt, int wpb) {
    emit(fmt("%s T=%s EPL=%d OP=%s NT=%d COPY=%d CPW=%d WPB=%d team=%d glog=%d check=%d split=%d no_empty=%d", k, tname,
             P.epl, op_name(P.op, P.ties), nt ? 1 : 0, P.copy ? 1 : 0, P.cpw, wpb, P.team, P.glog, P.check,
             P.split ? 1 : 0, P.no_empty).c_str());
  };
  rec(kern[P.form], P.nt, P.wpb);
  if (P.split) {
    rec("seg_reduce_tail_kernel", P.nt, 1);
    rec("seg_reduce_combine_kernel", false, COMBINE_WAVES_MAX / P.cpw);
  }
}
template <typename Emit>
static void trace_backward(const BackwardPlan& P, const char* tname, Emit&& emit) {
  static const char* const kern[] = {"seg_backward_rows_kernel", "seg_backward_ranks_kernel", "seg_backward_walk_kernel",
                                     "seg_backward_kernel"};
  for (int k = 0; k < P.n_phases; ++k)
    for (const char* name : {kern[P.form], "seg_backward_tail_kernel"}) {
      emit(fmt("%s T=%s EPL=%d OP=%s NT=%d TV=%d chunks=%d span=%d split=%d phased=%d ties_final=%d pad_memset=%d", name,
               tname, P.epl, op_name(P.op, false), P.nt ? 1 : 0, P.tv[k], P.n_chunks > 1 ? 1 : 0, P.span ? 1 : 0,
               P.do_split ? 1 : 0, P.phased ? 1 : 0, P.ties_final ? 1 : 0, P.pad_memset ? 1 : 0).c_str());
      if (!P.do_split) break;
    }
}

static const ReduceEntry* entry_for(int dtype) {
  switch (dtype) {
    case RUA_F32: return &reduce_entry_f32();
    case RUA_BF16: return &reduce_entry_bf16();
    case RUA_F16: return &reduce_entry_f16();
    case RUA_F64: return &reduce_entry_f64();
  }
  return nullptr;
}

// plan, trace if on, launch.  `dry` (rua_debug_reduce_plan): the plan's records go there and nothing is launched.
static int dispatch_reduce(int dtype, int op, hipStream_t s, const rua_layout& L, const int64_t* perm, const void* data,
                           void* out, int64_t H, int include_self, uint64_t empty_bits, void* extreme, int64_t split,
                           void* ws, const rua_layout* CD, void* copy, void* ties, int hints, std::string* dry,
                           void* acc_out = nullptr) {
  const ReduceEntry* E = entry_for(dtype);
  if (!E) return RUA_EINVAL;
  const ReducePlan P = plan_reduce(L, E->esize, H, op, include_self, perm != nullptr, ws != nullptr, ties != nullptr,
                                   copy != nullptr,
                                   (uintptr_t)data | (uintptr_t)out | (uintptr_t)copy | (uintptr_t)ties | (uintptr_t)acc_out,
                                   split, hints);
  if (P.err) return P.err;
  if (dry) trace_reduce(P, E->name, [&](const char* r) { dry->append(r).push_back('\n'); });
  else if (tracing()) trace_reduce(P, E->name, trace_add);
  return dry ? 0 : E->reduce(P, s, L, perm, data, out, H, include_self, empty_bits, extreme, ws, CD, copy, ties, acc_out);
}

constexpr int EXTREME_WORDS_ENTRY = RUA_EXTREME_WORDS;     // 1 024 slots, flags, the reset ticket, one spare
__global__ void extreme_init_entry_kernel(unsigned long long* ext, int want_max_of_data) {
  (void)want_max_of_data;                       // the slots are zero-neutral for the maximum and the minimum alike
  for (int i = threadIdx.x; i < EXTREME_WORDS_ENTRY; i += blockDim.x) ext[i] = 0ull;   // slots, flags, ticket
}
// integer element types (rua_reduce_int.hip)
int reduce_int(int dtype, int op, hipStream_t s, const rua_layout& L, const int64_t* perm, const void* data, void* out,
               int64_t H, int include_self, int64_t split, void* ws);
int64_t reduce_int_ws_bytes(int64_t n_rows, int64_t H, int64_t split);

// a layout a reduce can walk (`perm`: the row indirection of scatter_*, over a CAT enumeration only)
static bool layout_ok(const rua_layout* lay, const int64_t* perm, int64_t H) {
  if (!lay || H < 0 || lay->B < 0) return false;
  if (lay->kind != RUA_CAT && lay->kind != RUA_PACK && lay->kind != RUA_LEFT && lay->kind != RUA_RIGHT) return false;
  if (lay->kind == RUA_CAT && lay->lens && !lay->off) return false;
  if (lay->kind == RUA_PACK && lay->T > 0 && !lay->boff) return false;
  return !perm || lay->kind == RUA_CAT;
}
// the three reduce entry points (extern "C" below); with `dry` they validate, plan and print, and launch nothing
static int segment_reduce_backward(const rua_layout* lay, const int64_t* perm, const void* data, const void* out,
                                   const void* grad_out, void* grad_in, int64_t H, int32_t dtype, int32_t op,
                                   int32_t include_self, int64_t split_rows, void* ws, void* ties, const void* self_in,
                                   void* stream, std::string* dry) {
  if (!layout_ok(lay, perm, H)) return RUA_EINVAL;
  if (self_in && !perm) return RUA_EINVAL;       // the old destination row only exists for scatter_*
  if (lay->B == 0 || H == 0 || lay->n_rows == 0) return 0;
  if (!data || !out || !grad_out || !grad_in) return RUA_EINVAL;
  const bool fill = (include_self & RUA_BWD_FILL_PADDING) != 0;
  const int tie_rule = (include_self & RUA_BWD_TIES_POSITIVE) ? BWD_TIES_POSITIVE : 0;   // rides in extra_count
  include_self &= 0xff;
  const bool final = include_self == RUA_TIES_FINAL && ties != nullptr;   // the forward counted them (ties_out)
  const int extra_count = (include_self == 1 ? 1 : 0) | tie_rule;
  const ReduceEntry* E = entry_for(dtype);
  if (!E) return RUA_EINVAL;
  const BackwardPlan P = plan_backward(*lay, E->esize, H, op, extra_count, perm != nullptr, ws != nullptr, ties != nullptr,
                                       final, self_in != nullptr, fill,
                                       (uintptr_t)data | (uintptr_t)out | (uintptr_t)grad_out | (uintptr_t)grad_in |
                                           (uintptr_t)ties | (uintptr_t)self_in, split_rows);
  if (P.err) return P.err;
  if (dry) trace_backward(P, E->name, [&](const char* r) { dry->append(r).push_back('\n'); });
  else if (tracing()) trace_backward(P, E->name, trace_add);
  return dry ? 0 : E->backward(P, (hipStream_t)stream, *lay, perm, data, out, grad_out, grad_in, H, extra_count, ws, ties,
                               self_in);
}

static int segment_reduce(const rua_layout* lay, const int64_t* perm, const void* data, void* out, int64_t H,
                          int32_t dtype, int32_t op, int32_t include_self, uint64_t empty_bits, void* extreme,
                          int64_t split_rows, void* ws, void* ties, void* stream, std::string* dry) {
  if (!layout_ok(lay, perm, H)) return RUA_EINVAL;
  if (lay->B == 0 || H == 0) return 0;
  if (!out || (lay->n_rows > 0 && !data)) return RUA_EINVAL;
  const bool clean = (op & RUA_OP_SCRATCH_CLEAN) != 0;
  const int hints = ((op & RUA_OP_NO_EMPTY) ? 1 : 0) | ((op & RUA_OP_SHORT_SEQS) ? 2 : 0);     // plan_reduce's hints
  op &= 0xff;
  if (ties && op != RUA_MAX && op != RUA_MIN) return RUA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype >= RUA_I64 && dtype <= RUA_U8) {        // integer tensors: scatter_* only (reduce.py:6-23)
    if (ties || lay->kind != RUA_CAT || dry) return RUA_EINVAL;
    return reduce_int(dtype, op, s, *lay, perm, data, out, H, include_self, split_rows, ws);
  }
  if (!dry && extreme && !clean && (op == RUA_MAX || op == RUA_MIN || op == RUA_LOGSUMEXP))
    hipLaunchKernelGGL(extreme_init_entry_kernel, dim3(1), dim3(256), 0, s, (unsigned long long*)extreme,
                       op == RUA_MIN ? 1 : 0);
  return dispatch_reduce(dtype, op, s, *lay, perm, data, out, H, include_self, empty_bits, extreme, split_rows, ws, nullptr,
                         nullptr, ties, hints, dry);
}

static int pack_reduce(const rua_layout* src, const rua_layout* pack, const void* data, void* pack_data, void* out,
                       int64_t H, int32_t dtype, int32_t op, uint64_t empty_bits, void* extreme, int64_t split_rows,
                       void* ws, void* stream, std::string* dry) {
  if (!src || !pack || H < 0 || src->B < 0) return RUA_EINVAL;
  if (src->kind != RUA_CAT && src->kind != RUA_LEFT && src->kind != RUA_RIGHT) return RUA_EINVAL;
  if (src->kind == RUA_CAT && src->lens && !src->off) return RUA_EINVAL;
  if (pack->kind != RUA_PACK || pack->B != src->B || (pack->T > 0 && !pack->boff)) return RUA_EINVAL;
  if (src->B == 0 || H == 0) return 0;
  if (!out || !pack_data || !data) return RUA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool clean = (op & RUA_OP_SCRATCH_CLEAN) != 0;
  const int hints = (op & RUA_OP_NO_EMPTY) ? 1 : 0;
  op &= 0xff;
  if (!dry && extreme && !clean && (op == RUA_MAX || op == RUA_MIN || op == RUA_LOGSUMEXP))
    hipLaunchKernelGGL(extreme_init_entry_kernel, dim3(1), dim3(256), 0, s, (unsigned long long*)extreme,
                       op == RUA_MIN ? 1 : 0);
  return dispatch_reduce(dtype, op, s, *src, nullptr, data, out, H, 0, empty_bits, extreme, split_rows, ws, pack, pack_data,
                         nullptr, hints, dry);
}

}  // namespace rua

using namespace rua;

extern "C" {

int rua_debug_trace(int32_t on) { return g_trace_on.exchange(on ? 1 : 0, std::memory_order_relaxed); }

int64_t rua_debug_trace_take(char* buf, int64_t cap) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  int64_t n = 0;
  if (!buf || cap <= 0) {                   // the size of the whole log, left in place
    for (const std::string& r : g_trace_log) n += (int64_t)r.size() + 1;
    return n;
  }
  while (!g_trace_log.empty() && n + (int64_t)g_trace_log.front().size() + 1 <= cap) {
    const std::string& r = g_trace_log.front();
    memcpy(buf + n, r.data(), r.size());
    n += (int64_t)r.size();
    buf[n++] = '\n';
    g_trace_log.pop_front();
  }
  return n;
}

int64_t rua_debug_reduce_plan(int32_t call, const rua_layout* lay, const rua_layout* pack, int64_t H, int32_t dtype,
                              int32_t op, int32_t include_self, int64_t split_rows, int32_t present, int32_t align,
                              char* buf, int64_t cap) {
  // stand-ins for the device pointers, never dereferenced: present ones are non-null, and `data` carries the low bits
  char* const there = (char*)(uintptr_t)0x1000;
  char* const data = there + (align & 0xff);
  auto opt = [&](int bit) { return (present & bit) ? there : nullptr; };
  std::string text;
  int rc = RUA_EINVAL;
  if (call == RUA_PLAN_SEGMENT_REDUCE)
    rc = segment_reduce(lay, (const int64_t*)opt(RUA_PLAN_PERM), data, there, H, dtype, op, include_self, 0, nullptr,
                        split_rows, opt(RUA_PLAN_WS), opt(RUA_PLAN_TIES), nullptr, &text);
  else if (call == RUA_PLAN_PACK_REDUCE)
    rc = pack_reduce(lay, pack, data, there, there, H, dtype, op, 0, nullptr, split_rows, opt(RUA_PLAN_WS), nullptr, &text);
  else if (call == RUA_PLAN_BACKWARD)
    rc = segment_reduce_backward(lay, (const int64_t*)opt(RUA_PLAN_PERM), data, there, there, there, H, dtype, op,
                                 include_self, split_rows, opt(RUA_PLAN_WS), opt(RUA_PLAN_TIES), opt(RUA_PLAN_SELF_IN),
                                 nullptr, &text);
  if (rc != 0) return rc;
  if (!buf || (int64_t)text.size() > cap) return RUA_ERANGE;
  memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}

int rua_reduce_team_waves(int64_t n_rows, int64_t B, int64_t row_bytes) {
  // what plan_reduce decides for an aligned payload whose rows are a multiple of 16 bytes — or of 8 bytes,
  // beyond one vector (16-byte lanes with an overlapping last lane)
  if (row_bytes <= 0 || row_bytes % 8 != 0 || (row_bytes % 16 != 0 && row_bytes <= 16) || row_bytes > 16 * RUA_WAVE) return 1;
  return reduce_team_waves(n_rows, B, lanes_log2((row_bytes + 15) / 16), B);      // one column chunk per row: units = sequences
}

int rua_segment_reduce_backward(const rua_layout* lay, const int64_t* perm, const void* data, const void* out,
                                const void* grad_out, void* grad_in, int64_t H, int32_t dtype, int32_t op,
                                int32_t include_self, int64_t split_rows, void* ws, void* ties,
                                const void* self_in, void* stream) {
  return segment_reduce_backward(lay, perm, data, out, grad_out, grad_in, H, dtype, op, include_self, split_rows, ws, ties,
                                 self_in, stream, nullptr);
}

int rua_scatter_self_grad(const int64_t* counts, int64_t S, int64_t H, const void* self_in, const void* out,
                          const void* grad_out, const void* aux, void* grad_self, int32_t dtype, int32_t op,
                          int32_t include_self, void* stream) {
  if (S < 0 || H < 0 || op < RUA_SUM || op > RUA_LOGSUMEXP) return RUA_EINVAL;
  if (S == 0 || H == 0) return 0;
  if (!counts || !grad_out || !grad_self) return RUA_EINVAL;
  const bool reads_self = include_self && (op == RUA_MAX || op == RUA_MIN || op == RUA_LOGSUMEXP);
  if (reads_self && (!self_in || !out)) return RUA_EINVAL;
  if (include_self && op == RUA_PROD && !aux) return RUA_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int inc = include_self ? 1 : 0;
  const ReduceEntry* E = entry_for(dtype);
  return E ? E->self_grad(s, counts, S, H, self_in, out, grad_out, aux, grad_self, op, inc) : RUA_EINVAL;
}

int64_t rua_reduce_ws_bytes(int64_t n_rows, int64_t H, int32_t dtype, int64_t split_rows) {
  if (split_rows <= 0 || n_rows <= 0 || H <= 0) return 0;
  if (dtype >= RUA_I64 && dtype <= RUA_U8) return reduce_int_ws_bytes(n_rows, H, split_rows);
  const int64_t acc = dtype == RUA_F64 ? 8 : 4;
  const int64_t max_extra = n_rows / split_rows;
  const int64_t chunks_scalar = (H + RUA_WAVE - 1) / RUA_WAVE;              // worst case: one element per lane
  const int64_t max_u = max_extra * chunks_scalar;
  const int64_t cols = chunks_scalar * RUA_WAVE * (dtype == RUA_F64 ? 2 : 8);  // >= n_chunks * 64 * EPL on any path
  return 32 + max_u * 64 + 2 * max_extra * 2 * cols * acc + 256;
}

int rua_segment_reduce(const rua_layout* lay, const int64_t* perm, const void* data, void* out, int64_t H,
                       int32_t dtype, int32_t op, int32_t include_self, uint64_t empty_bits, void* extreme,
                       int64_t split_rows, void* ws, void* ties, void* stream) {
  return segment_reduce(lay, perm, data, out, H, dtype, op, include_self, empty_bits, extreme, split_rows, ws, ties, stream,
                        nullptr);
}

int rua_pack_reduce(const rua_layout* src, const rua_layout* pack, const void* data, void* pack_data, void* out,
                    int64_t H, int32_t dtype, int32_t op, uint64_t empty_bits, void* extreme, int64_t split_rows,
                    void* ws, void* stream) {
  return pack_reduce(src, pack, data, pack_data, out, H, dtype, op, empty_bits, extreme, split_rows, ws, stream, nullptr);
}

int rua_pack_sums(const rua_layout* src, const rua_layout* pack, const void* data, void* pack_data, float* sums,
                  int64_t H, int32_t dtype, int64_t split_rows, void* ws, void* stream) {
  const int rc = pack_sums_check(src, pack, H, dtype);
  if (rc) return rc;
  if (src->B == 0 || H == 0) return 0;
  if (!sums || !pack_data || !data) return RUA_EINVAL;
  // (the plan answers RUA_EALIGN for rows or pointers off 16 bytes, before anything is launched)
  return dispatch_reduce(dtype, RUA_SUM, (hipStream_t)stream, *src, nullptr, data, nullptr, H, 0, 0, nullptr, split_rows, ws,
                         pack, pack_data, nullptr, 0, nullptr, sums);
}

int rua_pack_sums_backward(const rua_layout* src, const rua_layout* pack, const void* grad_pack, const float* grad_sums,
                           void* grad_src, int64_t H, int32_t dtype, void* stream) {
  const int rc = pack_sums_check(src, pack, H, dtype);
  if (rc) return rc;
  if (src->B == 0 || H == 0 || src->n_rows == 0) return 0;
  if (!grad_pack || !grad_sums || !grad_src) return RUA_EINVAL;
  const ReduceEntry* E = entry_for(dtype);
  const PackSumsBackwardPlan P = plan_pack_sums_backward(src->B, H, E->esize,
                                                         (uintptr_t)grad_pack | (uintptr_t)grad_sums | (uintptr_t)grad_src);
  if (P.err) return P.err;
  const bool nt = reduce_nt(src->n_rows, H, E->esize);
  if (tracing())
    trace_add(fmt("pack_sums_backward_kernel T=%s EPL=%d NT=%d chunks=%lld", E->name, P.epl, nt ? 1 : 0,
                  (long long)P.n_chunks).c_str());
  return E->pack_sums_backward((hipStream_t)stream, *src, *pack, grad_pack, grad_sums, grad_src, H, P.lp_log2, P.n_chunks, nt);
}

int rua_sums_cast(const void* in, void* out, int64_t n, int32_t dtype, int32_t to_f32, void* stream) {
  if (n < 0 || (dtype != RUA_F32 && dtype != RUA_BF16 && dtype != RUA_F16)) return RUA_EINVAL;
  if (n == 0) return 0;
  if (!in || !out || in == out) return RUA_EINVAL;
  const ReduceEntry* E = entry_for(dtype);
  const uintptr_t narrow = (uintptr_t)(to_f32 ? in : out), wide = (uintptr_t)(to_f32 ? out : in);
  if (narrow % E->esize != 0 || wide % 4 != 0) return RUA_EALIGN;
  return E->sums_cast((hipStream_t)stream, in, out, n, to_f32 ? 1 : 0);
}

int rua_fill_empty(const rua_layout* lay, void* out, int64_t H, int32_t dtype, int32_t op, void* extreme,
                   void* stream) {
  if (!lay || H < 0 || !extreme) return RUA_EINVAL;
  const int reset = (op & RUA_OP_SCRATCH_CLEAN) ? 1 : 0;
  op &= 0xff;
  if (op != RUA_MAX && op != RUA_MIN && op != RUA_LOGSUMEXP) return RUA_EINVAL;
  const int64_t n = lay->B * H;
  if (n == 0) return 0;
  if (!out) return RUA_EINVAL;
  const ReduceEntry* E = entry_for(dtype);
  if (!E) return RUA_EINVAL;
  const int wmax = op == RUA_MIN ? 1 : 0;
  if (tracing()) {
    const int VE = 16 / E->esize;    // fill_empty_body's own predicate
    const bool wide = (H % VE) == 0 && ((uintptr_t)out & 15) == 0;
    trace_add(fmt("fill_empty_kernel T=%s form=%s want_max=%d reset=%d", E->name,
                  wide && H / VE <= 8 ? "narrow" : wide ? "ballot" : "ballot_scalar", wmax, reset).c_str());
  }
  return E->fill_empty((hipStream_t)stream, *lay, out, H, wmax, extreme, reset);
}

}  // extern "C"
