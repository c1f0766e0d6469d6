// rua_pack_sums.h — the kernels of pack() that keeps its sums, beside the fused forward (seg_reduce_kernel<COPY>, which
// stores the fp32 accumulators through SplitWs::acc_out): the adjoint for both cotangents at once, and the cast between
// the fp32 side buffer and the payload dtype.  Included by rua_reduce_impl.h (it uses its Unit / make_unit / elem), so
// each element type's translation unit instantiates them with the reducer's kernels.
#pragma once

namespace rua {

// The adjoint of the fused pack + sum when BOTH of its outputs carry a cotangent: the source row of token (b, t) gets
//   grad_src[row(b, t)] = grad_pack[boff[t] + rank(b)] + grad_sums[b]        (one fp32 add, rounded once)
// in ONE pass — N*H*e read, N*H*e written — where the reduce's backward followed by the adjoint move writes the payload
// twice.  The forward's walk, mirrored: one wave per (sequence, 64-lane column chunk) in rank order, UNROLL_T rows in
// flight, the PackedSequence's row table fetched 64 entries at a time.  16-byte lanes only (the forward's own
// condition); padding rows of a padded source are zeroed by the launcher.
template <typename T, int EPL, bool NT>
__global__ __launch_bounds__(RUA_WAVE) void pack_sums_backward_kernel(rua_layout L, rua_layout CD,
                                                                      const T* __restrict__ gpack,
                                                                      const typename elem<T>::acc* __restrict__ gsums,
                                                                      T* __restrict__ gsrc, int64_t H, int lp_log2,
                                                                      int64_t n_chunks) {
  using A = typename elem<T>::acc;
  struct alignas(16) Pack { T v[EPL]; };
  typedef unsigned int RawV __attribute__((ext_vector_type(4)));
  static_assert(sizeof(Pack) == 16, "16-byte lanes");
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x / n_chunks;
  if (q >= L.B) return;
  const Unit<T, EPL> U = make_unit<T, EPL, true>(L, CD, nullptr, q, (int64_t)blockIdx.x - q * n_chunks, H, lp_log2, lane);
  A add[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) add[e] = U.colok ? gsums[U.b * H + U.col + e] : (A)0;
  const int rpw = U.rpw;
  for (int64_t tblk = 0; tblk < U.len; tblk += RUA_WAVE) {
    const int64_t cv = (tblk + lane < U.len && tblk + lane < CD.T) ? CD.boff[tblk + lane] : -1;
    const int nblk = (U.len - tblk) < RUA_WAVE ? (int)(U.len - tblk) : RUA_WAVE;
    for (int k = 0; k < nblk; k += rpw * UNROLL_T) {
      int64_t srow[UNROLL_T];
      Pack p[UNROLL_T];
#pragma unroll
      for (int u = 0; u < UNROLL_T; ++u) {
        const int tl = k + u * rpw + U.rsub;
        const int64_t cb = __shfl(cv, tl & (RUA_WAVE - 1), RUA_WAVE);
        const int64_t prow = cb + U.q;
        srow[u] = -1;
        if (U.colok && tl < nblk && cb >= 0 && prow < CD.n_rows) srow[u] = U.base + tblk + tl;
        if (srow[u] >= L.n_rows) srow[u] = -1;       // lengths that run past either storage touch nothing
        if (srow[u] >= 0) {
          const T* src = gpack + prow * H + U.col;
          if (NT) {
            RawV raw = __builtin_nontemporal_load(reinterpret_cast<const RawV*>(src));
            __builtin_memcpy(&p[u], &raw, sizeof(Pack));
          } else {
            p[u] = *reinterpret_cast<const Pack*>(src);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL_T; ++u) {
        if (srow[u] < 0) continue;
        Pack o;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o.v[e] = elem<T>::down(elem<T>::up(p[u].v[e]) + add[e]);
        T* dst = gsrc + srow[u] * H + U.col;
        if (NT) {
          RawV raw;
          __builtin_memcpy(&raw, &o, sizeof(Pack));
          __builtin_nontemporal_store(raw, reinterpret_cast<RawV*>(dst));
        } else {
          *reinterpret_cast<Pack*>(dst) = o;
        }
      }
    }
  }
}

// the side buffer of rua_pack_sums <-> the payload dtype, elementwise (to_acc == 0: out = round(acc); 1: acc = widen(in))
template <typename T>
__global__ __launch_bounds__(RUA_BLOCK) void sums_cast_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t n,
                                                              int to_acc) {
  using A = typename elem<T>::acc;
  const int64_t i0 = ((int64_t)blockIdx.x * RUA_BLOCK + threadIdx.x) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    if (i >= n) break;
    if (to_acc) ((A*)out)[i] = elem<T>::up(((const T*)in)[i]);
    else ((T*)out)[i] = elem<T>::down(((const A*)in)[i]);
  }
}

template <typename T>
static int launch_pack_sums_backward(hipStream_t s, const rua_layout& L, const rua_layout& CD, const void* gpack,
                                     const void* gsums, void* gsrc, int64_t H, int lp_log2, int64_t n_chunks, bool nt) {
  using A = typename elem<T>::acc;
  constexpr int FULL = 16 / sizeof(T);
  if (L.kind == RUA_LEFT || L.kind == RUA_RIGHT) {          // the walk writes token rows only
    const hipError_t e = hipMemsetAsync(gsrc, 0, (size_t)L.n_rows * (size_t)H * sizeof(T), s);
    if (e != hipSuccess) return (int)e;
  }
  with_bool(nt, [&](auto nt_c) {
    hipLaunchKernelGGL((pack_sums_backward_kernel<T, FULL, decltype(nt_c)::value>), dim3((unsigned)(L.B * n_chunks)),
                       dim3(RUA_WAVE), 0, s, L, CD, (const T*)gpack, (const A*)gsums, (T*)gsrc, H, lp_log2, n_chunks);
  });
  return (int)hipGetLastError();
}
template <typename T>
static int launch_sums_cast(hipStream_t s, const void* in, void* out, int64_t n, int to_acc) {
  const int64_t blocks = (n + 4 * RUA_BLOCK - 1) / (4 * RUA_BLOCK);
  if (blocks > 0x7fffffffLL) return RUA_ERANGE;
  hipLaunchKernelGGL(sums_cast_kernel<T>, dim3((unsigned)blocks), dim3(RUA_BLOCK), 0, s, in, out, n, to_acc);
  return (int)hipGetLastError();
}
}  // namespace rua
