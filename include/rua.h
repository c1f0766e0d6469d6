/*
 * rua.h — C ABI of librua_hip.so: MI355X (gfx950) ragged-sequence row kernels.
 *
 * This is the drop-in boundary for the hot path of speedcell4/torchrua 0.5.1
 * (layout conversion cat/pack/left/right, select head/last/roll/rev/trunc,
 * segmented + scatter reduce).  The reference has no FFI of its own: its
 * boundary is the set of Python methods it monkey-patches onto the four layout
 * types.  Every entry point below cites the reference method(s) whose ATen
 * composition it replaces (paths relative to the reference checkout).
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; all index vectors int64
 *     (the reference's index dtype everywhere);
 *   - never allocates, never synchronises, never throws; work is enqueued on
 *     `stream` (a hipStream_t passed as void*); scratch is caller-provided;
 *   - returns 0 on success, a positive hipError_t if the HIP runtime refused
 *     the launch, or a negative RUA_E* code for a rejected argument;
 *   - stateless and re-entrant.
 */
#ifndef RUA_H_
#define RUA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RUA_ABI_VERSION 6

/* argument errors (negative so they cannot collide with hipError_t) */
#define RUA_EINVAL   (-1)  /* bad enum / null pointer / negative size      */
#define RUA_EALIGN   (-2)  /* pointer or row size not aligned as required   */
#define RUA_ERANGE   (-3)  /* size exceeds what the launch geometry covers  */

/* ---- layouts -------------------------------------------------------------
 * Logical coordinate of a token: (b, t), 0 <= t < len[b].  Flat storage row:
 *   CAT    row = off[b] + t                       core/get.py:25-26, layout/cat.py:79-81
 *   LEFT   row = b*T_phys + t                     core/get.py:41-42, layout/left.py:73-77
 *   PACK   row = boff[t] + unsorted[b]            core/get.py:57-58, layout/pack.py:43-45
 *   RIGHT  row = b*T_phys + (T_log - len[b]) + t  core/get.py:73-74, layout/right.py:74-79
 *   LIST   (destination only) row j holds token (bptr[j], tptr[j])   core/get.py tuple keys
 * Enumeration order of a layout's rows (= the order of X.ptr()):
 *   CAT/LEFT/RIGHT: for b: for t < len[b]         layout/cat.py:68-71
 *   PACK:           for t: for r < bsz[t]: (sorted[r], t)            layout/pack.py:23-27
 */
enum rua_kind { RUA_CAT = 0, RUA_LEFT = 1, RUA_PACK = 2, RUA_RIGHT = 3, RUA_LIST = 4 };

typedef struct rua_layout {
  int32_t kind;            /* enum rua_kind */
  int32_t tile_t_log2;     /* PACK with a tile table (below): bits 0-7 log2 of the time steps per tile (4 .. 6),
                              bits 8-15 log2 of the ranks per tile (4); a zero field = 4 (ABI <= 3: 16 x 16);
                              bits 16-23: R = 128 / row bytes (2, 4 or 8) when the table was built for windows that
                              begin up to R - 1 steps early — tile_start[c] counts the ranks alive at step
                              c * TT - (R - 1), and there are ceil((T + R - 1) / TT) chunks — so that the kernel may
                              align every rank's batch-major runs to 128-byte lines; 0 = plain windows;
                              bit 24 (ABI 5): no table — the tiles cover the whole (sequence x step) grid of a padded
                              DESTINATION, ceil(B / ranks) tiles per chunk of steps, n_tchunks = ceil(T_phys / steps):
                              P.left() / P.right() at narrow rows write tokens and fill in one pass;
                              bit 25 (ABI 5): the table counts tiles of ONE time step x (1 << bits 8-15) ranks
                              (n_tchunks = T): a roll inside the PackedSequence moves every step's rows as one run */
  int64_t n_rows;          /* storage rows: CAT/PACK: sum(len); LEFT/RIGHT: B*T_phys; LIST: M */
  int64_t B;               /* number of sequences */
  int64_t T_phys;          /* LEFT/RIGHT: rows per sequence in storage (data.size(1)) */
  int64_t T_log;           /* RIGHT: the T used for right alignment (reference: token_sizes.max()).
                              CAT: optional hint — the longest sequence when the caller knows it, 0 = unknown
                              (rua_enum_rows writes sequence by sequence only when no sequence can be a large
                              share of the launch; results never depend on it) */
  const int64_t* lens;     /* [B] or NULL                                   */
  int64_t len_add;         /* len[b] = (lens ? lens[b] : 0) + len_add       */
  const int64_t* off;      /* CAT: exclusive scan of lens, [B] (NULL when lens is NULL);
                              effective offset = off[b] + b*len_add         */
  const int64_t* boff;     /* PACK: exclusive scan of batch_sizes, [T]      */
  int64_t T;               /* PACK: number of time steps                    */
  const int64_t* sorted;   /* PACK: sorted_indices [B]                      */
  const int64_t* unsorted; /* PACK: unsorted_indices [B]                    */
  const int64_t* bptr;     /* LIST: [M]; NULL = all zeros (tptr then indexes ONE sequence,
                              e.g. a flat row gather `data[key]` against LEFT{B=1}; a negative
                              entry of such a flat list wraps by the source's n_rows, like
                              torch's own indexing in core/get.py:29, core/set.py:30)   */
  const int64_t* tptr;     /* LIST: [M]                                     */
  /* PACK, optional: a (rank x time) tile table that lets narrow-row C/L/R <-> P transposes move
   * multi-row runs on BOTH sides (rua_move_rows picks it up when rows are <= 64 bytes) .        */
  const int64_t* bsz;        /* PACK: device copy of batch_sizes [T].  CAT (optional, ABI 6): ONE word, the number of
                                lengths <= 0 (rua_exclusive_scan_i64's total[1]): 0 lets max / min / logsumexp skip
                                the tracking of the reference's global `initial` (rua_segment_reduce)            */
  const int64_t* tile_start; /* [n_tchunks + 1]: tile_start[c] = sum_{c'<c} ceil(batch_sizes[TT*c']/TR) (TT time steps, TR ranks per tile) */
  int64_t n_tchunks;         /* ceil(T / TT)                                                     */
  int64_t n_tiles;           /* tile_start[n_tchunks] (the caller knows it: batch_sizes is a host tensor) */
} rua_layout;

/* ---- per-sequence token maps: t_src = f(t_dst) ---------------------------- */
enum rua_tmap {
  RUA_T_SHIFT = 0,  /* t + arg            identity (arg=0), trunc (select/trunc.py:9-62)       */
  RUA_T_ROLL  = 1,  /* (t - arg) mod slen select/roll.py:6-13                                  */
  RUA_T_REV_S = 2,  /* slen - 1 - t       select/rev.py:6-41; last = REV_S with dlen = 1 (select/last.py:7-13) */
  RUA_T_REV_D = 3,  /* dlen - 1 - t       adjoint of REV_S (backward of last)                  */
  RUA_T_ZERO  = 4   /* 0                  broadcast one row per sequence (backward of sum)     */
};

#define RUA_MOVE_SCATTER 1  /* flags: enumerate `dst` layout rows as the SOURCE rows and write
                               them to the rows computed from `src` layout (core/set.py)        */
#define RUA_MOVE_NT_ON   2  /* force / forbid non-temporal payload accesses; default: on when the   */
#define RUA_MOVE_NT_OFF  4  /* destination is >= 512 MiB (cannot stay in the 256 MiB Infinity Cache) */
/* launch geometry of the mover (default: ~16 KiB of destination rows per workgroup, one contiguous span of tiles
 * per XCD on big launches; these override it, for A/B runs):
 * bits 4-7 = log2 of the destination rows one workgroup takes (2..8 -> 4..256 rows), */
#define RUA_MOVE_TILE_LOG2(k) (((k) & 0xf) << 4)
#define RUA_MOVE_XCD_SPAN_ON  256  /* every XCD takes ONE contiguous span of tiles (blockIdx % 8 picks the span) */
#define RUA_MOVE_XCD_SPAN_OFF 512  /* tiles in plain blockIdx order                                             */
#define RUA_MOVE_NO_TAIL8 1024     /* rows of 8 (mod 16) bytes: keep 8-byte lanes instead of 16-byte lanes + an 8-byte tail */
#define RUA_MOVE_NO_NARROW 2048    /* rows of one vector (1 .. 16 bytes): the generic kernel instead of the lane-per-row one */

/* K1. Exclusive prefix sum of n int64 (wavefront scan).  out[i] = sum(in[0..i)).
 * `ws` must hold rua_scan_ws_elems(n) int64.  If total != NULL it points at TWO device words (ABI 6; one before):
 * total[0] = sum(in), total[1] = #{i : in[i] <= 0} — of a length vector: the number of EMPTY sequences, which a CAT
 * layout may hand to rua_segment_reduce (rua_layout::bsz).
 * Replaces get_offsets, utils.py:16-19 (cumsum + roll + [0]=0). */
int64_t rua_scan_ws_elems(int64_t n);
int rua_exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t* total, int64_t n,
                           int64_t* ws, void* stream);

/* K3. PackedSequence metadata from lengths + the (host-sorted) descending order.
 *   unsorted[sorted[r]] = r                       utils.py:22-26 (invert_permutation)
 *   bsz[t] = #{b : len[b] > t}, t < T             core/view.py:47-58 (get_mask(..).sum(dim=0))
 * without materialising the B x T int64 mask (core/view.py:11-18). */
int rua_pack_meta(const int64_t* lens, const int64_t* sorted, int64_t B, int64_t T,
                  int64_t* unsorted, int64_t* bsz, void* stream);

/* K3 + K1 in one call — everything pack() derives on the device: rua_pack_meta's outputs plus
 *   boff[t] = sum(bsz[0..t))  (T entries)   and, if off != NULL,   off[b] = sum(lens[0..b))  (B entries).
 * Moderate sizes (T <= 2 048, B <= 131 072) take ONE launch instead of five; larger ones run the three steps back to
 * back.  `ws`: rua_scan_ws_elems(max(B, T)) int64 (only touched on the large path).  core/view.py:47-58 + utils.py:16-19. */
int rua_pack_prepare(const int64_t* lens, const int64_t* sorted, int64_t B, int64_t T, int64_t* unsorted,
                     int64_t* bsz, int64_t* boff, int64_t* off, int64_t* ws, void* stream);

/* K3b. token_sizes of a PackedSequence in original batch order:
 *   len[b] = #{t : bsz[t] > unsorted[b]}          core/view.py:21-25 (get_mask(P).sum(dim=1)) */
int rua_lens_from_pack(const int64_t* bsz, int64_t T, const int64_t* unsorted, int64_t B,
                       int64_t* lens, void* stream);

/* K2. Enumerate a layout's rows in ptr() order.  Any of the outputs may be NULL.
 *   batch_ptr[j], token_ptr[j]                    utils.py:7-13 (major_sizes_to_ptr), X.ptr()
 *   flat[j] = storage row of token j              layout/left.py:73-77, right.py:74-79 (X.idx()) */
int rua_enum_rows(const rua_layout* lay, int64_t n_tokens, int64_t* batch_ptr, int64_t* token_ptr,
                  int64_t* flat, void* stream);

/* get_mask / mask: out[b, t] = (t < len[b]) ? one : zero over a B x T grid of elem_bytes-wide
 * elements (1, 2, 4 or 8).  core/view.py:11-18, mask.py:6-14. */
int rua_mask(const int64_t* lens, int64_t B, int64_t T, void* out, int32_t elem_bytes,
             uint64_t zero_bits, uint64_t one_bits, void* stream);

/* K4/K5/K6/K7. The row mover.  For every storage row j of `dst` (token (b,t), or padding):
 *     ts = tmap(t);  if 0 <= ts < slen[b]: dst_row(j) = src_row(b, ts)  else  dst_row(j) = fill
 * Replaces every conversion in core/cast.py:8-71 (+ the new_full pre-fill of core/view.py:34-38,
 * 67-71: padding and payload are written in ONE pass), core/get.py / core/set.py tuple-key
 * indexing, select/head.py, select/last.py, select/roll.py, select/rev.py, select/trunc.py.
 * `fill16` is the fill element replicated to 16 bytes. Rows are row_bytes wide on both sides.
 * `pad_row` >= 0 makes PADDING rows of a LEFT/RIGHT destination copies of that source storage
 * row instead of `fill16` (select/roll.py:19-23,33-37: the reference pads its index tensor with
 * 0, so its padding rows come out as copies of storage row 0); -1 = use the fill. */
int rua_move_rows(const rua_layout* dst, const rua_layout* src, int32_t tmap, int64_t tmap_arg,
                  void* dst_data, const void* src_data, int64_t row_bytes,
                  const void* fill16, int64_t pad_row, int32_t flags, void* stream);

/* Backward of a row scatter  rows_of(src)[list] = value  (core/set.py:21-92; torch's index_put_ backward, which the
 * reference inherits through autograd: a clone, an index_put of zeros and an index gather):
 *   for every entry j of the LIST layout `list` (M entries), r = the storage row of `src` it names, resolved exactly
 *   as rua_move_rows(..., RUA_MOVE_SCATTER) resolves it (negative flat rows wrap; a pair that names no token is skipped):
 *     grad_value[j, :] = grad[r, :]      (zeros for a skipped entry)         if grad_value != NULL
 *     grad_raw[r, :]   = 0                                                   if grad_raw   != NULL
 *   and every other row of grad_raw is a copy of the same row of grad.
 * grad_raw must not alias grad (RUA_EINVAL).  Rows may repeat in the list: every repeat receives the row of `grad`,
 * and the result does not depend on the order the entries are served in (`grad` is only read, `grad_raw` only written).
 * With grad_raw != NULL the call is two launches in stream order — the mover's streaming copy of `grad`, then the
 * gather-and-zero kernel; with grad_raw == NULL the copy does not happen.  flags: 0, or RUA_MOVE_NT_ON / RUA_MOVE_NT_OFF
 * (default: non-temporal accesses when the larger output is >= 512 MiB, the mover's rule).
 * Never allocates, never synchronises; like rua_move_rows it accepts any alignment (narrower lanes) and returns the
 * same codes.  While the dispatch trace is on (below) it records `setitem_backward_copy` and
 * `setitem_backward_kernel ...`, one line per launch.  Added to ABI 6 (the version number did not move). */
int rua_setitem_backward(const rua_layout* list, const rua_layout* src, const void* grad, void* grad_value,
                         void* grad_raw, int64_t row_bytes, int32_t flags, void* stream);

/* ---- reductions ------------------------------------------------------------ */
enum rua_dtype {
  RUA_F32 = 0, RUA_BF16 = 1, RUA_F16 = 2, RUA_F64 = 3,
  /* integer element types (ABI 4): rua_segment_reduce only, over a CAT layout with or without `perm` — the
   * scatter_* of reduce.py:6-23 on integer tensors, which the reference hands to torch.index_reduce / index_add like
   * any other dtype.  SUM / MEAN / MAX / MIN / PROD in the element type itself, bit-exact: sums and products wrap,
   * MEAN is ATen's floor division by a count held in the same type (so the count wraps too); `extreme`, `ws`,
   * `ties_out` and `empty_bits` are ignored (empty sequences yield the op's identity unless include_self == 2),
   * LOGSUMEXP is RUA_EINVAL. */
  RUA_I64 = 4, RUA_I32 = 5, RUA_I16 = 6, RUA_I8 = 7, RUA_U8 = 8
};
#define RUA_TIES_FINAL 2   /* rua_segment_reduce_backward's include_self: see there */
#define RUA_BWD_FILL_PADDING 0x100  /* OR-ed into that include_self: also write zeros into the rows of a padded
                                      layout that hold no token (grad_in then needs no pre-zeroing)              */
#define RUA_BWD_TIES_POSITIVE 0x200 /* OR-ed into that include_self (MAX / MIN): tied extrema share a POSITIVE
                                      gradient (g / ties each) and each take a non-positive one WHOLE — what
                                      torch.segment_reduce's backward does (segment_max/min, reduce.py:34-41);
                                      without it ties share g / ties whatever the sign (index_reduce's backward:
                                      scatter_max/min, reduce.py:6-11)                                          */
enum rua_op {
  RUA_SUM = 0, RUA_MEAN = 1, RUA_MAX = 2, RUA_MIN = 3, RUA_PROD = 4, RUA_LOGSUMEXP = 5
};

/* K8/K9/K10/K11. out[b, :] = op over t < len[b] of data[row(b, t), :], accumulating in fp32
 * (fp64 for RUA_F64), for the sequences of `lay` in ANY layout:
 *   CAT   = torch.segment_reduce(data, op, lengths=lens)      reduce.py:34-61
 *   PACK  = the same over a PackedSequence without P.cat()     (core/cast.py:8-10 + reduce.py:44)
 *   LEFT/RIGHT = over the valid rows of a padded batch          segment.py:16-25, 38-47
 * `perm` (may be NULL) indirects CAT rows: row = perm[off[b]+t] — the sorted-by-destination
 * form of scatter_* (reduce.py:6-31).
 * Empty sequence -> `empty_bits` (the reference's `initial`: 0, 1, or the global min/max).
 * If `extreme` != NULL (MAX/MIN/LOGSUMEXP; RUA_EXTREME_WORDS uint64 of scratch, initialised by the library) the call
 * reproduces the reference's `initial = tensor.min()` / `.max()` (reduce.py:35,40,57) without its extra pass over the
 * data: every wave of the reduce folds the OPPOSITE extreme of the rows it reads into one of the 1 024 hashed slots
 * extreme[0..1023] (one atomic per wave) and raises flags in extreme[1024] — bit 0: some element is NaN (then `initial`
 * is NaN and poisons every segment), bit 1: some segment is empty.  rua_fill_empty then patches the output, every workgroup its share; with no NaN and no
 * empty segment (the common case) its workgroups read one word and leave.  (ABI <= 5 took a second walk over the
 * payload when a segment was empty; ABI 6 never reads the payload twice.)
 * include_self: 0 overwrite | 1 `out` already holds values that take part (scatter_* include_self) |
 *               2 rows of empty sequences are left untouched (torch.index_reduce semantics).
 * split_rows > 0 (with `ws` of rua_reduce_ws_bytes(lay->n_rows, H, dtype, split_rows) bytes) cuts sequences
 * longer than split_rows into parts handled by separate waves (published through a device-side work list,
 * fp32 partials folded in part order: deterministic); 0 = one wave streams each sequence.
 * Integer dtypes (RUA_I64 .. RUA_U8; CAT only, SUM / MEAN / MAX / MIN / PROD in the element type, as ATen's
 * index_reduce / index_add do): the same two arguments cut buckets longer than split_rows by POSITION into ranges of
 * split_rows, int64 partials in `ws` (exact in any order; two small launches when no bucket is long).
 * ties_out (MAX/MIN; may be NULL): [B, H] f32 (f64 for RUA_F64) that receives, per output element, how many elements
 * of the sequence equal it (with include_self == 1 the old row is folded into the result but not counted; rows that
 * include_self == 2 leaves untouched are not written: pre-zero the buffer) — what the backward needs, for free in the pass that
 * reads the payload anyway (rua_segment_reduce_backward with include_self = RUA_TIES_FINAL then takes ONE walk).
 * Bits that may be OR-ed into `op`:
 *   RUA_OP_SCRATCH_CLEAN  (here, in rua_pack_reduce and in rua_fill_empty) by a caller that keeps ONE persistent `extreme`
 *                         scratch of RUA_EXTREME_WORDS uint64 per stream, zeroed once when it was allocated: the scratch
 *                         arrives zeroed, so no initialising launch; rua_fill_empty (which must then be called with the
 *                         same bit) hands it back zeroed.
 *   RUA_OP_NO_EMPTY       (here and in rua_pack_reduce) the caller PROVES that no sequence is empty — lengths it holds on
 *                         the host, a PackedSequence whose batch_sizes[0] equals its sequence count: nothing will ever
 *                         ask for the global extreme, so the reduce does not track it (a NaN still poisons everything:
 *                         that needs no extreme).  Up to ABI 5 the bit meant "do not arm the second walk".  The device
 *                         can prove the same by itself: a CAT layout may carry in `bsz` a pointer to the number of
 *                         lengths <= 0, as rua_exclusive_scan_i64 leaves it in total[1] (rua_layout, below).
 * (Dropping the trailing launch altogether — the reduce's last wave patching the output, found by tickets — was built
 * and measured in round 5: no gain at the BASELINE shapes, a loss where waves are short; profiles/r05_self_patch_ab.txt.) */
#define RUA_EXTREME_WORDS    1027
#define RUA_OP_SCRATCH_CLEAN 0x100
#define RUA_OP_NO_EMPTY      0x200
/* rua_segment_reduce over a CattedSequence with rows narrower than 1 KiB: the caller KNOWS the lengths and vouches
 * that no sequence is far above the average (torchrua_amd: at most 8 x the average, or 64 rows).  When the sequences
 * are short (16 .. 64 rows on average by row width) every row slot of a wave then takes a sequence of its own — one
 * wave = one workgroup per sequence is bound by the workgroup dispatch rate there — and the wave walks to the longest of
 * them, hence the word.  (At rows of <= 32 bytes four sequences share a wave with or without it: that form checks its
 * own lengths, wave by wave.  Since ABI 6 so does every-row-slot-its-own-sequence when the word is NOT given — a batch
 * is short on average whatever the caller knows: rows / sequences — and a wave whose lengths are far apart walks them
 * one after the other; the word saves that check.)  A hint: results do not depend on it (sums to rounding: the fold's
 * association changes). */
#define RUA_OP_SHORT_SEQS    0x400
int64_t rua_reduce_ws_bytes(int64_t n_rows, int64_t H, int32_t dtype, int64_t split_rows);
/* Waves (1, 2 or 4) that share one sequence in rua_segment_reduce for an aligned payload of `row_bytes`-wide
 * rows (multiples of 16 bytes, or of 8 bytes beyond one vector), B sequences, n_rows rows in all — the launcher's own rule, exported so that a host planner pricing
 * `split_rows` (a unit streams team-times as fast) cannot drift from it. */
int rua_reduce_team_waves(int64_t n_rows, int64_t B, int64_t row_bytes);
int rua_segment_reduce(const rua_layout* lay, const int64_t* perm, const void* data, void* out,
                       int64_t H, int32_t dtype, int32_t op, int32_t include_self,
                       uint64_t empty_bits, void* extreme, int64_t split_rows, void* ws, void* ties_out,
                       void* stream);

/* Fused pack + reduce (an EXTENSION: the reference has no one-call equivalent; it is exactly
 * core/cast.py:41-49 followed by the reduction of reduce.py:34-61 over the packed rows).  One pass over
 * the payload of `src` (CAT/LEFT/RIGHT): every row is stored to its row of the PackedSequence `pack`
 * (boff[t] + unsorted[b]) AND folded into out[b, :].  The same PackedSequence, bit for bit, as rua_move_rows(pack <- src);
 * the same fp32 accumulation as rua_segment_reduce(pack) (bit-identical whenever that call gives each sequence to one wave —
 * few-but-long batches go through a team of waves there, which associates the partial sums differently), at 2/3 of the HBM traffic.  Needs H*sizeof(dtype) % 16 == 0 and 16-byte
 * aligned pointers (returns RUA_EALIGN otherwise: run the two-call form). */
int rua_pack_reduce(const rua_layout* src, const rua_layout* pack, const void* data, void* pack_data, void* out,
                    int64_t H, int32_t dtype, int32_t op, uint64_t empty_bits, void* extreme, int64_t split_rows,
                    void* ws, void* stream);

/* pack() that keeps the per-sequence sums of its one pass (what `pack(keep_sums=...)` calls).  rua_pack_reduce with
 * op = RUA_SUM, except that the sums are stored as the fp32 ACCUMULATORS, not rounded: sums[b, :] (fp32 [B, H], batch
 * order) is what rua_segment_reduce(pack, RUA_SUM) rounds to the payload dtype, so one side buffer serves any later
 * output dtype (rua_sums_cast).  dtype: RUA_F32 / RUA_BF16 / RUA_F16 (anything else RUA_EINVAL).  Sequences longer than
 * split_rows go through the work list of rua_segment_reduce (ws: rua_reduce_ws_bytes), folded in part order: deterministic.
 * Nothing is launched and the code says why when the call cannot be served: a null layout or pointer, a source that is
 * not CAT / LEFT / RIGHT, a `pack` of another batch size: RUA_EINVAL; rows that are not a multiple of 16 bytes or a
 * pointer (data, pack_data, sums) off a 16-byte boundary: RUA_EALIGN — the caller then packs with rua_move_rows and
 * keeps no sums; it never gets wrong ones.  Trace: the records of rua_pack_reduce (COPY=1). */
int rua_pack_sums(const rua_layout* src, const rua_layout* pack, const void* data, void* pack_data, float* sums,
                  int64_t H, int32_t dtype, int64_t split_rows, void* ws, void* stream);

/* The adjoint of rua_pack_sums when both outputs carry a cotangent, in one pass (N*H*e read, N*H*e written):
 *   grad_src[row(b, t)] = grad_pack[boff[t] + rank(b)] + grad_sums[b, :]       (added in fp32, rounded once)
 * grad_src has the storage of `src`; padding rows of a LEFT / RIGHT source are zeroed.  With one cotangent only the
 * existing calls are the adjoint: rua_segment_reduce_backward(src, RUA_SUM) for the sums, rua_move_rows(src <- pack) for
 * the payload.  One wave walks a whole sequence (no long-sequence split).  Codes as rua_pack_sums (RUA_EALIGN: rows or
 * pointers off 16 bytes).  Trace: `pack_sums_backward_kernel T= EPL= NT= chunks=`. */
int rua_pack_sums_backward(const rua_layout* src, const rua_layout* pack, const void* grad_pack, const float* grad_sums,
                           void* grad_src, int64_t H, int32_t dtype, void* stream);

/* n elements between the fp32 side buffer of rua_pack_sums and the payload dtype: to_f32 == 0 rounds in[fp32] to
 * out[dtype] (the rounding rua_segment_reduce applies to its accumulators), to_f32 != 0 widens in[dtype] to out[fp32].
 * dtype as in rua_pack_sums; a null pointer, in == out or n < 0: RUA_EINVAL; a pointer that is not aligned to its
 * element: RUA_EALIGN. */
int rua_sums_cast(const void* in, void* out, int64_t n, int32_t dtype, int32_t to_f32, void* stream);

/* Backward of rua_segment_reduce in one kernel (semantics of torch's
 * segment_reduce backward, which the reference inherits through autograd: reduce.py:34-61):
 *   SUM g | MEAN g/len | PROD g*prod(others) (zero factors handled like torch) | LOGSUMEXP g*exp(x-out) |
 *   MAX/MIN g/ties where x == out, else 0 (RUA_BWD_TIES_POSITIVE: g itself when g <= 0 or NaN).
 * grad_in has the storage of `data`; rows of padded layouts that hold no token are NOT written unless
 * RUA_BWD_FILL_PADDING is OR-ed into include_self (SUM / MEAN / LOGSUMEXP and MAX / MIN with RUA_TIES_FINAL then
 * write them in the same pass: the backward runs one storage row at a time, laid out like rua_move_rows).
 * With `perm` it is the gradient w.r.t. the SOURCE rows of scatter_* (reduce.py:6-31); include_self != 0 then
 * counts the old destination row in MEAN's divisor (MAX/MIN: seed `ties` with the old row's tie, below).
 * split_rows / ws as in rua_segment_reduce.
 * ties (MAX/MIN; may be NULL): [B, H] accumulators (f32, f64 for RUA_F64) that the caller pre-sets to the ties
 * the rows of `data` do not see (0, or 1 where the old destination row of a scatter_max/min with include_self
 * equals `out`).  The kernel adds every sequence's own ties (integer-valued float atomics: exact), then divides
 * the gradient by the total — which lets long sequences be split, and leaves the totals for the caller.
 * With ties == NULL each sequence is counted and applied by one wave (no splitting for MAX/MIN).
 * include_self == RUA_TIES_FINAL: `ties` already holds the complete counts (the forward's ties_out): no counting walk.
 * self_in (perm != NULL only; may be NULL): the old destination rows [B, H] of a scatter_* — the `tensor` argument of
 * reduce.py:6-31.  MAX/MIN with RUA_TIES_FINAL: the kernel itself adds the tie of the old row where it equals `out`
 * (torch's index_reduce backward counts it with and without include_self), so `ties` is the forward's ties_out
 * unchanged.  PROD with include_self == 1: the old row is one more factor of every source row's gradient
 * (g * tensor * prod(other sources), zero factors handled like torch). */
int rua_segment_reduce_backward(const rua_layout* lay, const int64_t* perm, const void* data, const void* out,
                                const void* grad_out, void* grad_in, int64_t H, int32_t dtype, int32_t op,
                                int32_t include_self, int64_t split_rows, void* ws, void* ties,
                                const void* self_in, void* stream);

/* Gradient of scatter_* w.r.t. the destination `tensor` (reduce.py:6-31; torch's index_add / index_reduce backward),
 * one elementwise launch over [S, H]:
 *   include_self != 0:  SUM g | MEAN g/(counts+1) | MAX/MIN (tensor == out) ? g/(aux+1) : 0 | PROD g*aux |
 *                       LOGSUMEXP g*exp(tensor - out)
 *   include_self == 0:  g in rows no index names (counts == 0: they keep `tensor`), 0 elsewhere.
 * counts[S]: bucket sizes (rua_index_buckets).  aux [S, H]: MAX/MIN — the source rows' tie counts (f32; f64 for
 * RUA_F64; rua_segment_reduce's ties_out; NULL = none); PROD — the product of each bucket's source rows in the
 * payload dtype (rua_segment_reduce into ones with include_self = 2).  self_in/out may be NULL where unused. */
int rua_scatter_self_grad(const int64_t* counts, int64_t S, int64_t H, const void* self_in, const void* out,
                          const void* grad_out, const void* aux, void* grad_self, int32_t dtype, int32_t op,
                          int32_t include_self, void* stream);

/* Per-sequence softmax / log_softmax (an EXTENSION, added to ABI 6 — the version number did not move: the reference
 * spells it as segment_logsumexp, reduce.py:56-61, followed by repeat_interleave, a subtraction and an exp over [N, H]
 * temporaries, for a CattedSequence only).  For every sequence b of `lay` (ANY layout) and column h, over t < len[b]:
 *   log == 0:  out[row(b,t), h] = exp(data[row(b,t), h] - lse[b,h])      lse[b,h] = logsumexp_t data[row(b,t), h]
 *   log != 0:  out[row(b,t), h] =     data[row(b,t), h] - lse[b,h]
 * i.e. torch.softmax(seq, dim=0) / torch.log_softmax(seq, dim=0) of every sequence on its own, NaN included: a column
 * of a sequence that holds NaN or +inf, or only -inf, is NaN throughout, and stays inside its sequence and column (no
 * global `initial`, no `extreme` scratch, no rua_fill_empty).  fp32 accumulation (fp64 for RUA_F64), every output
 * element rounded once; RUA_F32 / RUA_BF16 / RUA_F16 / RUA_F64 (integer dtypes: RUA_EINVAL).  An empty sequence owns no
 * row of CAT / PACK: nothing is written for it.  Padding rows of a LEFT / RIGHT result are written as zeros in the same
 * pass (no pre-zeroing) and padding rows of the input are never read.
 * The fold order of a (sequence, column) — blocks of 2 048 tokens in order; inside a block 32 interleaved chains joined
 * by a butterfly — depends on NOTHING but the sequence's length: not on the layout, the kernel form, the alignment or
 * `ws`.  The operator therefore commutes with the casts BIT FOR BIT: cat(softmax(z)) == softmax(cat(z)) etc.
 * Three kernel forms by row width and lengths: rows of one vector (<= 16 bytes) put consecutive tokens on consecutive
 * lanes, two sequences per wave; wider rows give a workgroup per (sequence x 128-byte column chunk), which keeps the
 * slab in LDS between the fold and the rewrite when the sequence has at most 512 rows (backward: 256) and otherwise walks
 * global memory twice; few but long sequences (fewer than 1 024 units whose length bound — CAT: T_log or n_rows, LEFT /
 * RIGHT: T_phys, PACK: T — is at least 8 192) are cut into their blocks across workgroups when `ws` is given:
 * rua_softmax_ws_bytes(lay, H, dtype) bytes (0 = never needed; ws == NULL = do not cut).  Two launches then.
 * A CAT layout's T_log, where it is given (> 0), must be a TRUE upper bound of every length: the cut form sizes `ws` and
 * its grid from it, and never touches `ws` or rows beyond that bound, so tokens of a longer sequence past
 * ceil(T_log / 2 048) blocks would be left unwritten.  T_log == 0 (unknown) is always safe: the bound is then n_rows.
 * `out` may equal `data` (every row is read before it is written, by the same wave or workgroup).  Any alignment is
 * accepted (narrower accesses).  While the dispatch trace is on (below) every launch records
 * `seg_softmax_lanes_kernel`, `seg_softmax_resident_kernel` or `seg_softmax_stream_kernel` (cut=1 phase=partial|finish for
 * the cut form) with key=value pairs. */
int64_t rua_softmax_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_softmax(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype, int32_t log,
                        void* ws, void* stream);
/* Its backward, from the forward's OUTPUT y alone:
 *   log == 0:  grad_in = y * (g - s),        s[b,h] = sum_t g * y
 *   log != 0:  grad_in = g - exp(y) * s,     s[b,h] = sum_t g
 * the sums in the forward's fold order; padding rows of grad_in are written as zeros.  grad_in may equal grad_out; y must
 * not alias grad_in (RUA_EINVAL).  Same forms, same `ws`; the trace names are `seg_softmax_backward_lanes_kernel` etc. */
int rua_segment_softmax_backward(const rua_layout* lay, const void* y, const void* grad_out, void* grad_in, int64_t H,
                                 int32_t dtype, int32_t log, void* ws, void* stream);

/* Per-sequence softmax-weighted sum — attention pooling (an EXTENSION, added to ABI 6 — the version number did not
 * move: the reference's users spell it as segment_logsumexp, repeat_interleave, exp, a broadcast multiply and segment_sum
 * over [N, H] temporaries, for a CattedSequence only).  `values` has rows of H elements, `scores` rows of G = H / D
 * elements in the same row order (the same layout `lay`), both of `dtype`; column h is weighted by score column h / D.
 * For every sequence b of `lay` (ANY layout) and column h, over t < len[b]:
 *   out[b, h] = sum_t exp(scores[row(b,t), h / D] - lse[b, h / D]) * values[row(b,t), h]
 *   lse[b, g] = logsumexp_t scores[row(b,t), g]
 * i.e. (torch.softmax(s_seq, dim=0)[..., None] * v_seq).sum(0) of every sequence on its own.  out is [B, H] of `dtype`;
 * lse is [B, G] in the accumulator type (float; double for RUA_F64), -inf for an empty sequence, and may be NULL.  An
 * empty sequence gives zeros.  A NaN or +inf score, or only -inf scores, make that (sequence, score column) NaN and touch
 * nothing else; a non-finite value poisons its own (sequence, column) even at weight 0.  fp32 accumulation (fp64 for
 * RUA_F64), every output element rounded once; RUA_F32 / RUA_BF16 / RUA_F16 / RUA_F64.  Padding rows of LEFT / RIGHT
 * values and scores are never read.
 * Checks: a null layout, an integer dtype, D <= 0 or H % D != 0 and an output that aliases an input (or the other
 * output) give RUA_EINVAL; B == 0, H == 0 or n_rows == 0 return 0 without a launch (the caller fills out / lse);
 * lengths are clamped to the storage and every row is range-checked, as in rua_segment_softmax.
 * The fold order of a (sequence, column) is the softmax's — blocks of 2 048 tokens in ascending order; inside a block 32
 * interleaved chains (chain r takes the tokens t = r mod 32, ascending, with a one-exp online update of (max, sum of
 * weights, weighted sum)) joined by a butterfly whose combine rescales both sides to the common max and is symmetric —
 * and depends on NOTHING but the sequence's length: the operator commutes with the casts BIT FOR BIT.  out = weighted
 * sum / sum of weights.  Two kernel forms by row width: rows of one vector (H * esize <= 16 bytes, 1-D values included)
 * put consecutive tokens on consecutive lanes, two sequences per wave; wider rows give a workgroup per (sequence x
 * 128-byte column chunk), 32 rows x 8 lanes of 16 bytes, a lane carrying one (max, sum) where D * esize is a multiple
 * of 16 and one per element otherwise.  The values are read once, the scores of a sequence once per column chunk (H *
 * esize / 128 times for wide rows with few score columns).  Any alignment is accepted (narrower accesses, the
 * same bits).  `ws` is reserved for cutting few-but-long sequences across workgroups: rua_softmax_pool_ws_bytes
 * returns 0 today, ws may be NULL, and one workgroup walks a whole sequence.
 * RUA_POOL_OUT_ACC OR-ed into `dtype`: `out` is written UNROUNDED, in the accumulator type — what a caller keeps for the
 * backward when the payload is bf16 / f16 (delta below is a difference's subtrahend: from a rounded `out` it would carry
 * the payload dtype's rounding error into grad_scores); the caller rounds it to the payload dtype itself, once.
 * While the dispatch trace is on every launch records `seg_pool_lanes_kernel` or `seg_pool_rows_kernel` with key=value
 * pairs (T= AL= D= kind= ...). */
#define RUA_POOL_OUT_ACC 0x100
int64_t rua_softmax_pool_ws_bytes(const rua_layout* lay, int64_t H, int64_t D, int32_t dtype);
int rua_segment_softmax_pool(const rua_layout* lay, const void* values, const void* scores, void* out, void* lse,
                             int64_t H, int64_t D, int32_t dtype, void* ws, void* stream);
/* Its backward, token-parallel given the forward's `out` and `lse` (both required), with p = exp(scores - lse):
 *   grad_values[row, h] = p[row, h / D] * grad_out[b, h]
 *   grad_scores[row, g] = p[row, g] * (sum_{h in g} values[row, h] * grad_out[b, h] - delta[b, g])
 *   delta[b, g]         = sum_{h in g} out[b, h] * grad_out[b, h]
 * ONE launch that reads the values once and writes both gradients once; either gradient pointer may be NULL (both NULL:
 * returns 0).  With RUA_POOL_OUT_ACC in `dtype`, `out` is read in the accumulator type (the forward's with the same
 * bit).  Padding rows of LEFT / RIGHT gradients are written as zeros.  The order of the sums over the D columns of a
 * score column is fixed by (H, D, dtype) alone: rows of one vector ascending; wider rows deal the columns in units (16
 * bytes when D * esize is a multiple of 16, else one element) round-robin to S = min(64, pow2ceil(units)) lanes, each
 * lane sums ascending and the lanes are joined by a butterfly.  A gradient that aliases any input or the other gradient:
 * RUA_EINVAL; the other checks are the forward's.  The trace record is `seg_pool_backward_kernel` (form=lanes|team). */
int rua_segment_softmax_pool_backward(const rua_layout* lay, const void* grad_out, const void* values,
                                      const void* scores, const void* out, const void* lse, void* grad_values,
                                      void* grad_scores, int64_t H, int64_t D, int32_t dtype, void* ws, void* stream);

/* Per-sequence mean / variance and standardize (an EXTENSION, added to ABI 6 — the version number did not move: the
 * reference's users spell it as segment_mean, repeat_interleave, a subtraction, a square, segment_mean again, rsqrt and
 * a multiply over [N, H] temporaries, for a CattedSequence only).  For every sequence b of `lay` (ANY layout) and column
 * h, with n = len[b] and c = correction, over t < n:
 *   mean[b,h] = (1/n) sum_t x        M2[b,h] = sum_t (x - mean[b,h])^2        var[b,h] = M2 / (n - c)
 *   standardize:  out[row(b,t), h] = (x - mean[b,h]) * rstd[b,h],   rstd = 1 / sqrt(M2 / (n - c) + eps)
 * i.e. torch.var_mean(seq, dim=0, correction=c) and (seq - mean) * rsqrt(var + eps) of every sequence on its own.
 * RUA_F32 / RUA_BF16 / RUA_F16 / RUA_F64 (integer dtypes: RUA_EINVAL); fp32 accumulation (fp64 for RUA_F64), every
 * output element rounded once.  `var` and `mean` are [B, H] of `dtype` (either may be NULL; both NULL: returns 0);
 * `rstd` is [B, H] in the accumulator type (float; double for RUA_F64) and may be NULL.  n - c <= 0 makes that
 * sequence's var, rstd and out NaN; an empty sequence gives NaN var and NaN mean and owns no row of CAT / PACK.  A NaN or
 * an infinity poisons its own (sequence, column) and nothing else; a constant column has var == 0 exactly.  Padding rows
 * of a LEFT / RIGHT input are never read; padding rows of a LEFT / RIGHT result are written as zeros in the same pass.
 * `correction` >= 0 and `eps` >= 0 are passed by value (negative: RUA_EINVAL).
 * The fold order of a (sequence, column) is the softmax's — blocks of 2 048 tokens in ascending order; inside a block 32
 * interleaved chains (chain r takes the tokens t = r mod 32, ascending, Welford's update with one reciprocal per token
 * shared by the columns of a thread) joined by a butterfly with Chan's pairwise formula, both partners computing
 * merge(lower slot, upper slot); blocks joined in order — and depends on NOTHING but the sequence's length: the operators
 * commute with the casts BIT FOR BIT.
 * Kernel forms as for rua_segment_softmax: rows of one vector (<= 16 bytes) put consecutive tokens on consecutive lanes,
 * two sequences per wave; wider rows give a workgroup per (sequence x 128-byte column chunk), which keeps the slab in
 * LDS between the fold and the rewrite when the sequence has at most 480 rows (backward: 224 — what a 64 KiB budget
 * leaves) and otherwise walks global memory twice; few but long sequences (fewer than 1 024 units whose length bound is
 * at least 8 192) are cut into their blocks across workgroups when `ws` is given: rua_norm_ws_bytes(lay, H, dtype) =
 *   B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * 2 * sizeof(accumulator)
 * bytes — (mean, M2), or the backward's two sums, per block and padded column — and 0 where the cut form is never
 * taken (ws == NULL = do not cut).  Two launches then.  A CAT layout's T_log, where given, must be a TRUE bound, as for
 * rua_segment_softmax.  rua_segment_var_mean is the standardize's first walk alone: it reads the payload once and writes
 * [B, H].  `out` may equal `data`; a [B, H] output that aliases an input or the other output: RUA_EINVAL.  B == 0,
 * H == 0 and n_rows == 0 return 0 without a launch (the caller fills var / mean).  Lengths are clamped to the storage,
 * every row is range-checked, any alignment is accepted (narrower accesses, the same bits).
 * RUA_NORM_MEAN_ACC OR-ed into `dtype` of rua_segment_var_mean[_backward]: `mean` is written (read) UNROUNDED, in the
 * accumulator type — what a caller keeps for the backward when the payload is bf16 / f16 (x - mean is a difference).
 * While the dispatch trace is on every launch records `seg_norm_lanes_kernel`, `seg_norm_resident_kernel` or
 * `seg_norm_stream_kernel` with key=value pairs (T= AL= cut= phase= cap= kind= W= op=standardize|var_mean). */
#define RUA_NORM_MEAN_ACC 0x100
int64_t rua_norm_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_var_mean(const rua_layout* lay, const void* data, void* var, void* mean, int64_t H, int32_t dtype,
                         int64_t correction, void* ws, void* stream);
int rua_segment_standardize(const rua_layout* lay, const void* data, void* out, void* rstd, int64_t H, int32_t dtype,
                            int64_t correction, double eps, void* ws, void* stream);
/* The backward of var_mean, token-parallel, one elementwise form for every width and alignment:
 *   grad_in = grad_var[b,h] * 2 (x - mean[b,h]) / (n - c) + grad_mean[b,h] / n
 * grad_var / grad_mean: [B, H] of `dtype`, either may be NULL (its term is dropped); `mean` as the forward wrote it (in
 * the accumulator type with RUA_NORM_MEAN_ACC).  Padding rows of grad_in are written as zeros.  grad_in may equal data;
 * grad_in aliasing mean or a cotangent: RUA_EINVAL.  The trace record is `seg_var_mean_backward_kernel`. */
int rua_segment_var_mean_backward(const rua_layout* lay, const void* data, const void* mean, const void* grad_var,
                                  const void* grad_mean, void* grad_in, int64_t H, int32_t dtype, int64_t correction,
                                  void* stream);
/* The backward of standardize, from the forward's OUTPUT y and its rstd alone:
 *   grad_in = rstd * (g - (1/n) sum_t g - y * (sum_t g * y) / (n - c))
 * the sums in the forward's fold order with `+`; padding rows of grad_in are written as zeros.  grad_in may equal
 * grad_out; y or rstd aliasing grad_in: RUA_EINVAL.  Same forms, same `ws`; the trace names are
 * `seg_norm_backward_lanes_kernel` etc. */
int rua_segment_standardize_backward(const rua_layout* lay, const void* y, const void* rstd, const void* grad_out,
                                     void* grad_in, int64_t H, int32_t dtype, int64_t correction, void* ws,
                                     void* stream);

/* Per-sequence inclusive cumsum (an EXTENSION, added to ABI 6 — the version number did not move: the reference has no
 * prefix operator; its users pad, call torch.cumsum along dim 1 and cast back).  For every sequence b of `lay` (ANY
 * layout) and column h:
 *   reverse == 0:  out[row(b,t), h] = sum over s <= t of data[row(b,s), h]
 *   reverse != 0:  out[row(b,t), h] = sum over s >= t of data[row(b,s), h]
 * i.e. torch.cumsum(seq, dim=0) of every sequence on its own: a NaN or an infinity poisons only the later (reverse: the
 * earlier) tokens of its own sequence and column.  RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16 — fp32 accumulation (fp64 for
 * RUA_F64), every output element rounded once — and RUA_I64, which wraps; any other dtype: RUA_EINVAL.  An empty
 * sequence owns no row of CAT / PACK: nothing is written for it; B == 0, H == 0 and n_rows == 0 return 0 without a
 * launch.  Padding rows of a LEFT / RIGHT result are written as zeros in the same pass (no pre-zeroing) and padding rows
 * of the input are never read.  Lengths are clamped to the storage and every row is range-checked.
 * The association order of a (sequence, column, direction), with u = t (reverse: u = len - 1 - t) the position along the
 * scan: groups of 8 positions are scanned by three doubling steps (p_j <- p_(j-d) + p_j for j >= d; d = 1, 2, 4); a tile
 * is 4 groups, whose totals g0 .. g3 precede the later groups as g0, g0 + g1, (g0 + g1) + g2, the tile's total being
 * ((g0 + g1) + g2) + g3; a block is 64 tiles (2 048 positions), whose carry adds the tile totals one after the other,
 * afresh in every block; the base of a block adds the totals of the blocks before it one after the other; and
 *   out = ((base + carry) + groups before) + prefix inside the group.
 * A term that does not exist is the additive identity (-0.0 for floats, so that the sign of a zero survives).  The
 * order depends on NOTHING but the sequence's length and the direction: not on the layout, the kernel form, the
 * alignment or `ws`.  The operator therefore commutes with the casts BIT FOR BIT — cat(cumsum(z)) == cumsum(cat(z))
 * etc. — and `reverse` equals reversing every sequence, scanning forward and reversing back, bit for bit.
 * Kernel forms by row width and lengths: rows of one vector (<= 16 bytes) put consecutive tokens on consecutive lanes,
 * two sequences per wave, the carry in registers; wider rows give a workgroup per (sequence x 128-byte column chunk),
 * 32 rows per step, the carry in registers again: the payload is read once and written once, there is no slab and no
 * second walk.  Few but long sequences (fewer than 1 024 units whose length bound — CAT: T_log or n_rows, LEFT / RIGHT:
 * T_phys, PACK: T — is at least 8 192) are cut into their blocks across workgroups when `ws` is given: phase 1 leaves
 * every block's total in `ws`, phase 2 adds the totals before a block in order and scans it (two launches; the payload
 * is read twice).  rua_cumsum_ws_bytes(lay, H, dtype) =
 *   B * ceil(bound / 2 048) * ceil(H * esize / 128) * (128 / esize) * (4, or 8 for RUA_F64 / RUA_I64)
 * bytes when the cut form applies, else 0 (0 = never needed; ws == NULL = do not cut).  A CAT layout's T_log, where it
 * is given (> 0), must be a TRUE upper bound of every length, as for rua_segment_softmax.
 * `out` may equal `data` (every row is read before it is written, by the same thread; the cut form's first launch only
 * reads).  Any alignment is accepted (narrower accesses).  While the dispatch trace is on (below) every launch records
 * `seg_cumsum_lanes_kernel` or `seg_cumsum_rows_kernel` (cut=1 phase=partial|finish for the cut form) with key=value
 * pairs (T=, AL=, rev=, kind=). */
int64_t rua_cumsum_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_cumsum(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype, int32_t reverse,
                       void* ws, void* stream);

/* Per-sequence running max / min with indices and logcumsumexp (EXTENSIONS, added to ABI 6 — the version number did not
 * move): the rest of torch's cum* family on rua_segment_cumsum's skeleton (csrc/rua_cumext.hip).  The positions along
 * the scan (u = t, reverse: u = len - 1 - t), the groups of 8, tiles of 32 and blocks of 2 048, the three kernel forms
 * (lanes for rows of one vector, rows, and the cut form when `ws` is given), the cut rule, the clamped lengths, the
 * zeroed padding rows of a LEFT / RIGHT result (in EVERY output; padding rows of the inputs are never read), the empty
 * returns (B == 0, H == 0, n_rows == 0: 0 without a launch) and the accepted alignments are those of
 * rua_segment_cumsum; what changes is the state that is combined.  Every combine absorbs its identity EXACTLY (it
 * returns the other operand), so a form that meets a carry that does not exist gives the bits of one that skips it.
 *
 * rua_segment_cumextreme: torch.cummax(seq, dim=0) (op == RUA_MAX) / torch.cummin (RUA_MIN; any other op RUA_EINVAL) of
 * every sequence on its own, per column, bit for bit in both outputs.  The state is (value, position) under ONE total
 * order: NaN above every number, -0.0 == +0.0, and among equals the LATER position along the scan wins (the opposite of
 * rua_segment_argreduce's "first wins"); once a NaN is met the value stays NaN and the index moves on to every later
 * NaN.  The combine picks one of its operands, so it is associative and idempotent: every association order, layout and
 * kernel form gives the same bits.  The identity is "no element" (position -1), not a -inf.  `values` (payload dtype)
 * holds the winner's bits, `indices` (int64, the storage shape of the payload) its token POSITION inside the sequence in
 * un-mirrored coordinates (so with `reverse` the EARLIER token wins among equals).  Either output may be NULL and is
 * then not written; both NULL, a null `data`, or values == indices: RUA_EINVAL.  RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16
 * / RUA_I64.  The cut form keeps a (value, position) pair per block and padded column:
 *   rua_cumextreme_ws_bytes = B * ceil(bound / 2 048) * ceil(H * esize / 128) * (128 / esize) * 16, or 0.
 *
 * rua_segment_cumextreme_backward: the adjoint of "gather by `indices`" for the `indices` of the forward whose direction
 * was `reverse`.  Along the scan `indices` is constant on a run and the head s of a run has indices[s] == s, so
 *   grad_in[s] = [indices[s] == s] * sum of grad[t] over the run of s.
 * A segmented scan, state (sum, run id), run AGAINST the forward's direction on the same skeleton: no atomics, fp32
 * accumulation (fp64 for RUA_F64), one rounding, one order per (sequence, column).  Tokens that never win and padding
 * rows get exact zeros whatever `grad` holds in the padding.  `indices` is compared, never dereferenced: any content is
 * memory-safe.  Float dtypes only; workspace: rua_cumextreme_ws_bytes.
 *
 * rua_segment_logcumsumexp: torch.logcumsumexp(seq, dim=0) of every sequence on its own.  The state is (m, s) with value
 * m + log s, combined as s = s_a * exp(m_a - M) + s_b * exp(m_b - M), M = max(m_a, m_b) — the softmax kernels'
 * convention — where the factor of the operand that holds M is exactly 1.  A token is (x, 1), -inf is the identity
 * (-inf, 0), a NaN is (-inf, NaN).  A prefix of only -inf gives -inf, +inf gives +inf from there on, a NaN poisons only
 * the later tokens of its own sequence and column.  One association order (the cumsum's) per (sequence, column,
 * direction): the operator commutes with the casts and `reverse` equals rev / scan / rev, bit for bit.  The float
 * dtypes; fp32 accumulation (fp64 for RUA_F64), one rounding.  The cut form keeps (m, s) per block and padded column:
 *   rua_logcumsumexp_ws_bytes = B * ceil(bound / 2 048) * ceil(H * esize / 128) * (128 / esize) * (8, or 16 for RUA_F64).
 *
 * rua_segment_logcumsumexp_backward: grad_in[s] = sum over t >= s (scan order) of grad[t] * exp(data[s] - out[t]) — the
 * SAME fold with exponents -out[t] and signed weights grad[t], run against the forward's direction and finished as
 * s_state * exp(m_state + data[s]).  A token with data[s] == -inf gets exactly 0 (torch gives NaN there: a documented
 * deviation).  Workspace: rua_logcumsumexp_ws_bytes.
 *
 * Checks of the four, before any HIP call: the layout, H < 0 and the dtype (RUA_EINVAL), the empty returns, null
 * pointers (RUA_EINVAL), a payload too large for 64-bit offsets (RUA_ERANGE), a pointer not aligned to its element
 * (RUA_EALIGN).  Trace: `seg_cumextreme_{lanes,rows}_kernel`, `seg_cumextreme_bwd_*`, `seg_logcumsumexp_*`,
 * `seg_logcumsumexp_bwd_*` with T=, W= / H= (lanes), AL=, rev= (the direction of THAT scan), kind=, op=, and cut= /
 * phase=partial|finish / blocks= / chunks= (rows). */
int64_t rua_cumextreme_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_cumextreme(const rua_layout* lay, const void* data, void* values /* NULL: not written */,
                           void* indices /* NULL: not written */, int64_t H, int32_t dtype, int32_t op, int32_t reverse,
                           void* ws, void* stream);
int rua_segment_cumextreme_backward(const rua_layout* lay, const void* grad, const void* indices, void* grad_in,
                                    int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream);
int64_t rua_logcumsumexp_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_logcumsumexp(const rua_layout* lay, const void* data, void* out, int64_t H, int32_t dtype,
                             int32_t reverse, void* ws, void* stream);
int rua_segment_logcumsumexp_backward(const rua_layout* lay, const void* grad, const void* data, const void* out,
                                      void* grad_in, int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream);

/* Per-sequence linear-chain CRF (an EXTENSION, added to ABI 6 — the version number did not move): the log partition
 * function, its gradients (the marginals) and Viterbi over the emissions [rows, K] of ANY layout (csrc/rua_crf.hip).
 * `emissions` is the storage of `lay` with rows of K elements, `transitions` [K, K] row-major (transitions[i, j]: tag i
 * at t-1, then tag j at t), `start` / `end` [K] or NULL (NULL adds 0 and gives the bits of a zeros tensor); all four in
 * the element type `dtype` (RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16).  The per-sequence results and the table `alpha` are
 * in the ACCUMULATOR type (float; double for RUA_F64) and are never rounded to a 16-bit type.  1 <= K <= RUA_CRF_MAX_TAGS.
 *
 * Geometry: one wave per sequence, lane j owns tag j; wave w of the launch walks sequences w, w + waves, ... (the
 * forward launches at most 1 024 workgroups, the backward at most 1 024 WAVES).  A kernel per element type, semiring
 * and tag bucket (K <= 8 / 16 / 32 / 64).  One very long sequence is walked by ONE wave: correct and slow (cutting it
 * needs K x K matrix products per block; out of scope).
 *
 * ONE evaluation order per (sequence, tag, step), whatever the layout (no contraction):
 *   alpha_0[j] = start[j] + x_0[j];   v_i = alpha_{t-1}[i] + transitions[i, j] for i = 0 .. K-1;
 *   RUA_CRF_LOG: m = max_i v_i, s = sum_i exp(v_i - m) in ascending i, alpha_t[j] = x_t[j] + (m + log s), or
 *                x_t[j] + (-inf) when m == -inf (an unreachable tag is -inf, never NaN; a NaN v_i makes alpha_t[j] NaN);
 *   RUA_CRF_MAX: the maximum under rua_segment_argreduce's order (a NaN beats every number, the first of equals wins),
 *                its i is the backpointer of (t, j), alpha_t[j] = x_t[j] + max;
 *   out[b] = the same fold of alpha_{n-1}[j] + end[j] over j (RUA_CRF_MAX: last[b] = its j).  An empty sequence gives
 *   out[b] = 0 (last[b] = -1).  -inf is a forbidden move; +inf is out of scope.  Padding rows are never read.
 *
 * rua_segment_crf_forward: `out` [B] always; RUA_CRF_LOG writes `alpha` [rows, K] (the storage layout of the
 * emissions; padding rows are not written) when it is not NULL; RUA_CRF_MAX writes `backptr` (one uint8 per (row, tag);
 * the rows of token 0 are not written) and `last` [B] int64, both required.
 * rua_segment_crf_backtrace: a launch of its own on the same stream; a thread per sequence walks `backptr` from
 * `last` and writes `tags` (int64, one per row of the storage; zeros in the padding rows of LEFT / RIGHT).
 * rua_segment_crf_backward (of RUA_CRF_LOG, with `grad` [B] the cotangent of `out`, `alpha` and `logz` what the forward
 * wrote): beta_{n-1} = end, beta_{t-1}[i] = logsumexp_j(transitions[i, j] + (x_t[j] + beta_t[j])) in ascending j,
 *   grad_emissions[t, j] = grad[b] * exp((alpha_t[j] + beta_t[j]) - logz[b])      (rounded once; padding rows: zeros)
 * and the sums over tokens and sequences grad_transitions [K, K], grad_start [K], grad_end [K] (element type; each may
 * be NULL).  A sequence with logz == -inf gets exact zeros and adds nothing.  No float atomics: every wave leaves one
 * part [K * K + 2 K] in `ws` and a finish launch adds the parts in part order — bitwise reproducible for the same
 * container.  `ws` is required when one of the three sums is wanted:
 *   rua_crf_ws_bytes(lay, K, dtype) = 4 * min(ceil(B / 4), 256) * (K * K + 2 * K) * sizeof(acc), 0 for B == 0.
 *
 * Checks, before any HIP call: a null layout, a dtype outside the four, K outside [1, 64], an unknown semiring
 * (RUA_EINVAL); B == 0 returns 0 without a launch; a missing required pointer (RUA_EINVAL); a table too large for
 * 64-bit offsets (RUA_ERANGE); a pointer not aligned to its element (RUA_EALIGN).  Trace: `seg_crf_forward_kernel`
 * (T=, K=, bucket=, semiring=, alpha=, kind=, grid=), `seg_crf_backtrace_kernel`, `seg_crf_backward_kernel` (parts=),
 * `seg_crf_finish_kernel`. */
#define RUA_CRF_MAX_TAGS 64
#define RUA_CRF_LOG 0
#define RUA_CRF_MAX 1
int64_t rua_crf_ws_bytes(const rua_layout* lay, int32_t K, int32_t dtype);   /* backward only */
int rua_segment_crf_forward(const rua_layout* lay, const void* emissions, const void* transitions,
                            const void* start /* NULL */, const void* end /* NULL */, void* alpha /* NULL */,
                            void* backptr, void* out, void* last, int32_t K, int32_t dtype, int32_t semiring,
                            void* stream);
int rua_segment_crf_backtrace(const rua_layout* lay, const void* backptr, const void* last, void* tags, int32_t K,
                              void* stream);
int rua_segment_crf_backward(const rua_layout* lay, const void* grad, const void* emissions, const void* transitions,
                             const void* end /* NULL */, const void* alpha, const void* logz,
                             void* grad_emissions /* NULL */, void* grad_transitions /* NULL */,
                             void* grad_start /* NULL */, void* grad_end /* NULL */, int32_t K, int32_t dtype, void* ws,
                             void* stream);

/* Per-sequence CTC (an EXTENSION, added to ABI 6 — the version number did not move): the loss, its TRUE gradient and the
 * forced alignment (csrc/rua_ctc.hip).  The first entry points that read two ragged containers at once: `frames`
 * describes `log_probs` (rows of V elements of `dtype`, RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16, ANY layout), `targets`
 * describes `labels` (int64, one per row, ANY layout, independently of `frames`); both have the same B and sequence b is
 * the same sequence in both (a PACK layout: through `unsorted`).  0 <= S_max <= RUA_CTC_MAX_TARGET bounds the labels of
 * a sequence (longer ones are cut to it: the caller sizes the launch by the longest target); 0 <= blank < V.  The
 * per-sequence results and the table `alpha` are in the ACCUMULATOR type (float; double for RUA_F64).
 *
 * The extended target is l' = (blank, y_0, blank, ..., y_{S-1}, blank), S' = 2 S + 1 states.  Geometry: the lanes form
 * (2 S_max + 1 <= 512) walks a sequence with ONE wave, lane i keeping the R = 1 / 2 / 4 / 8 consecutive states
 * i R .. i R + R - 1 in registers (2 S_max + 1 <= 64 / 128 / 256 / 512), the boundary values coming from lane i - 1 by a
 * cross-lane move; the workgroup form (up to 2 047 states) walks it with one workgroup, 8 states per thread, the
 * boundary values through LDS with one barrier per frame.  At most 1 024 workgroups; the teams stride over b.  ONE long
 * target sends the whole batch to the workgroup form; one wave / workgroup walks ALL the frames of a sequence.
 *
 * ONE evaluation order per (sequence, frame, state), whatever the layouts, the form or R (no contraction):
 *   v0 = alpha[s], v1 = alpha[s-1] (s >= 1), v2 = alpha[s-2] (s >= 2, l'_s != blank, l'_s != l'_{s-2}); a term that does
 *   not exist is absent.  RUA_CRF_LOG: m = max (a NaN stays one); m == -inf gives -inf; else
 *   alpha_t[s] = lp_t[l'_s] + (m + log(exp(v0 - m) + exp(v1 - m) [+ exp(v2 - m)])).  RUA_CRF_MAX: the maximum in ascending
 *   predecessor state (s-2, s-1, s) under rua_segment_argreduce's order (a NaN beats every number, the first of equals
 *   wins); s minus the predecessor is the code of (row, state); -inf stays -inf.  alpha_0[0] = lp_0[blank],
 *   alpha_0[1] = lp_0[y_0], -inf elsewhere.  The end folds alpha_{T-1}[S'-1], then alpha_{T-1}[S'-2], the same way.
 *
 * rua_segment_ctc_forward: RUA_CRF_LOG writes out[b] = -logZ (0 instead of +inf when zero_infinity != 0), `logz` [B]
 *   (may be NULL) and `alpha` [rows of the frames' storage, 2 S_max + 1] (may be NULL; padding rows and the states
 *   >= S' are not written).  RUA_CRF_MAX writes out[b] = the best path's log-probability, `last` [B] int64 (its final
 *   state; -1: there is no alignment) and `codes` (one uint8 per (row, state); the rows of frame 0 are not written),
 *   both required.  T = 0: 0 for S = 0, else no alignment (logZ = -inf).  A label outside [0, V) is never dereferenced:
 *   out[b] = logz[b] = NaN, last[b] = -1.
 * rua_segment_ctc_backtrace: a thread per sequence walks `codes` from `last` and writes `out_labels` (the class of
 *   every frame) and `out_positions` (the index into the sequence's own target, -1 for a blank frame), int64, one per
 *   row of the frames' storage, zeros in padding rows; a sequence without alignment gets `blank` and -1.
 * rua_segment_ctc_backward (of RUA_CRF_LOG; `grad` [B] the cotangent of out): beta WITHOUT the emission at t,
 *   beta_{T-1}[S'-1] = beta_{T-1}[S'-2] = 0, u_s = lp_{t+1}[l'_s] + beta_{t+1}[s], beta_t[s] = the same logsumexp of u_s,
 *   u_{s+1}, u_{s+2}; grad_log_probs[t, c] = -grad[b] * sum_{s : l'_s = c} exp((alpha_t[s] + beta_t[s]) - logz[b]),
 *   rounded once; every V-wide row is written exactly once, zeros included; padding rows, sequences with
 *   logz == -inf and sequences with a label outside [0, V) get exact zeros.  NO FLOAT ATOMICS; the class sum is, for
 *   c != blank, the states of c in ascending s added from 0; for blank, lane i of 64 adds post[2 k] and then
 *   post[2 k + 1] when y_k == blank over k = i, i + 64, ... from 0 and the 64 parts are folded by the butterfly
 *   xor 32 .. 1.  Bitwise reproducible and identical for every pair of layouts and for both forms.  No workspace.
 *
 * Checks, before any HIP call: a null layout, different B, a dtype outside the four, V < 1, S_max outside
 * [0, RUA_CTC_MAX_TARGET], blank outside [0, V), an unknown semiring (RUA_EINVAL); B == 0 returns 0 without a launch; a
 * missing required pointer (RUA_EINVAL); a table too large for 64-bit offsets (RUA_ERANGE); a pointer not aligned to
 * its element (RUA_EALIGN).  Trace: `seg_ctc_forward_kernel` (T=, V=, S_max=, form=, R=, semiring=, alpha=, kind=,
 * tkind=, grid=), `seg_ctc_backtrace_kernel`, `seg_ctc_backward_kernel`. */
#define RUA_CTC_MAX_TARGET 1023
int rua_segment_ctc_forward(const rua_layout* frames, const rua_layout* targets, const void* log_probs,
                            const void* labels, void* alpha /* NULL */, void* codes, void* out, void* logz /* NULL */,
                            void* last, int32_t V, int32_t S_max, int32_t blank, int32_t dtype, int32_t semiring,
                            int32_t zero_infinity, void* stream);
int rua_segment_ctc_backtrace(const rua_layout* frames, const rua_layout* targets, const void* labels, const void* codes,
                              const void* last, void* out_labels, void* out_positions, int32_t V, int32_t S_max,
                              int32_t blank, void* stream);
int rua_segment_ctc_backward(const rua_layout* frames, const rua_layout* targets, const void* grad,
                             const void* log_probs, const void* labels, const void* alpha, const void* logz,
                             void* grad_log_probs, int32_t V, int32_t S_max, int32_t blank, int32_t dtype, void* stream);

/* Per-sequence edit distance and alignment (an EXTENSION, added to ABI 6 — the version number did not move): the
 * Levenshtein distance of every hypothesis against its reference, and its split into substitutions, insertions and
 * deletions (csrc/rua_edit.hip).  `hyp` describes `hyp_tokens`, `ref` describes `ref_tokens` (both int64,
 * one per row, ANY layout, independently of each other); both have the same B and sequence b is the same sequence in
 * both (a PACK layout: through `unsorted`).  Tokens are compared as 64-bit values: there is no vocabulary.
 * 0 <= S_max <= RUA_EDIT_MAX_REF bounds the tokens of a reference (longer ones are cut to it: the caller sizes the launch
 * by the longest reference); a hypothesis is as long as its storage allows.  The arithmetic is pure integer (int32 in
 * registers: rows of `hyp` + S_max < 2^31, else RUA_ERANGE), every output is int64.
 *
 *   D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (hyp[i-1] != ref[j-1]), D[i-1][j] + 1, D[i][j-1] + 1).
 *
 * Geometry: a TEAM walks one pair, hyp token by hyp token, thread i keeping the R consecutive columns i R + 1 ..
 * i R + R and their ref tokens in registers.  The lanes form (S_max <= 512) is one wave, R = 1 / 2 / 4 / 8 for
 * S_max <= 64 / 128 / 256 / 512, four teams per workgroup; the workgroup form (S_max <= 2 048) is 256 threads with R = 8.
 * At most 1 024 workgroups; the teams stride over b.  The dependence on the left neighbour is a prefix minimum, not a
 * walk: with t[j] = min(Dprev[j-1] + neq, Dprev[j] + 1) and t[0] = i, D[j] = j + min_{k <= j} (t[k] - k) — an R-long
 * chain in registers and ONE prefix-min across the team per row (a shuffle scan; across the four waves of the workgroup
 * form through LDS with one barrier).  The same bits in every bucket and both forms.
 *
 * rua_segment_edit_forward: writes distance[b] = D[T][S].  `codes` NULL: nothing else.  Otherwise one uint8 per cell,
 *   codes[row of hyp token i-1][j-1] for 1 <= j <= S, rows of the hyp storage S_max apart: 0 the diagonal attains
 *   D[i][j] and the tokens are equal, 1 the diagonal attains it and they differ, else 2 up (D[i-1][j] + 1) attains it,
 *   else 3 (left).  Padding rows and the columns >= S are not written.
 * rua_segment_edit_backtrace: a thread per sequence walks `codes` from (T, S) — the diagonal if it attains D[i][j], else
 *   up, else left; at j == 0 only up, at i == 0 only left — and writes `positions` (int64, one per row of the hyp
 *   storage: the index into the sequence's own ref of the token hyp token t is paired with, -1 for an inserted token,
 *   0 in padding rows) and `substitutions`, `insertions`, `deletions` [B] int64.
 *
 * Checks, before any HIP call: a null or malformed layout, different B, S_max outside [0, RUA_EDIT_MAX_REF]
 * (RUA_EINVAL); B == 0 returns 0 without a launch; a missing required pointer (RUA_EINVAL; `codes` and `positions` may
 * be NULL where they have no element); more rows than int32 distances hold (RUA_ERANGE); a pointer not aligned to 8 bytes
 * (RUA_EALIGN).  Trace: `seg_edit_forward_kernel` (S_max=, form=, R=, codes=, kind=, rkind=, grid=),
 * `seg_edit_backtrace_kernel`. */
#define RUA_EDIT_MAX_REF 2048
int rua_segment_edit_forward(const rua_layout* hyp, const rua_layout* ref, const void* hyp_tokens, const void* ref_tokens,
                             void* distance, void* codes /* NULL */, int32_t S_max, void* stream);
int rua_segment_edit_backtrace(const rua_layout* hyp, const rua_layout* ref, const void* codes, void* positions,
                               void* substitutions, void* insertions, void* deletions, int32_t S_max, void* stream);

/* Per-sequence gated linear recurrence (an EXTENSION, added to ABI 6 — the version number did not move: the reference's
 * users pad, loop over the time steps with elementwise kernels and cast back).  For every sequence b of `lay` (ANY
 * layout) and column h, with u the position along the scan (u = t; reverse != 0: u = len - 1 - t):
 *   h_0 = x_0                              (the gate at scan position 0 is NEVER read into the result)
 *   h_u = a_u * h_(u-1) + x_u   for u >= 1
 * so reverse != 0 is the return recursion G_t = r_t + a_t * G_(t+1).  Forward ignores the gate of the first token,
 * reverse the gate of the last one: a NaN or an infinity there reaches no output.  Sequences and columns are
 * independent; a NaN stays in its own sequence and column, at or after the position where it entered.
 * `gate` is a tensor of exactly the payload's storage shape and dtype, or NULL: then `gate_scalar` is the gate of every
 * position, passed by value and held in the accumulator type (no gate tensor is read).  RUA_F32 / RUA_F64 / RUA_BF16 /
 * RUA_F16 — bf16 / f16 accumulate in fp32, gate included (fp64 for RUA_F64), every output element rounded once; any
 * other dtype (integers included): RUA_EINVAL.  B == 0, H == 0 and n_rows == 0 return 0 without a launch.  Padding rows
 * of a LEFT / RIGHT result are written as zeros in the same pass and padding rows of the inputs are never read.  Lengths
 * are clamped to the storage and every row is range-checked.  Argument checks and error codes are those of
 * rua_segment_cumsum.
 * ONE association order: the operator is associative on pairs (A, B); an EARLIER (A1, B1) and a LATER (A2, B2) combine
 * as (A2 * A1, A2 * B1 + B2), never contracted into an fma.  Position u enters as (a_u, x_u), position 0 as (1, x_0).
 * The pairs are combined in rua_segment_cumsum's order, unchanged (groups of 8 by three doubling steps, tiles of 4
 * groups, blocks of 64 tiles whose carry starts afresh, the base of a block from the totals of the blocks before it;
 *   out = B of (((base . carry) . groups before) . prefix inside the group)),
 * for every layout, kernel form, alignment and `ws`.  A term that does not exist is the pair (1, -0.0).  Hence, BIT FOR
 * BIT: the operator commutes with the casts; `reverse` equals reversing every sequence (payload and gate), scanning
 * forward and reversing back; cut == uncut; aligned == unaligned; a gate that is exactly 1 everywhere gives
 * rua_segment_cumsum's result; a scalar gate equals a tensor filled with it.
 * LIMIT: a blocked scan forms partial gate products.  The result is finite only if the product of the gates over any
 * aligned group, tile or block (and over the blocks before a block) is representable in the accumulator type.
 * Kernel forms and the cut rule are those of rua_segment_cumsum (rows of one vector: lanes along time; wider rows: a
 * workgroup per (sequence x 128-byte chunk); fewer than 1 024 units with a length bound of at least 8 192: cut into
 * blocks across workgroups when `ws` is given — two launches, payload and gate read twice).  The workspace holds an
 * (A, B) pair per block and column: rua_linear_scan_ws_bytes == 2 * rua_cumsum_ws_bytes (0 for rows of one vector and
 * for dtypes the scan does not take).  Payload and gate are read once (twice when cut), the result is written once;
 * no slab, no temporaries.
 * Aliasing: `out` may equal `data` (every row is read before it is written, by the same thread); it must not be `gate`
 * (RUA_EINVAL).
 * rua_segment_linear_scan_backward: from the cotangent `grad_out`, the gate and the forward's OUTPUT `h` (the payload is
 * not needed), for the scan whose direction was `reverse`:
 *   grad_x    = the same recurrence run the OTHER way over grad_out, the gate of a position taken from the previous
 *               position of that scan (forward: dx_t = g_t + a_(t+1) * dx_(t+1)) — which drops exactly the gate the
 *               forward ignored;
 *   grad_gate = grad_x * h at the forward's previous position (forward: da_t = dx_t * h_(t-1)), exactly 0 at the
 *               ignored gate; both factors in the accumulator type, rounded once.  grad_gate == NULL: not computed (and
 *               `h` is not read: it may be NULL); with gate == NULL (a scalar gate has no gradient) it MUST be NULL.
 * Padding rows of both gradients are zeros.  `grad_x` may equal `grad_out`; it must not be `gate` or `h`; `grad_gate`
 * must not be anything that is read, nor `grad_x` (RUA_EINVAL).  The shifted gate and `h` are loaded from the
 * neighbouring token's row: lines the neighbouring threads load anyway, no second pass.
 * While the dispatch trace is on (below) every launch records `seg_linear_scan_lanes_kernel` or
 * `seg_linear_scan_rows_kernel` with key=value pairs: T=, AL=, rev= (the direction this launch scans in: the backward
 * of a forward scan records rev=1), kind=, gate=scalar|tensor, bwd=, cut= (and phase=partial|finish for the cut form). */
int64_t rua_linear_scan_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_linear_scan(const rua_layout* lay, const void* data, const void* gate /* NULL: scalar */,
                            double gate_scalar, void* out, int64_t H, int32_t dtype, int32_t reverse, void* ws,
                            void* stream);
int rua_segment_linear_scan_backward(const rua_layout* lay, const void* grad_out, const void* gate /* NULL: scalar */,
                                     double gate_scalar, const void* h, void* grad_x, void* grad_gate /* NULL */,
                                     int64_t H, int32_t dtype, int32_t reverse, void* ws, void* stream);

/* Per-sequence causal depthwise convolution over the tokens of a sequence (an EXTENSION, added to ABI 6 — the version
 * number did not move: the reference has no convolution; its users pad, transpose, call a grouped conv1d, slice,
 * transpose and cast back).  For every sequence b of `lay` (ANY layout), column h and token t < len[b]:
 *   reverse == 0:  out[t] = bias[h] + sum_{k = 0 .. K-1, t - (K-1) + k >= 0}   weight[k,h] * data[t - (K-1) + k]
 *   reverse != 0:  out[t] = bias[h] + sum_{k = 0 .. K-1, t + (K-1) - k < len}  weight[k,h] * data[t + (K-1) - k]
 * `weight` is [K, H], tap-major (weight[K-1] multiplies the current token), `bias` is [H] or NULL, both in the payload
 * dtype.  1 <= K <= RUA_CONV_MAX_TAPS (K < 1: RUA_EINVAL, K > RUA_CONV_MAX_TAPS: RUA_ERANGE).  For finite weights this
 * is a zero-padded grouped conv1d of every sequence on its own; the ONE difference from zero padding: a tap that falls
 * outside the sequence is NOT EVALUATED instead of being multiplied by zero, so a non-finite weight does not poison the
 * first (last) K - 1 tokens.  `reverse` is the anti-causal mirror — the adjoint the backward needs.
 * RUA_F32 / RUA_BF16 / RUA_F16 / RUA_F64 (anything else: RUA_EINVAL).  ONE evaluation order per (token, column),
 * whatever the layout, kernel form, alignment or block boundary: the accumulator (fp32; fp64 for RUA_F64) starts at the
 * bias (+0 without one), the taps that exist are added in ascending k with a fused multiply-add, the result is rounded
 * once.  Hence, BIT FOR BIT: the operator commutes with the casts; `reverse` equals reversing every sequence, convolving
 * forward and reversing back; K == 1 with weight 1 and no bias returns the payload (but for the sign of a zero).
 * Padding rows of a LEFT / RIGHT payload are never read and are written as zeros in the same pass; an empty sequence
 * contributes nothing; B == 0, n_rows == 0 and H == 0 return 0 without a launch.  Lengths are clamped to the storage
 * and every row is range-checked.
 * Kernel forms: rows of one vector (<= 16 bytes) put consecutive tokens on consecutive lanes, two sequences per wave,
 * and take the K - 1 rows before a token from the lanes below by shuffle; wider rows give a workgroup per (sequence x
 * 128-byte column chunk) whose 32 x 8 threads each walk a contiguous run of tokens with the previous K - 1 vectors, the
 * K weight vectors and the bias in registers (the K - 1 rows in front of a run are loaded again); few but long sequences
 * (the cut rule of rua_segment_softmax: fewer than 1 024 units with a length bound of at least 8 192) always spread
 * over workgroups per block of 2 048 tokens — blocks need nothing of each other but those K - 1 rows: no workspace,
 * no second launch.  Every row is read once and written once.
 * Aliasing: `out` may equal `data` (then a sequence stays with one workgroup); it must not be `weight` or `bias`
 * (RUA_EINVAL).
 * rua_segment_causal_conv_backward, for the convolution whose direction was `reverse`; each output may be NULL:
 *   grad_in     = the convolution of grad_out by `weight` the OTHER way, no bias (the forward kernel: `data` is not
 *                 read, no workspace);
 *   grad_weight = [K, H]: sum over every token of grad_out[t] * data[the token tap k read];
 *   grad_bias   = [H]: sum over every token of grad_out[t];
 * all in the payload dtype, the sums accumulated in fp32 (fp64) and rounded once.  ONE walk computes all three: a
 * workgroup keeps the sums of the units it walks in registers, folds them over its threads in a fixed tree and leaves
 * one partial per (part, chunk) in `ws`; a finish launch adds the parts in part order.  No float atomics: grad_weight
 * and grad_bias are bitwise reproducible from run to run for the same container; they are NOT the same bits across
 * layouts (the order over the sequences follows the storage).  The workspace is bounded independently of n_rows:
 *   rua_causal_conv_ws_bytes(lay, H, K, dtype) = parts * n_chunks * (128 / esize) * (K + 1) * sizeof(acc)
 * with n_chunks = ceil(H * esize / 128), sizeof(acc) = 4 (8 for RUA_F64) and parts = min(1 024, units), units = B
 * for rows wider than 16 bytes (B * ceil(bound / 2 048) when the cut rule applies), ceil(ceil(B / 2) / 4) for rows of
 * one vector; 0 for arguments the entry points refuse and when there is nothing to do.  Needed only when grad_weight
 * or grad_bias is wanted (then ws == NULL: RUA_EINVAL).  `data` may be NULL unless grad_weight is wanted, `weight` unless
 * grad_in is.  grad_in must not alias grad_out, data or weight; grad_weight / grad_bias nothing that is read and no
 * other output (RUA_EINVAL).  Padding rows of grad_in are zeros.
 * While the dispatch trace is on (below) every launch records `seg_conv_lanes_kernel` or `seg_conv_rows_kernel` with
 * key=value pairs (T=, K=, AL= / W=, rev= — the direction this launch walks in —, kind=, bwd= — 1 when it sums
 * grad_weight / grad_bias —, cut=, parts=), and `seg_conv_finish_kernel` for the finish. */
#define RUA_CONV_MAX_TAPS 8
int64_t rua_causal_conv_ws_bytes(const rua_layout* lay, int64_t H, int32_t K, int32_t dtype);   /* backward only */
int rua_segment_causal_conv(const rua_layout* lay, const void* data, const void* weight, const void* bias /* NULL */,
                            void* out, int64_t H, int32_t K, int32_t dtype, int32_t reverse, void* stream);
int rua_segment_causal_conv_backward(const rua_layout* lay, const void* grad_out,
                                     const void* data /* NULL unless grad_weight */,
                                     const void* weight /* NULL unless grad_in */, void* grad_in /* NULL */,
                                     void* grad_weight /* NULL */, void* grad_bias /* NULL */, int64_t H, int32_t K,
                                     int32_t dtype, int32_t reverse, void* ws, void* stream);

/* Per-sequence compress — keep the tokens where a mask is set (an EXTENSION, added to ABI 6 — the version number did
 * not move: the reference's users spell it as data[mask], a segment_sum of the mask and a new constructor, for a
 * CattedSequence only).  The first operator whose result has ANOTHER raggedness than its input: sequence b of the result
 * holds the tokens t of sequence b of the input with mask[row(b,t)] != 0, in their order.  Two entry points, because the
 * new lengths size the result and the caller reads them back in between (ONE read-back of [B] int64; nothing here
 * synchronises).
 * rua_segment_compress_plan: `mask` holds one byte per STORAGE ROW of `lay` (ANY layout; n_rows bytes).  Writes
 *   rank[j]     (int32, n_rows entries) = #{s < t : mask[row(b,s)] != 0} for the row j of token (b, t) when its own
 *               byte is set — the position the token takes in its new sequence — and -1 for a dropped token AND for a
 *               padding row of a LEFT / RIGHT storage (whose mask bytes are never read);
 *   new_lens[b] (int64) = the number of kept tokens of sequence b.
 * The mask is read once, four bytes are written per storage row, nothing else per token.  The walk goes sequence by
 * sequence through the layout's own row formula, the same for the four kinds.  Integer work: every form gives the same
 * bits.  Four forms by the length bound (CAT: T_log or n_rows, LEFT / RIGHT: T_phys, PACK: T): up to 64, two sequences
 * per wave, 32 lanes each; below 2 048, a wave per sequence; longer, a workgroup per sequence that walks blocks of
 * 2 048 tokens with a carried count — in all three the count in front of a lane is a popcount over one 64-bit ballot;
 * few but long sequences (fewer than 1 024 of them with a bound of at least 8 192) are cut into their blocks across
 * workgroups when `ws` is given: the first launch leaves every block's count in `ws`, the second adds the counts of
 * the blocks before a block in block order.  rua_compress_ws_bytes(lay) =
 *   B * ceil(bound / 2 048) * 4
 * bytes when the cut form applies, else 0 (0 = never needed; ws == NULL = do not cut).  A CAT layout's T_log, where it
 * is given (> 0), must be a TRUE upper bound of every length, as for rua_segment_softmax.  Lengths are clamped to the
 * storage and every row is range-checked.
 * Checks, before any HIP call: a null or inconsistent layout RUA_EINVAL; a length bound of 2^31 or more RUA_ERANGE (a
 * rank is an int32; rua_compress_ws_bytes returns 0 for both); B == 0 returns 0 without a launch; then a null mask /
 * rank (with n_rows > 0) / new_lens, or outputs that alias, RUA_EINVAL.  Trace: `seg_compress_plan_kernel form=lanes|
 * rows|long|cut G= kind= cut= blocks= phase=whole|count|finish`.
 * rua_segment_compress_move: `big` is the input's layout, `small` the result's (any two kinds, the same B; small's
 * lengths are new_lens, its offsets / PackedSequence metadata the caller's, from rua_exclusive_scan_i64 /
 * rua_pack_prepare as for any container); rows are row_bytes wide on both sides and move as BITS.
 *   expand == 0: every row of big with rank >= 0 is copied to small's row of token (b, rank); padding rows of a LEFT /
 *                RIGHT small are written as zeros in the same launch (no pre-zeroing).  For CAT / PACK results the
 *                payload is read once and written once.
 *   expand != 0: the adjoint.  Every row of big with rank >= 0 reads that row of small; every other row of big —
 *                dropped tokens and padding — is written as zeros: big is written completely.
 * A rank that names no token of its new sequence moves nothing.  Two forms: rows of at most 16 bytes put the tokens of
 * a sequence on 32 lanes, two sequences per wave; wider rows give a workgroup per (sequence x 128-byte column chunk),
 * 32 tokens x 8 pieces of 16 bytes, four tokens in flight per thread; few but long sequences (the cut rule over
 * B * chunks units) spread over workgroups per block of 2 048 tokens — no workspace, no second launch.  Accesses are
 * the widest power of two, up to 16 bytes, that divides row_bytes and both base addresses: any alignment is accepted.
 * Checks: the entry checks of the plan for `big`, then for `small`; different B RUA_EINVAL; B == 0, row_bytes == 0 or a
 * destination without rows return 0; a null rank or payload, or small_data == big_data, RUA_EINVAL.  Trace:
 * `seg_compress_move_lanes_kernel` / `seg_compress_move_rows_kernel` with W= row_bytes= expand= small= big= cut=.
 * (A variant with a caller-given capacity that never reads the lengths back is the natural follow-up; it is not built.) */
int64_t rua_compress_ws_bytes(const rua_layout* lay);
int rua_segment_compress_plan(const rua_layout* lay, const void* mask, int32_t* rank, int64_t* new_lens, void* ws,
                              void* stream);
int rua_segment_compress_move(const rua_layout* small, const rua_layout* big, const int32_t* rank, void* small_data,
                              void* big_data, int64_t row_bytes, int32_t expand, void* stream);

/* Per-sequence unique_consecutive — collapse every run of equal consecutive tokens INSIDE a sequence to its first token
 * and say how long the run was (an EXTENSION, added to ABI 6 — the version number did not move: stock torch offers
 * torch.unique_consecutive per sequence in a Python loop; a global call merges a run across the border of two
 * sequences).  The inverse of rua_segment_repeat_*.  It reuses the compress pair: the caller runs
 *   rua_segment_runs_heads -> rua_segment_compress_plan (rank, new_lens) [-> rua_segment_runs_inverse]
 *   -> ONE read-back of new_lens -> rua_segment_compress_move (the values) [-> rua_segment_runs_counts]
 * and nothing here synchronises.
 * rua_segment_runs_heads: the only kernel that reads the payload.  For the storage row j of every token (b, t) of `lay`
 * (ANY layout) it writes head[j] (one byte per storage row, n_rows bytes) = 1 when t == 0 or the row differs from the
 * row of token (b, t - 1), else 0; padding rows of a LEFT / RIGHT storage are neither read nor written.  The
 * predecessor's row comes from the layout's own row formula, so a sequence's first token is compared with nothing.  `eq`
 * is the equality rule: RUA_F32 / RUA_BF16 / RUA_F16 / RUA_F64 compare element by element as IEEE does (a NaN differs
 * from everything, itself included; -0.0 equals +0.0; row_bytes must be a multiple of the element size), RUA_RUNS_BITS
 * compares bits.  Rows are row_bytes wide.  Two compares: rows of at most 16 bytes take one vector load of the row and
 * one of its predecessor, a lane per token, in the geometry of the offsets scan (form=lanes|rows|long|cut by the length
 * bound, as rua_segment_compress_plan; no workspace: a block needs nothing from the blocks before it); wider rows give
 * a workgroup per sequence (form=long) or per block of 2 048 tokens of one (form=cut, the same rule), 32 tokens x 8
 * lanes, every lane a 16-byte piece of each 128-byte chunk, combined by ballot, stopping at the first chunk that
 * differs.  Accesses are the widest power of two, up to 16 bytes, that divides row_bytes and the base address.  The
 * payload is read at most twice — a row, and the same row as its successor's predecessor — and no [N, H] temporary
 * exists.  Checks, before any HIP call: a null or inconsistent layout or row_bytes < 0 RUA_EINVAL; a length bound of
 * 2^31 or more RUA_ERANGE; an `eq` that is neither, or a float rule with a row that is no multiple of its element,
 * RUA_EINVAL; B == 0 or n_rows == 0 returns 0; a null head, a null payload (row_bytes > 0) or head == data RUA_EINVAL.
 * Trace: `seg_runs_heads_lanes_kernel` / `seg_runs_heads_rows_kernel form= G= kind= cut= blocks= phase=whole W=
 * row_bytes=`.
 * rua_segment_runs_inverse: inverse[j] (int64, n_rows entries) = #{s <= t : head[row(b, s)] != 0} - 1 for the row j of
 * token (b, t) — the index of the token's run inside its sequence — and 0 for a padding row; new_lens[b] = the number of
 * heads (what rua_segment_compress_plan writes too; B entries).  The offsets scan of rua_segment_compress_plan over the
 * same mask: its four forms, its workspace rule (rua_compress_ws_bytes; ws == NULL = do not cut) and its checks, in its
 * order; a pointer that is not aligned to its element RUA_EALIGN.  Trace: `seg_runs_inverse_kernel form=lanes|rows|
 * long|cut G= kind= cut= blocks= phase=whole|count|finish`.
 * rua_segment_runs_counts: `big` is the input's layout, `small` the result's (any two kinds, the same B), `rank` the
 * plan's table.  counts[row_small(b, r)] (int64, small's n_rows entries) = start(b, r + 1) - start(b, r), where
 * start(b, r) is the position of the head of rank r in sequence b of big and start(b, R_b) = the length of that
 * sequence; padding rows of a LEFT / RIGHT small are zeros.  Two launches and no atomics (a long run costs what a short
 * one does): the heads of big leave their positions in `starts` (int32, small's n_rows entries, laid out like counts;
 * caller-given scratch), then every run reads its own and its successor's.  Both walk in the geometry of the offsets
 * scan, the first over big, the second over small.  Checks: the entry checks of the plan for `big`, then for `small`;
 * different B RUA_EINVAL; B == 0 or a small without rows returns 0; a null pointer or two that alias RUA_EINVAL; a
 * misaligned one RUA_EALIGN.  Trace: `seg_runs_counts_kernel form= G= kind= cut= blocks= phase=starts|diff`. */
#define RUA_RUNS_BITS 0x100   /* `eq` of rua_segment_runs_heads: rows are equal when their bits are */
int rua_segment_runs_heads(const rua_layout* lay, const void* data, int64_t row_bytes, int32_t eq, void* head,
                           void* stream);
int rua_segment_runs_inverse(const rua_layout* lay, const void* head, int64_t* inverse, int64_t* new_lens, void* ws,
                             void* stream);
int rua_segment_runs_counts(const rua_layout* small, const rua_layout* big, const int32_t* rank, int32_t* starts,
                            int64_t* counts, void* stream);

/* Per-sequence sliding-window pooling — max / mean / sum over windows of K tokens every S tokens along time (an
 * EXTENSION, added to ABI 6 — the version number did not move: the reference's users pad with left(), transpose, call
 * F.max_pool1d / F.avg_pool1d, compute the new lengths by hand and cast back; windows at a sequence's end then read the
 * padding).  The first operator whose new raggedness is a CLOSED FORM of the old one.  For a sequence of n tokens
 * (clamped to its storage), 1 <= K <= RUA_WINDOW_MAX_K, 1 <= S <= 2^31 - 1:
 *   n <= 0:            n_out = 0
 *   ceil_mode == 0:    n_out = (n - K) / S + 1 if n >= K, else 0
 *   ceil_mode != 0:    m = ceil(max(n - K, 0) / S) + 1;  n_out = m - 1 if (m - 1) * S >= n, else m
 * (ceil mode: a sequence shorter than K gives ONE clipped window).  Window u covers the tokens [u S, min(u S + K, n)):
 * never empty, clipped at the end of the sequence, never reaching into padding or the next sequence.  S > K skips
 * tokens; K == 1 is the strided subsample.  Where torch accepts the input, n_out and the values are those of
 * F.max_pool1d(ceil_mode) / F.avg_pool1d(ceil_mode, count_include_pad=False).
 * rua_window_lens: out_lens[b] = n_out of sequence b ([B] int64, one thread per sequence, one launch); own_lens, if
 *   given ([B]), receives the length as `lay` GIVES it (lens[b] + len_add, unclamped) — what a caller that has to read
 *   the new lengths back reads back with them.  A RIGHT `lay` whose T_log the caller does not know yet may be described
 *   with T_log = T_phys here: only the clamp reads it.
 * rua_segment_window_pool: `src_lay` describes `data`, `dst_lay` `out` (any two kinds, the same B; dst's lengths are
 *   rua_window_lens's, or any others: a window past its sequence's end is written as zeros).  DESTINATION-driven: window
 *   (b, u) reads its at most K rows through src's own row formula and writes ONE row; padding rows of src are never
 *   read, padding rows of a LEFT / RIGHT dst are zeros written in the same launch.  Per column, `mode`:
 *     RUA_SUM   the accumulator (fp32; fp64 for RUA_F64; int64, wrapping, for RUA_I64) starts at the window's first
 *               token and adds the others in ascending position; one rounding.
 *     RUA_MEAN  that sum, divided ONCE in the accumulator type by the number of tokens IN the window (never by K where
 *               the window is clipped); one rounding.  RUA_I64: RUA_EINVAL.
 *     RUA_MAX   argmax's total order on (value, position): a NaN beats every number, the first NaN or the first maximal
 *               position wins, -0.0 == +0.0.  out holds the winner's BITS.  `arg` (may be NULL; uint8, shaped like out)
 *               receives the winner's offset inside its window, 0 .. K - 1.
 *     RUA_WINDOW_TAKE  reads `arg`: out[u] = data[u S + arg[u]] per column (zeros where that offset is outside the
 *               window) — RUA_MAX as the linear map it is once arg is known.
 *   ONE evaluation order per (window, column) whatever the layouts, the kernel form, the alignment or a block border: the
 *   operator commutes with the casts bit for bit.
 * rua_segment_window_spread: the adjoint.  `pooled_lay` describes grad_out (and arg), `big_lay` grad_in.  SOURCE-driven,
 *   no atomics: token (b, t) of big adds, in ascending u, the windows u in [ceil((t - K + 1) / S), floor(t / S)] that
 *   exist — g[u] (RUA_SUM), g[u] / cnt[u] with cnt the tokens in window u, divided first and then added (RUA_MEAN), g[u]
 *   where arg[u] == t - u S (RUA_MAX and RUA_WINDOW_TAKE alike) — into an accumulator of the types above that starts at
 *   +0; one rounding.  Tokens in no window (the gaps of S > K, a dropped tail) and the padding rows of a LEFT / RIGHT big
 *   get exact zeros whatever grad_out holds; every row of grad_in is written.  Bit-identical across layouts too.
 * Forms (those of rua_segment_causal_conv): rows of at most 16 bytes put consecutive windows (the spread: tokens) of a
 * sequence on consecutive lanes, 32 per sequence, two sequences per wave (`form=lanes`); wider rows give a workgroup per
 * (sequence x 128-byte column chunk), 16 bytes per thread (`form=rows`; `form=unaligned`: rows or bases off 16 bytes,
 * elementwise accesses).  Few but long sequences (the family's cut rule over the BIG layout: fewer than 1 024
 * sequence x chunk units with a bound of at least 8 192 tokens) are cut across workgroups, no workspace and no second
 * launch: block i of the spread takes the tokens [2 048 i, 2 048 (i + 1)), block i of the pool the windows that BEGIN
 * there.  A CAT big layout's T_log, where given (> 0), must be a TRUE bound, as for rua_segment_softmax.  Any H, any
 * alignment of an element; lengths are clamped to the storages and every row is range-checked.
 * Checks, before any HIP call: a null or inconsistent layout, H < 0, a dtype other than the four float types and
 * RUA_I64, layouts of different B, a mode other than the four, RUA_I64 with RUA_MEAN, K < 1 or S < 1: RUA_EINVAL;
 * K > RUA_WINDOW_MAX_K: RUA_ERANGE; then B == 0, a written side without rows or H == 0 returns 0 without a launch; then
 * a null output, a null input where its layout has rows, a null arg where the mode reads it, out == data (grad_in ==
 * grad_out), arg equal to either: RUA_EINVAL; a pointer that is not aligned to its element: RUA_EALIGN.  Trace:
 * `seg_window_lens_kernel K= S= ceil= kind= B=` and `seg_window_pool_kernel` / `seg_window_spread_kernel form=lanes|rows|
 * unaligned T= K= S= mode=sum|mean|max|take kind=<written> from=<read> cut= blocks=` (+ `W= H=` / `AL= chunks=`). */
#define RUA_WINDOW_MAX_K 64
#define RUA_WINDOW_TAKE 6   /* the fourth `mode`, next to RUA_SUM, RUA_MEAN and RUA_MAX of enum rua_op */
int rua_window_lens(const rua_layout* lay, int32_t K, int32_t S, int32_t ceil_mode, int64_t* out_lens, int64_t* own_lens,
                    void* stream);
int rua_segment_window_pool(const rua_layout* src_lay, const rua_layout* dst_lay, const void* data, void* out,
                            uint8_t* arg, int64_t H, int32_t K, int32_t S, int32_t mode, int32_t dtype, void* stream);
int rua_segment_window_spread(const rua_layout* pooled_lay, const rua_layout* big_lay, const void* grad_out,
                              const uint8_t* arg, void* grad_in, int64_t H, int32_t K, int32_t S, int32_t mode,
                              int32_t dtype, void* stream);

/* Per-sequence join and unjoin — concatenate ragged batches along time, and cut one at per-sequence boundaries (an
 * EXTENSION, added to ABI 6 — the version number did not move: the reference's users loop over B pairs with torch.cat,
 * or gather through an index built with repeat_interleave, and call a constructor again; for a CattedSequence only).
 * n_parts (1 .. RUA_JOIN_MAX_PARTS) parts with the same B: sequence b of the JOINED side is sequence b of part 0, then
 * of part 1, ... in order.  With len_k[b] the length of part k clamped to its storage and pre_k[b] = sum_{i<k} len_i[b]:
 *   token (b, u) of the joined side  <->  token (b, u - pre_k[b]) of part k,   pre_k[b] <= u < pre_(k+1)[b]
 * — a closed form per token: there is no per-token table of any kind (no rank, no index, no workspace).  `part_lays` is
 * an ARRAY of n_parts layouts of ANY kinds.  One token per sequence (a [B, *hidden] tensor: a BOS embedding, a
 * conditioning vector) is the LEFT layout with T_phys = 1, lens = NULL, len_add = 1.  Nothing here synchronises.
 * rua_segment_join_lens: out_lens[b] = sum_k len_k[b] ([B] int64, one thread per sequence, one launch); part_lens, if
 *   given ([n_parts, B]), receives the length of every part as its layout GIVES it (lens[b] + len_add, unclamped) —
 *   what a caller that has to read the sums back reads back with them.  A RIGHT part whose T_log the caller does not
 *   know yet may be described with T_log = T_phys here: only the clamp reads it.
 * rua_segment_unjoin_lens: the lengths of the parts an unjoin of `joined` cuts.  wanted_k[b] = (sizes[k] ? sizes[k][b] :
 *   0) + size_add[k] (`sizes` and `size_add` are HOST arrays of n_parts entries; sizes[k] a device [B] int64 or NULL),
 *   out_lens[k * B + b] = min(max(wanted_k[b], 0), len[b] - pre_k[b]): a part that would run past the end of its
 *   sequence is clamped to it, tokens beyond the last part are dropped.  own_lens, if given ([B]), receives the length
 *   of every sequence as `joined` GIVES it (unclamped): what a caller that has to read the parts' lengths back reads
 *   back with them; a RIGHT `joined` whose T_log the caller does not know yet may be described with T_log = T_phys here.
 * rua_segment_join: rows are row_bytes wide on every side and move as BITS.
 *   unjoin == 0: every storage row of `joined` is written exactly once — its tokens from their parts (a token no part
 *                holds: zeros), the padding rows of a LEFT / RIGHT `joined` as zeros in the same launch (no pre-zeroing).
 *                A CAT `joined` whose storage holds more rows than its lengths add up to (a caller that sizes it by
 *                the parts' storages without reading the lengths back) gets the spare rows behind its last sequence
 *                as zeros too.  Padding rows of the parts are never read.  Every payload byte is read once and
 *                written once.
 *   unjoin != 0: the adjoint, and the inverse.  Token (b, t) of part k reads token (b, pre_k[b] + t) of `joined` (zeros
 *                if `joined` does not hold it); every part's LEFT / RIGHT padding rows are written as zeros: every
 *                part is written completely, in ONE launch for all parts.  Tokens of `joined` beyond the parts are not
 *                read.  The parts' lengths are those of their layouts (rua_segment_unjoin_lens's, or any others).
 * ONE kernel, walked by the sequences of `joined`; a thread group owns WHOLE rows, 16 bytes per thread and step, four
 * rows in flight, so the lengths, the (at most 8) prefixes and both row formulas are paid once per row.  Three forms:
 * rows of at most 16 bytes put the tokens of a sequence on 32 lanes, two sequences per wave (`lanes`); wider rows whose
 * longest joined sequence (the bound: CAT T_log or n_rows, LEFT / RIGHT T_phys, PACK T) times row_bytes is at most
 * 16 KiB give a wave per sequence (`wave`); anything longer a workgroup per sequence (`rows`).  Few but long sequences
 * (fewer than 1 024 with a bound of at least 8 192; narrow rows too) are cut into blocks of 2 048 tokens across
 * workgroups: blocks need nothing of each other, so no workspace and no second launch.  A CAT `joined` layout's T_log,
 * where given (> 0), must be a TRUE bound, as for rua_segment_softmax.  Accesses are the widest power of two, up to 16
 * bytes, that divides row_bytes and every base address: any alignment is accepted.  Lengths are clamped to the storage
 * and every row is range-checked.
 * Checks, before any HIP call: a null or inconsistent layout, n_parts outside 1 .. 8, a null `part_lays` (`sizes`,
 * `size_add`), a part of another B: RUA_EINVAL; B == 0 (and, for the move, row_bytes == 0 or a destination without
 * rows) returns 0 without a launch; then a null output or a null payload where its layout has rows, the joined payload
 * equal to a part's, two parts of an unjoin in one place, out_lens equal to part_lens / own_lens or either equal to a
 * sizes[k]: RUA_EINVAL; a length vector that is not 8-byte aligned RUA_EALIGN.  The alias checks compare BASE POINTERS
 * only, like the family's: buffers that overlap at another offset are the caller's to avoid (torchrua_amd always
 * allocates its outputs afresh).  Sums and parts agree where the layouts are well formed — lengths within their
 * storages; out_lens sums the CLAMPED lengths, part_lens / own_lens hold the lengths as given.  Trace: `seg_join_lens_kernel` / `seg_unjoin_lens_kernel` with
 * parts= B=, and `seg_join_kernel form=lanes|wave|rows W= row_bytes= parts= unjoin= joined=<kind> G= cut= blocks=`. */
#define RUA_JOIN_MAX_PARTS 8
int rua_segment_join_lens(const rua_layout* part_lays, int32_t n_parts, int64_t* out_lens, int64_t* part_lens,
                          void* stream);
int rua_segment_unjoin_lens(const rua_layout* joined, const int64_t* const* sizes, const int64_t* size_add,
                            int32_t n_parts, int64_t* out_lens, int64_t* own_lens, void* stream);
int rua_segment_join(const rua_layout* joined, const rua_layout* part_lays, int32_t n_parts, void* joined_data,
                     void* const* part_data, int64_t row_bytes, int32_t unjoin, void* stream);

/* Per-sequence repeat_interleave — every token counts[b, t] times inside its own sequence (an EXTENSION, added to ABI 6
 * — the version number did not move: the reference's users spell it as torch.repeat_interleave(data, counts, dim=0), a
 * segment_sum of the counts and a new constructor, for a CattedSequence only, or as a gather through an int64 index).
 * The inverse direction of compress: the result's raggedness GROWS from the data.  Sequence b of the result is
 * repeat_interleave(sequence b of the input, its counts); a count may be 0.  Three entry points; the caller reads the
 * new lengths back between the first two (ONE read-back of [B + 1] int64; nothing here synchronises).
 * rua_segment_repeat_plan (replaces segment_sum(counts) and the cumsum of torch.repeat_interleave): `counts` and `first`
 * hold one int64 per STORAGE ROW of `lay` (ANY layout; n_rows entries).  A count below 0 or above 2^31 - 1 is INVALID: it
 * is counted and taken as 0.  Writes
 *   first[j]        = the sum of the valid counts of the tokens s < t of sequence b, for the row j of token (b, t): the
 *                     position of the token's first copy in its new sequence; -1 for a padding row of a LEFT / RIGHT
 *                     storage (whose counts are never read);
 *   new_lens[b]     = the sum of the valid counts of sequence b (b < B);
 *   new_lens[B]     = the number of invalid counts (the entry point zeroes the word on the stream, lanes that met one
 *                     add to it with a vector atomic): new_lens has B + 1 entries, so the one read-back carries it.
 * Integer work: every form gives the same bits.  Four forms by the length bound (CAT: T_log or n_rows, LEFT / RIGHT:
 * T_phys, PACK: T), as for rua_segment_compress_plan: up to 64, two sequences per wave, 32 lanes each; below 2 048, a
 * wave per sequence; longer, a workgroup per sequence with the sum carried from step to step — in all three the sum in
 * front of a lane is a shuffle scan; few but long sequences (fewer than 1 024 of them with a bound of at least 8 192)
 * are cut into blocks of 2 048 tokens across workgroups when `ws` is given: the first launch leaves every block's sum
 * in `ws`, the second adds the sums of the blocks before a block in block order.  rua_repeat_ws_bytes(lay) =
 *   B * ceil(bound / 2 048) * 8
 * bytes when the cut form applies, else 0 (0 = never needed; ws == NULL = do not cut).  Lengths are clamped to the
 * storage and every row is range-checked.
 * Checks, before any HIP call: a null or inconsistent layout RUA_EINVAL (rua_repeat_ws_bytes: 0); B == 0 returns 0
 * without a launch; then a null counts / first (with n_rows > 0) / new_lens, or outputs that alias each other or the
 * counts, RUA_EINVAL; a pointer that is not 8-byte aligned RUA_EALIGN.  Trace: `seg_repeat_plan_kernel form=lanes|rows|
 * long|cut G= kind= cut= blocks= phase=whole|sum|finish`.
 * rua_segment_repeat_move (replaces torch.repeat_interleave(data, counts, dim=0) / the gather): DESTINATION-driven.
 * `src` is the input's layout, `dst` the result's (any two kinds, the same B; dst's lengths are new_lens, its offsets /
 * PackedSequence metadata the caller's); rows are row_bytes wide on both sides and move as BITS.  The row of every token
 * (b, u) of dst receives the row of source token t:
 *   first != NULL: the largest t < len_src[b] with first[row_src(b, t)] <= u.  `first` is non-decreasing over t and tokens
 *                  that share a value all have count 0 except the last of them, so that t is the token whose run
 *                  [first, first + count) holds u — with zero counts anywhere, leading and trailing included;
 *   first == NULL: t = u / uniform (every token `uniform` times; uniform == 0: dst holds no token).
 * A token of dst that no source token answers for (layouts that do not belong together) is written as zeros; padding
 * rows of a LEFT / RIGHT dst are written as zeros in the same launch (no pre-zeroing).  One kernel: a workgroup per
 * (sequence of dst, 128-byte column chunk) walks the sequence in blocks of 2 048 destination tokens; few but long
 * destination sequences (the cut rule over B * chunks units of dst) spread their blocks over workgroups — no workspace,
 * no second launch.  Per block the source tokens it covers are found ONCE (two searches of the sequence's `first`
 * entries — strided rows for a PACK src), their entries are staged in LDS as offsets from the block's start (up to
 * 2 048 of them; a block that covers more — long stretches of zero counts — searches the table itself) and every
 * destination token searches there.  32 tokens x 8 pieces of 16 bytes per step for rows wider than 16 bytes (`form=
 * rows`), a token per thread for rows of one vector (`form=lanes`); four tokens in flight per thread.  The copies of
 * a long run are different destination tokens, so they spread over the threads of the workgroup that owns their block
 * (256 at most) and, when the destination is cut, over the workgroups of its blocks; WITHOUT the cut — the ordinary batch
 * of 1 024 or more (sequence x chunk) units — one workgroup per chunk walks a whole destination sequence block after
 * block, a count of 100 000 among short sequences included: correct, and slow (the skew limit of DESIGN 3.2j).
 * Accesses are the widest power of two, up to 16 bytes, that divides row_bytes and both base addresses: any alignment is
 * accepted.  Every row index is range-checked on both sides.
 * Checks: the layout checks for `src`, then for `dst`; different B, or first == NULL with uniform < 0, RUA_EINVAL; B == 0,
 * row_bytes == 0 or a destination without rows return 0; a null payload, or dst_data == src_data, RUA_EINVAL.  Trace:
 * `seg_repeat_move_kernel form=rows|lanes W= row_bytes= table= dst= src= cut= blocks= chunks=`.
 * rua_segment_repeat_sum (replaces the index_add / segment_sum of the stock backward): the adjoint, SOURCE-driven.
 *   grad_src[row_src(b, t)] = sum over u in [first, first + count) of grad_dst[row_dst(b, u)]
 * (first == NULL: first = t * uniform, count = uniform; an invalid count is 0, a run is clamped to dst's length).  The
 * sum runs in ascending u in fp32 (fp64 for RUA_F64) and is rounded once: ONE fold order per (token, column) whatever
 * the two layouts are, so it commutes with the casts bit for bit and is the same from run to run.  dtype is RUA_F32 /
 * RUA_F64 / RUA_BF16 / RUA_F16 (anything else: RUA_EINVAL).  A token with count 0 and every padding row of a LEFT / RIGHT
 * src receive exact zeros whatever grad_dst holds around them.  No float atomics, no workspace.  A workgroup per
 * (sequence of src, 128-byte column chunk[, block of 2 048 source tokens: the cut rule over src]); a run is walked by
 * ONE thread group (the eight threads of its row chunk): correct for any count, SLOW for a very long one — a count of
 * 100 000 is 100 000 dependent steps of one group.  Splitting runs is not built.  16-byte accesses where H * esize and
 * both bases allow (`vec=1`), else element by element.  Checks as for the move, plus: a table without counts, or
 * grad_src equal to grad_dst / first / counts, RUA_EINVAL.  Trace: `seg_repeat_sum_kernel form= dtype= H= vec= table=
 * src= dst= cut= blocks= chunks=`.
 * (A variant with a caller-given capacity that never reads the lengths back is the follow-up compress names too.) */
int64_t rua_repeat_ws_bytes(const rua_layout* lay);
int rua_segment_repeat_plan(const rua_layout* lay, const int64_t* counts, int64_t* first, int64_t* new_lens /* B + 1 */,
                            void* ws, void* stream);
int rua_segment_repeat_move(const rua_layout* dst, const rua_layout* src, const int64_t* first /* NULL: uniform */,
                            int64_t uniform, void* dst_data, const void* src_data, int64_t row_bytes, void* stream);
int rua_segment_repeat_sum(const rua_layout* src, const rua_layout* dst, const int64_t* first /* NULL: uniform */,
                           const int64_t* counts, int64_t uniform, void* grad_src, const void* grad_dst, int64_t H,
                           int32_t dtype, void* stream);

/* Per-sequence STABLE sort / argsort, and the per-sequence permutation that goes with it (an EXTENSION, added to ABI 6
 * — the version number did not move: the reference cannot put the tokens of a sequence in order; its users pad with
 * +inf and call torch.sort along dim 1, which is wrong when the payload holds inf or NaN, or run two global stable
 * sorts).  For every sequence b of `lay` (ANY layout) and column h, over t < len[b]:
 *   indices[row(b,t), h] = the token position — NOT a storage row: the same number in every layout — of the element
 *                          of rank t; int64, in the storage layout of `data`
 *   values[row(b,t), h]  = data[row(b, indices[row(b,t), h]), h], the input's BITS (values == NULL: argsort, nothing but
 *                          the indices is written)
 * under ONE total order on (key, position): a NaN is greater than every number (ascending: NaNs last; descending: first),
 * -0.0 == +0.0, and equal keys — all NaNs among themselves too — keep ascending position in BOTH directions:
 * torch.sort(seq, dim=0, stable=True, descending=d) of every sequence on its own.  RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16
 * and RUA_I64; any other dtype: RUA_EINVAL.  Because the order is total, the bits depend on nothing but the sequence —
 * not on the layout, the kernel form or the alignment.  Padding rows of a LEFT / RIGHT input are never read and are
 * zeros in both outputs; an empty sequence contributes nothing; lengths are clamped to the storage and every row is
 * range-checked.
 * An element is (key image, position), sorted ascending as a whole: the image is the value's bits with the sign
 * flipped (negative floats inverted), every NaN the all-ones maximum, -0 taken as +0, int64 biased by 2^63; `descending`
 * inverts the image.  2- and 4-byte values pack image and position into one 64-bit word, 8-byte values keep 64 + 32 bits.
 * Three forms by the length bound (CAT: T_log or n_rows, LEFT / RIGHT: T_phys, PACK: T):
 *   lanes   bound <= 64: a (sequence, column) on G = 8 / 16 / 32 / 64 lanes (the power of two that holds the bound),
 *           64 / G of them per wave, a bitonic network of cross-lane exchanges — no LDS;
 *   block   bound <= 2 048 (rua_sort_block_len()): a workgroup per (sequence, column), a bitonic network over an LDS slab
 *           of the next power of two above the length (16 KiB, 24 KiB for 8-byte values);
 *   merge   longer: the block kernel sorts every block of 2 048 tokens — CAT: B + ceil(n_rows / 2 048) units per column,
 *           so a long sequence among short ones costs what its rows cost; other layouts B * ceil(bound / 2 048) — and
 *           leaves the runs of sequences longer than a block in the workspace; then ceil(log2(ceil(bound / 2 048)))
 *           launches of a rank merge over a FLAT grid, a thread per storage element: an element of a left run goes to
 *           its offset plus the lower bound of its key in the right run, one of a right run to its offset plus the
 *           upper bound in the left run; the last pass of every sequence writes `values` / `indices` themselves.  The
 *           first workspace word holds the passes any sequence needs: a launch beyond it returns at once.
 * A CAT layout's T_log, where given (> 0), must be a TRUE upper bound of every length.  A bound of 2^31 or more is
 * refused (RUA_ERANGE): positions are 31 bits.  rua_sort_ws_bytes(lay, H, dtype) =
 *   256 + 2 * pad256(n_rows * H * 8) + (8-byte values: 2 * pad256(n_rows * H * 4))     pad256 = up to a multiple of 256
 * bytes when bound > 2 048, else 0.  `ws` must be 256-byte aligned; merge form without it: RUA_EINVAL.
 * Checks, before any HIP call: a null or inconsistent layout, H < 0 or an unknown dtype RUA_EINVAL (ws_bytes: 0); the
 * bound RUA_ERANGE; B == 0, H == 0 or n_rows == 0 return 0; a null data / indices, or outputs that alias the input or
 * each other, RUA_EINVAL; a misaligned pointer RUA_EALIGN.  Trace: `seg_sort_lanes_kernel | seg_sort_block_kernel dtype=
 * H= G= kind= values= desc= passes=`, `seg_sort_merge_kernel pass= of= run=`.
 * rua_segment_reorder: the per-sequence permutation; elements move as BITS (elem_bytes 1 / 2 / 4 / 8, else RUA_EINVAL).
 *   per_row != 0: index [n_rows] int64, rows of H elements:    out[row(b,t)] = data[row(b, index[row(b,t)])]
 *   per_row == 0: index [n_rows, H] int64:                     out[row(b,t), h] = data[row(b, index[row(b,t), h]), h]
 *   inverse != 0: the scatter,                                 out[row(b, index[row(b,t)])] = data[row(b,t)]
 * A position outside [0, len[b]) is never dereferenced: the gather writes zeros there, the scatter drops the element;
 * padding rows are never read and are zeros in `out`.  The gather writes `out` completely in one launch; the scatter
 * zeroes `out` on the stream first.  `index` must hold a permutation per sequence for the scatter to be defined
 * (a repeated position: one of the writers wins).  Per row a thread group owns a row (one lane for rows of one
 * vector, eight lanes of 16 bytes otherwise) with the widest access that divides the row and both bases; per element
 * a thread per element.  Checks as above.  Trace: `seg_reorder_rows_kernel form= W= row_bytes= kind= inverse=`,
 * `seg_reorder_elems_kernel elem_bytes= H= kind= inverse=`. */
int64_t rua_sort_block_len(void);
int64_t rua_sort_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_sort(const rua_layout* lay, const void* data, void* values /* NULL: argsort */, int64_t* indices,
                     int64_t H, int32_t dtype, int32_t descending, void* ws, void* stream);
int rua_segment_reorder(const rua_layout* lay, const void* data, const int64_t* index, void* out, int64_t H,
                        int32_t elem_bytes, int32_t per_row, int32_t inverse, void* stream);

/* Per-sequence argmax / argmin with the selected values (an EXTENSION, added to ABI 6 — the version number did not
 * move: the reference has no position-returning reduction; its users pad with -inf and call torch.argmax along dim 1).
 * For every sequence b of `lay` (ANY layout) and column h, over t < len[b] (op = RUA_MAX or RUA_MIN, anything else:
 * RUA_EINVAL):
 *   index[b,h]  = the token position t — NOT a storage row: the same number in every layout — of the largest
 *                 (smallest) data[row(b,t), h]; [B, H] int64 in batch order (PACK: original order, not sorted order)
 *   values[b,h] = data[row(b, index[b,h]), h], in the payload dtype (values == NULL: positions only)
 * under ONE total order on (value, position): a NaN beats every number, for max AND for min; otherwise the greater
 * (smaller) value wins, +0.0 == -0.0; between equals (two NaNs included) the smaller position wins.  That is
 * torch.max(seq, dim=0) / torch.min(seq, dim=0) of every sequence on its own (CPU torch).  An EMPTY sequence gives
 * index -1 and the identity as its value: -inf (max) / +inf (min) in the float types, INT64_MIN / INT64_MAX for RUA_I64
 * — no global `initial`, no `extreme` scratch, no rua_fill_empty: both outputs are written completely in the one pass
 * (also when n_rows == 0; B == 0 and H == 0 return 0 without a launch).  RUA_F32 / RUA_F64 / RUA_BF16 / RUA_F16 (the 16-bit
 * types compare after the exact widening to fp32) and RUA_I64; any other dtype: RUA_EINVAL.  The result is exact, and
 * because the order is total the fold is associative and commutative: the bits depend on NOTHING but the sequence —
 * not on the layout, the kernel form, the alignment or `ws`.  Padding rows of a LEFT / RIGHT input are never read;
 * lengths are clamped to the storage and every row is range-checked.
 * Three kernel forms, chosen as rua_segment_softmax chooses its own: rows of one vector (<= 16 bytes) put consecutive
 * tokens on consecutive lanes, two sequences per wave, eight tokens in flight per lane; wider rows give a workgroup per
 * (sequence x 128-byte column chunk), 32 rows x 4 in flight, combined by shuffles and through LDS; few but long sequences
 * (fewer than 1 024 units whose length bound — CAT: T_log or n_rows, LEFT / RIGHT: T_phys, PACK: T — is at least 8 192)
 * are cut into blocks of 2 048 tokens across workgroups when `ws` is given: every block leaves its (value, position) per
 * column in `ws` and a finish launch combines them (two launches; the payload is still read once).
 * rua_argreduce_ws_bytes(lay, H, dtype) =
 *   B * ceil(bound / 2 048) * ceil(H * esize / 128) * (128 / esize) * (8 + (4, or 8 for RUA_F64 / RUA_I64))
 * bytes when the cut form applies, else 0 (0 = never needed; ws == NULL = do not cut).  A CAT layout's T_log, where it
 * is given (> 0), must be a TRUE upper bound of every length, as for rua_segment_softmax.
 * `data` is only read; `values` / `index` must not overlap it.  Any alignment of `data` is accepted (narrower
 * accesses).  While the dispatch trace is on (below) every launch records `seg_argreduce_lanes_kernel` or
 * `seg_argreduce_rows_kernel` (cut=1 phase=partial|finish for the cut form) with key=value pairs (T=, op=, AL=,
 * values=, kind=). */
int64_t rua_argreduce_ws_bytes(const rua_layout* lay, int64_t H, int32_t dtype);
int rua_segment_argreduce(const rua_layout* lay, const void* data, void* values /* NULL: indices only */,
                          int64_t* index, int64_t H, int32_t dtype, int32_t op /* RUA_MAX | RUA_MIN */,
                          void* ws, void* stream);
/* The two row operators the autograd of the selected values is made of; each is the adjoint of the other (put is the
 * backward of the values, take the backward of put, and so on: derivatives of any order).  `index` is a [B, H] int64
 * tensor of token positions as rua_segment_argreduce writes it; elements move as bits, so both take the dtypes above
 * (by element size) and are exact.
 *   take:  out[b,h] = data[row(b, index[b,h]), h];  0 where index[b,h] < 0 or >= len[b].  [B, H], one thread per
 *          element, written completely.  Trace: `seg_take_kernel`.
 *   put:   out[row(b,t), h] = (t == index[b,h]) ? src[b,h] : 0 for EVERY token; padding rows of a LEFT / RIGHT `out`
 *          are zeros: the whole payload is written once, with 16-byte stores where rows and base allow, and needs no
 *          pre-zeroing.  A position that names no token of its sequence puts nothing.  The thread that owns a 16-byte
 *          piece of a row loads its positions and source elements once per sequence; few but long sequences are cut
 *          into blocks of 2 048 positions across workgroups (no workspace: a row needs nothing from another block).
 *          Trace: `seg_put_kernel`.
 * `out` must not alias `data` / `src` (RUA_EINVAL). */
int rua_segment_take(const rua_layout* lay, const void* data, const int64_t* index, void* out,
                     int64_t H, int32_t dtype, void* stream);
int rua_segment_put(const rua_layout* lay, const void* src, const int64_t* index, void* out,
                    int64_t H, int32_t dtype, void* stream);

/* After rua_segment_reduce / rua_pack_reduce with `extreme` (MAX/MIN/LOGSUMEXP): write the
 * global extreme — the reduce left it in the scratch — into the rows of empty sequences, or NaN into every row when
 * the NaN flag is up (the reference's initial=NaN behaviour).  Every workgroup patches its share of the batch.
 * (ABI <= 5 also took `data` and `perm` for a second walk over the payload; there is none any more.) */
int rua_fill_empty(const rua_layout* lay, void* out, int64_t H, int32_t dtype, int32_t op,
                   void* extreme, void* stream);

/* Bucket `index` (values in [0,S); others are ignored): counts[S], off[S] (exclusive scan) and perm[M] such that
 * perm[off[s] .. off[s]+counts[s]) are the rows i with index[i] == s IN ASCENDING ORDER — a stable radix sort on the
 * destination, deterministic for any fan-in.  513 .. 262 144 destinations with M < 2^31 (ABI 4): most significant
 * digit first in two levels, the second local to a bin, 32-bit words where (low digit, row) fit them
 * (rua_bucket_msd.hip; entries whose index is out of range are dropped and the tail of `perm` behind the valid
 * entries is left unwritten); otherwise least significant digit first over packed (destination, row) words with
 * <= 9-bit digits (rua_scatter.hip; needs bits(S) + bits(M) <= 62, RUA_ERANGE otherwise).  `ws` holds
 * rua_bucket_ws_elems(M, S) int64.  Feeds rua_segment_reduce(perm=..) for scatter_* (reduce.py:6-31). */
int64_t rua_bucket_ws_elems(int64_t M, int64_t S);
int rua_index_buckets(const int64_t* index, int64_t M, int64_t S, int64_t* counts, int64_t* off,
                      int64_t* perm, int64_t* ws, void* stream);

/* ---- host side of pack() (no GPU involved; plain host pointers) ------------------------------------------
 * sorted_indices of core/view.py:48 — `torch.sort(token_sizes.cpu(), descending=True)` — for int64 keys, with the
 * SAME tie order: ATen's CPU kernel is the C++ library's introsort over (key, index) pairs compared by key only,
 * a deterministic function of the input that is reproduced here step for step, the two halves of every partition
 * on different threads (n_threads >= 1, the caller included).  The Python layer verifies the equality against
 * torch.sort itself at first use and otherwise keeps making the reference's call. */
int rua_host_sort_desc(const int64_t* keys, int64_t n, int64_t* sorted_indices, int32_t n_threads);
/* The same sort on a helper thread (ABI 4): `begin` returns at once, `end` waits for the job and returns its code;
 * keys / sorted_indices must stay valid in between, one job at a time (RUA_EINVAL if one is already posted, or if `end`
 * finds none).  pack() with device-only lengths uses the interval for the rest of its host work (core/view.py:47-58:
 * batch_sizes, the offset scans), because the GPU idles until the order is known. */
int rua_host_sort_desc_begin(const int64_t* keys, int64_t n, int64_t* sorted_indices, int32_t n_threads);
int rua_host_sort_desc_end(void);
/* diagnostics for the tests: how many segments, over all calls so far, exhausted the introsort's depth budget and
 * were heap-sorted (the branch a random input never reaches; tests/golden/sort_killer.npy does) */
int64_t rua_host_sort_heap_segments(void);

/* batch_sizes[t] = #{b : lens[b] > t}, t < T — the CPU tensor PackedSequence mandates
 * (core/view.py:55: get_mask(self).sum(dim=0).cpu()), from the host copy of the lengths. */
int rua_host_batch_sizes(const int64_t* lens, int64_t B, int64_t T, int64_t* batch_sizes);

/* The two exclusive scans pack() needs next to batch_sizes (layout/pack.py:43-45 `offsets()`, utils.py:16-19), on the
 * host: boff[t] = sum of batch_sizes[< t], off[b] = sum of lens[< b] (either may be NULL).  With device-only lengths
 * the host computes them while the order is being sorted and uploads them with it (one launch less in front of the
 * mover); with a host mirror of the lengths they are derived on the device (rua_pack_prepare). */
int rua_host_pack_scans(const int64_t* lens, int64_t B, const int64_t* batch_sizes, int64_t T, int64_t* boff,
                        int64_t* off);

/* Introspection: ABI version and the gfx target the code objects were built for. */
/* Dispatch trace, for tests: while on, every launch of a segmented-reduce kernel (rua_segment_reduce, rua_pack_reduce,
 * rua_segment_reduce_backward, rua_fill_empty) and of the row mover (rua_move_rows) appends one record on the host — the kernel template's name as spelled
 * in rua_reduce_impl.h, then key=value pairs that tell its instantiations apart.  The log is process-global, holds the
 * newest 512 records and costs one relaxed load per dispatch while off.  rua_debug_trace switches it and returns the
 * previous state; rua_debug_trace_take copies whole records, one per line, into `buf`, removes them from the log and
 * returns the bytes written (with buf == NULL: the bytes the whole log needs, nothing removed). */
int rua_debug_trace(int32_t on);
int64_t rua_debug_trace_take(char* buf, int64_t cap);
/* The plan of a reduce call, without the call: the records rua_segment_reduce, rua_pack_reduce (`pack` = its second
 * layout) or rua_segment_reduce_backward would append to the trace for these arguments, one per line, into `buf`.
 * Launches nothing and touches no device.  In place of the device pointers: `present` says which optional ones are
 * given, `align` is the OR of the payload pointers' low 8 bits; of the layouts only scalars and the null-ness of
 * pointers are read.  Returns the bytes written (0: nothing to launch), the call's own RUA_E*, or RUA_ERANGE (`cap`). */
enum { RUA_PLAN_SEGMENT_REDUCE, RUA_PLAN_PACK_REDUCE, RUA_PLAN_BACKWARD };      /* `call` */
#define RUA_PLAN_PERM 1
#define RUA_PLAN_WS 2
#define RUA_PLAN_TIES 4
#define RUA_PLAN_SELF_IN 8
int64_t rua_debug_reduce_plan(int32_t call, const rua_layout* lay, const rua_layout* pack, int64_t H, int32_t dtype,
                              int32_t op, int32_t include_self, int64_t split_rows, int32_t present, int32_t align,
                              char* buf, int64_t cap);
/* The plan of a rua_move_rows call, without the call: the ONE record the call would append to the trace — the kernel
 * family (move_rows_kernel, move_rows_narrow_kernel, move_rows_span_kernel, seq_copy_kernel, pack_tile_lds_kernel,
 * pack_tile_vec_kernel, pack_roll_tile_kernel, pack_roll_steps_kernel), its template arguments, grid, per_xcd and the
 * run-time launch parameters — after the same validation and the same plan (csrc/rua_move_plan.h).  Launches nothing and
 * touches no device.  `dst_addr` / `src_addr` stand in for the payload pointers (only their alignment matters; 0 = NULL);
 * of the layouts only scalars, the null-ness of pointers and whether two of them are equal are read.  Returns the bytes
 * written to `buf` (no terminator; 0: nothing to launch), the call's own RUA_E*, or RUA_ERANGE (`cap`). */
int64_t rua_debug_move_plan(const rua_layout* dst, const rua_layout* src, int32_t tmap, int64_t tmap_arg,
                            uint64_t dst_addr, uint64_t src_addr, int64_t row_bytes, int64_t pad_row, int32_t flags,
                            char* buf, int64_t cap);
int rua_abi_version(void);
const char* rua_build_target(void);

#ifdef __cplusplus
}
#endif
#endif /* RUA_H_ */
