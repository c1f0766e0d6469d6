"""Attention inside every sequence of a ragged batch, over unpadded storage — an extension, and the library's first
contraction: the operator users of ragged containers otherwise pad for (`left()` + a masked
`scaled_dot_product_attention` on the [B, T_max, ...] tensors the containers exist to avoid; nothing at all for a
PackedSequence).  Fused HIP kernels on the gfx950 matrix unit (csrc/rua_attention.hip), the same bits for
all 4 x 4 pairs of layouts.

    attention(q, k, v, causal=False, scale=None, window=None, align='start') -> container of q's type
                                                                                    also q.attention(k, v, ...)
    segment_attention(q, q_sizes, k, v, kv_sizes, causal=False, scale=None, window=None, align='start')
                                                                                    -> Tensor [N, heads, D]

`q` is a container (C / L / P / R) with exactly the hidden dimensions (heads, D); `k` and `v` are containers of ONE type
— any of the four, chosen independently of q's — with the hidden dimensions (heads_kv, D), the same as each other, the
same lengths as each other, and the same number of sequences, dtype and device as `q`.  Sequence b is the same sequence
in all three (a P: the original batch order).  `q.attention(q, q)` is self-attention; other kv lengths give
cross-attention.  For query t of sequence b and head h the output row is

    sum_s softmax_s(scale * q[t, h, :] . k[s, h // G, :]) * v[s, h // G, :]      over the VISIBLE kv tokens of sequence b

returned in q's container type, storage shape and dtype, with q's metadata objects; padding rows of L / R are zeros.
`scale=None` is D ** -0.5.  bfloat16 / float16, D in {32, 64, 128}.

HEADS.  heads % heads_kv == 0; with G = heads // heads_kv query head h reads kv head h // G (the `repeat_interleave`
convention: grouped-query attention, heads_kv == 1 multi-query).  K and V are never expanded; `grad_k` / `grad_v` have
the kv shape, the sum over the group taken in fp32 and rounded once.  G == 1 is the plain operator.

MASK.  Per sequence b with T_b queries and S_b keys, shift_b = 0 for align='start' and S_b - T_b for align='end' (the
last query sits on the last key: chunked prefill against a cache, a decoder over a memory plus its own prefix; it may
be negative).  Query t sees key s iff 0 <= s < S_b and -left <= s - (t + shift_b) <= right.  `window=None`: both sides
unbounded; `window=w` (an int >= 0): (w, w); `window=(left, right)`: each an int >= 0 or None (unbounded).
`causal=True` sets right = 0, so a causal window that sees W keys, the query's own included, is `causal=True,
window=W - 1`.  Only the tiles that meet the band are visited: a window makes the cost O(T W).

SEMANTICS — every input has one answer.  A sequence without queries produces no rows.  A query with NO visible key — a
sequence without keys; align='end' with T_b > S_b; a bounded left with t + shift_b - left >= S_b — gets a ZERO output
row, lse = -inf and zero gradients, and contributes nothing to grad_k / grad_v (torch's softmax over nothing gives NaN:
a documented deviation).  Non-finite inputs stay inside their own (sequence, head).  fp32 accumulation; the weights are
rounded once to the payload dtype before they meet `v` (bf16: hi + lo, the rounded remainder follows), their sum is taken
unrounded, every output element is rounded once (DESIGN 3.2r derives the error bound the tests assert).

AUTOGRAD.  Gradients flow to q, k and v; the forward saves them, the rounded output and an fp32 logsumexp
[q storage rows, heads]; the backward recomputes the weights, uses no atomics and is bitwise reproducible.
`create_graph=True` raises.

LENGTHS.  The launch is sized by the longest `q` sequence: with host lengths (C.new, with_host_sizes, a P, an earlier
read-back) nothing is read back, otherwise there is ONE blocking copy of [B], attached to the container.  The kv lengths
are needed on the host only by the backward's key-side grid (the same rule, and only when a gradient is requested);
align='end' takes S_b - T_b on the device and reads nothing back.  When `k` and `v` carry different device-only length
tensors whose host copies are unknown, their equality is not checked.

REFUSALS, all before any launch, each a RuaError naming the argument: something that is no container; a dtype other
than bf16 / f16 or dtypes that differ; hidden dimensions of `q` that are not exactly (heads, D); a `k` that is not
(heads_kv, D) with q's D, or whose heads do not divide q's; a `v` whose hidden dimensions differ from k's; D outside
{32, 64, 128}; `k` and `v` of different container type or lengths; another number of sequences or device; a `scale` that
is not a finite number; a `window` that is not None, an int >= 0 or a pair of such or None (bools are refused); a
`window` whose right side is neither None nor 0 together with `causal=True`; an `align` other than 'start' / 'end'; and
last a CPU tensor.

OUT OF SCOPE: additive bias or arbitrary masks, dropout, fp32 / fp64 payloads, other D, returning the weights, second
derivatives.  Decode steps — a handful of queries per sequence against a long cache — are `attention_decode` below: it
splits the keys of one sequence across workgroups and packs a group's heads into the matrix columns; `attention` is
correct there and wastes the tile, and never dispatches to it (the fold order differs).

DECODE.

    attention_decode(q, k, v, causal=True, scale=None, window=None, align='end', kv_chunk=None, return_lse=False,
                     k_scale=None, v_scale=None)
                                                                                    also q.attention_decode(k, v, ...)
    segment_attention_decode(q, q_sizes, k, v, kv_sizes, ...the same keywords...)   -> Tensor [N, heads, D]

The forward of `attention` for sequences of at most 32 queries (one new token per sequence, or a few for speculative
decoding or verification) over a ragged KV cache, as a split-KV kernel (csrc/rua_attention_decode.hip).  The
mathematics, the containers, the argument checks and the one-answer semantics are those above.  The differences:
  * THE DEFAULTS ARE THE DECODE MASK, `causal=True, align='end'` — not `attention`'s (`causal=False, align='start'`).
  * Forward only: the result carries no graph; with grad mode on and a `q.data` / `k.data` / `v.data` that requires grad
    it raises and names `attention`, the differentiable operator.
  * At most 32 queries per sequence; a longer one is refused and pointed to `attention` — from the host bound before any
    device work when the lengths are known, else after the one [B] read-back `attention` also makes.
  * The kv lengths are needed on the host (the longest one sizes the splits): nothing is read back with host lengths,
    otherwise ONE blocking [B] copy, attached to the container.
  * `kv_chunk`: the keys per split, None (the plan chooses: rua_attention_decode_plan, from B, the head counts, the
    longest q and kv sequence — never from a layout) or a positive multiple of 128.  THE BITS OF ONE SEQUENCE DEPEND ON
    THE PLAN — on `kv_chunk`, and through `kv_chunk=None` on the batch it is computed in; pin `kv_chunk` for run-to-run
    identical bits across batches.  For one batch all 4 x 4 pairs of layouts give the same bits; every call is bitwise
    reproducible (no atomics).
  * `return_lse=True` returns (out, lse): lse fp32 [*q storage rows, heads], the logsumexp of the scaled visible scores,
    -inf where nothing is visible, 0 in padding rows — what merging with attention over another cache segment needs.
  * AN 8-BIT CACHE: `k` and `v` may BOTH be `torch.float8_e4m3fn` (OCP e4m3) while `q` stays bf16 / f16 and fixes the
    compute and output dtype (csrc/rua_attention_decode_fp8.hip).  `k_scale` / `v_scale` are None (exactly
    1), a finite Python number > 0 (passed by value: no fill launch) or a float32 tensor [heads_kv] on q's device; the
    value of a cache element is float(code) * scale[hk], and the result is attention_decode of that dequantised cache —
    softmax_s(scale * q . (k8 * k_scale)) (v8 * v_scale), `lse` of those scaled scores — with the same zero rows, -inf
    and padding zeros.  The codes are converted exactly in registers; power-of-two scales add no rounding at all, others
    two to the score scale and one to the accumulator.  Nothing saturates or clamps; a NaN code (0x7F / 0xFF) stays
    inside its (sequence, kv head).  Refused: an fp8 `q`; one cache fp8 and the other not; any other 1-byte dtype
    (float8_e5m2, the fnuz types, uint8); a scale with a bf16 / f16 cache; a scale tensor that is not float32
    [heads_kv] on q's device or requires grad; a scale number that is not finite and > 0 (bools are refused).
    `attention` itself refuses fp8.
  * A PAGED CACHE: `attention_decode_paged(q, k_pages, v_pages, page_table, kv_sizes, ...the same keywords...)` (also
    `q.attention_decode_paged(...)` and `segment_attention_decode_paged(q, q_sizes, k_pages, ...)`;
    csrc/rua_attention_decode_paged.hip).  `k_pages` / `v_pages` are contiguous tensors [num_pages,
    page_size, heads_kv, D] of q's dtype or both float8_e4m3fn, page_size in {16, 32, 64, 128, 256}; `page_table` a
    contiguous int32 [B, max_pages] and `kv_sizes` an int64 [B] on q's device (sequence b of a P is the sequence in
    original order).  Key and value s of sequence b, 0 <= s < kv_sizes[b], are k_pages[page_table[b, s // page_size],
    s % page_size] and the same element of v_pages; THE RESULT IS attention_decode OVER THOSE ROWS GATHERED INTO A C
    CONTAINER, with the same keywords — for the same `kv_chunk` the same bits, out and lse.  Host-known kv_sizes: nothing
    is read back; otherwise ONE blocking [B] copy.  Table columns at or past ceil(kv_sizes[b] / page_size) and the rows of
    a last page past kv_sizes[b] are never read; two sequences may name the same page.  MEMORY SAFETY DOES NOT REST ON
    THE CALLER: a page id outside [0, num_pages) is never dereferenced — its keys and values read as zero rows, a
    defined result — and a max(kv_sizes) above max_pages * page_size is refused before the launch.  Refused besides what
    attention_decode refuses: pools that are not 4-D, differ from each other, are not contiguous, have another dtype,
    page_size, D or head ratio; a `page_table` that is not contiguous int32 [B, max_pages] on q's device; `kv_sizes`
    that are not int64 [B].

PREFILL OVER A PAGED CACHE.

    attention_paged(q, k_pages, v_pages, page_table, kv_sizes, causal=True, scale=None, window=None, align='end',
                    return_lse=False, k_scale=None, v_scale=None)                   also q.attention_paged(...)
    segment_attention_paged(q, q_sizes, k_pages, v_pages, page_table, kv_sizes, ...the same keywords...)

The forward of `attention` for ANY number of queries per sequence — a prompt, or a chunk of one — over the pool, table,
sizes and scales of `attention_decode_paged`, a bf16 / f16 or float8_e4m3fn cache (csrc/rua_attention_paged.hip; DESIGN
3.2v).  THE DEFAULTS ARE THE DECODE MASK.  THE RESULT IS attention(q, C(gathered k), C(gathered v), causal, scale, window,
align) over the rows the table names, an fp8 cache dequantised first: q's container type and metadata objects, zeros in
padding rows, a zero row and lse = -inf without a visible key; `return_lse=True` also returns attention_decode's lse.
Forward only (an input that requires grad under grad mode is refused and pointed to `attention`); no `kv_chunk`, no
32-query limit; ONE launch sized by the longest q sequence (attention's rule); `kv_sizes` by attention_decode_paged's
rule (host-known: nothing read back, else ONE [B] copy; a max above max_pages * page_size refused before the launch).
The refusals are attention_decode_paged's for the pool, table, sizes, scales and dtypes and attention's for the rest.  A
group's G query heads are packed into the matrix columns: a K / V tile is staged once per kv head, and all four q
layouts give the same bits — those of `attention` over the gathered cache, out and lse (an fp8 cache: with power-of-two
scales; others add the rounding terms of attention_decode's fp8 cache).

Out of scope there: gradients, more than 32 queries in a decode step, additive bias, merging across calls
(`return_lse` makes it possible outside), tuning the plan; of paged caches: an append or quantising append kernel
(`index_copy_` on the flat view of the pool does it), page sizes below 16 or not a power of two, int64 tables, the
head-major page layout [pages, heads_kv, page_size, D]; of 8-bit caches: float8_e5m2 and the fnuz formats, per-token
or per-block scales, int8 / int4, an fp8 `q` or output and the fp8 matrix instruction, a quantising `join`.
"""
import torch

from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import (P, T, Z, cat_lay, cls_of, hidden_of, install, lay_hidden, lens_of, n_seq, rewrap)
from torchrua_amd._lib import ATTN_DECODE_MAX_T, RuaError

__all__ = ['attention', 'segment_attention', 'attention_decode', 'segment_attention_decode', 'attention_decode_paged',
           'segment_attention_decode_paged', 'attention_paged', 'segment_attention_paged']


def _known_bound(z: Z):
    """The longest sequence if the host can tell without a device (None: it cannot)."""
    if isinstance(z, P):
        return int(z.batch_sizes.numel())
    return M.known_max_len(z.token_sizes) if z.token_sizes.numel() else 0


def _bound(z: Z) -> int:
    known = _known_bound(z)
    return known if known is not None else M.max_len(lens_of(z))


def _same_lengths(what: str, k: Z, v: Z) -> None:
    """`k` and `v` walk the same tokens: one type, one storage, the same lengths wherever the host can tell."""
    if cls_of(k) is not cls_of(v):
        raise RuaError(f'{what}: `k` and `v` are containers of ONE type; got {type(k).__name__} and {type(v).__name__}')
    a, b = (k.batch_sizes, v.batch_sizes) if isinstance(k, P) else (k.token_sizes, v.token_sizes)
    same = a is b
    if not same and M.host_known(a) and M.host_known(b):
        ha, hb = M.host_lens(a), M.host_lens(b)
        same = ha.shape == hb.shape and bool(torch.equal(ha.to(torch.long), hb.to(torch.long)))
    elif not same:
        same = a.shape == b.shape
    if not same or tuple(k.data.shape[:-2]) != tuple(v.data.shape[:-2]):
        raise RuaError(f'{what}: `k` and `v` have the same lengths (one key and one value per kv token)')


def _plan(what: str, q: Z, k: Z, v: Z, causal, scale, window, align) -> O.AttentionPlan:
    for name, z in (('q', q), ('k', k), ('v', v)):
        if cls_of(z) is None:
            raise RuaError(f'{what}: `{name}` is a container (C / L / P / R); got {type(z).__name__}')
    a = O.attention_args(what, q.data, hidden_of(q), n_seq(q), k.data, hidden_of(k), n_seq(k), v.data, hidden_of(v),
                         n_seq(v), scale, causal, window, align, before_device=lambda: _same_lengths(what, k, v))
    return O.AttentionPlan(lay_hidden(q)[0], lay_hidden(k)[0], a.heads, a.D, bool(causal), a.scale, _bound(q),
                           lambda: _bound(k), a.heads_kv, a.left, a.right, a.align_end)


def attention(q: Z, k: Z, v: Z, causal: bool = False, scale=None, window=None, align: str = 'start') -> Z:
    """softmax(q k^T * scale) v over the visible keys inside every sequence, in q's container type with its metadata
    objects."""
    plan = _plan('attention', q, k, v, causal, scale, window, align)
    return rewrap(q, O.attention(q.data, k.data, v.data, plan))


def segment_attention(q: T, q_sizes: T, k: T, v: T, kv_sizes: T, causal: bool = False, scale=None, window=None,
                      align: str = 'start') -> T:
    """Attention of every run of `q_sizes` rows of `q` [N, heads, D] over the run of `kv_sizes` rows of `k` / `v`
    [M, heads_kv, D]."""
    what = 'segment_attention'
    for name, t in (('q', q), ('q_sizes', q_sizes), ('k', k), ('v', v), ('kv_sizes', kv_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')

    def rows():
        if tuple(k.shape[:1]) != tuple(v.shape[:1]):
            raise RuaError(f'{what}: `k` and `v` have the same lengths (one key and one value per kv token)')

    n_kv = int(kv_sizes.numel())
    a = O.attention_args(what, q, tuple(q.shape[1:]), int(q_sizes.numel()), k, tuple(k.shape[1:]), n_kv, v,
                         tuple(v.shape[1:]), n_kv, scale, causal, window, align, before_device=rows)

    def bound(sizes):
        known = M.known_max_len(sizes) if sizes.numel() else 0
        return known if known is not None else M.max_len(sizes)

    plan = O.AttentionPlan(cat_lay(q, q_sizes), cat_lay(k, kv_sizes), a.heads, a.D, bool(causal), a.scale, bound(q_sizes),
                           lambda: bound(kv_sizes), a.heads_kv, a.left, a.right, a.align_end)
    return O.attention(q, k, v, plan)


def _decode_checks(what: str, tensors, kv_chunk, q_bound, names=('q', 'k', 'v')) -> None:
    """What attention_decode refuses on top of attention's checks, before the CPU-tensor refusal."""
    if kv_chunk is not None and (isinstance(kv_chunk, bool) or not isinstance(kv_chunk, int) or kv_chunk <= 0 or
                                 kv_chunk % 128):
        raise RuaError(f'{what}: `kv_chunk` = {kv_chunk!r} is None or a positive multiple of 128 (the keys per split)')
    _forward_only(what, tensors, names)
    _at_most_decode(what, q_bound)


def _forward_only(what: str, tensors, names) -> None:
    if torch.is_grad_enabled():
        for name, t in zip(names, tensors):
            if t.requires_grad:
                raise RuaError(f'{what}: `{name}` requires grad and {what} is forward only; `attention` is the '
                               f'differentiable operator')


def _at_most_decode(what: str, q_bound) -> None:
    if q_bound is not None and q_bound > ATTN_DECODE_MAX_T:
        raise RuaError(f'{what}: `q` holds a sequence of {q_bound} queries; a decode step has at most '
                       f'{ATTN_DECODE_MAX_T} per sequence — use `attention`')


def attention_decode(q: Z, k: Z, v: Z, causal: bool = True, scale=None, window=None, align: str = 'end', kv_chunk=None,
                     return_lse: bool = False, k_scale=None, v_scale=None):
    """`attention` for decode steps: at most 32 queries per sequence over a ragged KV cache, forward only, the keys split
    across workgroups.  THE DEFAULTS ARE THE DECODE MASK (`causal=True, align='end'`), unlike `attention`'s.  `k` / `v`
    may be a float8_e4m3fn cache with per-kv-head `k_scale` / `v_scale`."""
    what = 'attention_decode'
    for name, z in (('q', q), ('k', k), ('v', v)):
        if cls_of(z) is None:
            raise RuaError(f'{what}: `{name}` is a container (C / L / P / R); got {type(z).__name__}')

    scales = []

    def before_device():
        _same_lengths(what, k, v)
        _decode_checks(what, (q.data, k.data, v.data), kv_chunk, _known_bound(q))
        scales.extend(O.cache_scale(what, name, s, z.data, hidden_of(k)[0], q.data)
                      for name, s, z in (('k_scale', k_scale, k), ('v_scale', v_scale, v)))

    a = O.attention_args(what, q.data, hidden_of(q), n_seq(q), k.data, hidden_of(k), n_seq(k), v.data, hidden_of(v),
                         n_seq(v), scale, causal, window, align, before_device=before_device, kv_8bit=True)
    t_max = _bound(q)
    _at_most_decode(what, t_max)
    plan = O.AttentionPlan(lay_hidden(q)[0], lay_hidden(k)[0], a.heads, a.D, bool(causal), a.scale, t_max,
                           lambda: _bound(k), a.heads_kv, a.left, a.right, a.align_end)
    out, lse = O.attention_decode(q.data, k.data, v.data, plan, kv_chunk, *scales)
    return (rewrap(q, out), lse) if return_lse else rewrap(q, out)


def segment_attention_decode(q: T, q_sizes: T, k: T, v: T, kv_sizes: T, causal: bool = True, scale=None, window=None,
                             align: str = 'end', kv_chunk=None, return_lse: bool = False, k_scale=None, v_scale=None):
    """`attention_decode` of every run of `q_sizes` rows of `q` [N, heads, D] over the run of `kv_sizes` rows of `k` / `v`
    [M, heads_kv, D]."""
    what = 'segment_attention_decode'
    for name, t in (('q', q), ('q_sizes', q_sizes), ('k', k), ('v', v), ('kv_sizes', kv_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')

    def bound(sizes, known_only=False):
        known = M.known_max_len(sizes) if sizes.numel() else 0
        return known if known is not None or known_only else M.max_len(sizes)

    def before_device():
        if tuple(k.shape[:1]) != tuple(v.shape[:1]):
            raise RuaError(f'{what}: `k` and `v` have the same lengths (one key and one value per kv token)')
        _decode_checks(what, (q, k, v), kv_chunk, bound(q_sizes, True))
        scales.extend(O.cache_scale(what, name, s, t, int(k.shape[1]), q)
                      for name, s, t in (('k_scale', k_scale, k), ('v_scale', v_scale, v)))

    scales = []
    n_kv = int(kv_sizes.numel())
    a = O.attention_args(what, q, tuple(q.shape[1:]), int(q_sizes.numel()), k, tuple(k.shape[1:]), n_kv, v,
                         tuple(v.shape[1:]), n_kv, scale, causal, window, align, before_device=before_device, kv_8bit=True)
    t_max = bound(q_sizes)
    _at_most_decode(what, t_max)
    plan = O.AttentionPlan(cat_lay(q, q_sizes), cat_lay(k, kv_sizes), a.heads, a.D, bool(causal), a.scale, t_max,
                           lambda: bound(kv_sizes), a.heads_kv, a.left, a.right, a.align_end)
    out, lse = O.attention_decode(q, k, v, plan, kv_chunk, *scales)
    return (out, lse) if return_lse else out


PAGE_SIZES = (16, 32, 64, 128, 256)


def _table_fits(what: str, s_max, page_table: T, page_size: int) -> None:
    if s_max is not None and s_max > int(page_table.size(1)) * page_size:
        raise RuaError(f'{what}: `page_table` has {int(page_table.size(1))} columns of {page_size} keys and the longest '
                       f'sequence of `kv_sizes` holds {s_max}: the table names the pages of every key')


def _paged_plan(what: str, q: T, q_hidden, B: int, q_lay, q_bound, k_pages: T, v_pages: T, page_table: T, kv_sizes: T,
                causal, scale, window, align, k_scale, v_scale, decode: bool, kv_chunk=None):
    """(the plan, the two scales) of every paged form behind its own first checks.  `q` is the payload; `q_lay()` its
    layout; `q_bound(known_only)` its longest sequence (None: only a read-back can tell, and `known_only` forbids one).
    `decode`: attention_decode's own refusals (`kv_chunk`, at most 32 queries) apply; otherwise only its forward-only
    one does."""
    for name, t in (('k_pages', k_pages), ('v_pages', v_pages)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise RuaError(f'{what}: `{name}` is a tensor [num_pages, page_size, heads_kv, D]; got '
                           f'{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
    if tuple(v_pages.shape) != tuple(k_pages.shape):
        raise RuaError(f'{what}: `v_pages` has the shape {tuple(v_pages.shape)}, `k_pages` {tuple(k_pages.shape)}')
    for name, t in (('k_pages', k_pages), ('v_pages', v_pages)):
        if not t.is_contiguous():
            raise RuaError(f'{what}: `{name}` is contiguous (a pool is addressed by page id, never copied)')
    page_size = int(k_pages.size(1))
    if page_size not in PAGE_SIZES:
        raise RuaError(f'{what}: `k_pages` has page_size = {page_size}; it is one of {PAGE_SIZES}')
    scales = []

    def before_device():
        if (not isinstance(page_table, torch.Tensor) or page_table.dtype != torch.int32 or page_table.dim() != 2 or
                int(page_table.size(0)) != B or not page_table.is_contiguous() or page_table.device != q.device):
            got = (f'{page_table.dtype} {tuple(page_table.shape)} on {page_table.device}'
                   if isinstance(page_table, torch.Tensor) else type(page_table).__name__)
            raise RuaError(f'{what}: `page_table` is a contiguous int32 tensor [B, max_pages] = [{B}, max_pages] on '
                           f'{q.device}; got {got}')
        if (not isinstance(kv_sizes, torch.Tensor) or kv_sizes.dtype != torch.int64 or tuple(kv_sizes.shape) != (B,) or
                kv_sizes.device != q.device):
            got = (f'{kv_sizes.dtype} {tuple(kv_sizes.shape)} on {kv_sizes.device}'
                   if isinstance(kv_sizes, torch.Tensor) else type(kv_sizes).__name__)
            raise RuaError(f'{what}: `kv_sizes` is an int64 tensor [B] = [{B}] on {q.device}; got {got}')
        if decode:
            _decode_checks(what, (q, k_pages, v_pages), kv_chunk, q_bound(True), ('q', 'k_pages', 'v_pages'))
        else:
            _forward_only(what, (q, k_pages, v_pages), ('q', 'k_pages', 'v_pages'))
        scales.extend(O.cache_scale(what, name, s, t, int(k_pages.size(2)), q)
                      for name, s, t in (('k_scale', k_scale, k_pages), ('v_scale', v_scale, v_pages)))
        _table_fits(what, M.known_max_len(kv_sizes) if B else 0, page_table, page_size)

    a = O.attention_args(what, q, q_hidden, B, k_pages, tuple(k_pages.shape[2:]), B, v_pages, tuple(v_pages.shape[2:]), B,
                         scale, causal, window, align, before_device=before_device, kv_8bit=True,
                         kv_names=('k_pages', 'v_pages'))
    t_max = q_bound(False)
    if decode:
        _at_most_decode(what, t_max)
    s_max, kv_lay = 0, None
    if B and t_max and q.numel():                               # (else: zeros without a launch, as attention_decode)
        s_max = M.max_len(kv_sizes)                             # the ONE [B] read-back, when the host does not know them
        _table_fits(what, s_max, page_table, page_size)
        kv_lay = M.lay_cat(kv_sizes, B, M.total_len(kv_sizes))  # it supplies the lengths alone
    plan = O.AttentionPlan(q_lay(), kv_lay, a.heads, a.D, bool(causal), a.scale, t_max, lambda: s_max, a.heads_kv, a.left,
                           a.right, a.align_end)
    return plan, scales


def _decode_paged(what: str, q: T, q_hidden, B: int, q_lay, q_bound, k_pages: T, v_pages: T, page_table: T, kv_sizes: T,
                  causal, scale, window, align, kv_chunk, k_scale, v_scale):
    plan, scales = _paged_plan(what, q, q_hidden, B, q_lay, q_bound, k_pages, v_pages, page_table, kv_sizes, causal,
                               scale, window, align, k_scale, v_scale, True, kv_chunk)
    return O.attention_decode_paged(q, k_pages, v_pages, page_table, plan, kv_chunk, *scales)


def attention_decode_paged(q: Z, k_pages: T, v_pages: T, page_table: T, kv_sizes: T, causal: bool = True, scale=None,
                           window=None, align: str = 'end', kv_chunk=None, return_lse: bool = False, k_scale=None,
                           v_scale=None):
    """`attention_decode` over a PAGED cache: `k_pages` / `v_pages` [num_pages, page_size, heads_kv, D] (q's dtype or
    float8_e4m3fn), `page_table` int32 [B, max_pages], `kv_sizes` int64 [B].  Key s of sequence b is
    k_pages[page_table[b, s // page_size], s % page_size]; the result is attention_decode over those rows gathered into a
    C container — for the same `kv_chunk` the same bits."""
    what = 'attention_decode_paged'
    if cls_of(q) is None:
        raise RuaError(f'{what}: `q` is a container (C / L / P / R); got {type(q).__name__}')
    out, lse = _decode_paged(what, q.data, hidden_of(q), n_seq(q), lambda: lay_hidden(q)[0],
                             lambda known_only: _known_bound(q) if known_only else _bound(q), k_pages, v_pages, page_table,
                             kv_sizes, causal, scale, window, align, kv_chunk, k_scale, v_scale)
    return (rewrap(q, out), lse) if return_lse else rewrap(q, out)


def segment_attention_decode_paged(q: T, q_sizes: T, k_pages: T, v_pages: T, page_table: T, kv_sizes: T,
                                   causal: bool = True, scale=None, window=None, align: str = 'end', kv_chunk=None,
                                   return_lse: bool = False, k_scale=None, v_scale=None):
    """`attention_decode_paged` of every run of `q_sizes` rows of `q` [N, heads, D]."""
    what = 'segment_attention_decode_paged'
    for name, t in (('q', q), ('q_sizes', q_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')

    def bound(known_only):
        known = M.known_max_len(q_sizes) if q_sizes.numel() else 0
        return known if known is not None or known_only else M.max_len(q_sizes)

    out, lse = _decode_paged(what, q, tuple(q.shape[1:]), int(q_sizes.numel()), lambda: cat_lay(q, q_sizes), bound, k_pages,
                             v_pages, page_table, kv_sizes, causal, scale, window, align, kv_chunk, k_scale, v_scale)
    return (out, lse) if return_lse else out


def attention_paged(q: Z, k_pages: T, v_pages: T, page_table: T, kv_sizes: T, causal: bool = True, scale=None,
                    window=None, align: str = 'end', return_lse: bool = False, k_scale=None, v_scale=None):
    """The forward of `attention` for ANY number of queries per sequence over a PAGED cache — a prompt, or a chunk of
    one, against the pool `attention_decode_paged` reads, with its arguments: `k_pages` / `v_pages` [num_pages,
    page_size, heads_kv, D] (q's dtype or float8_e4m3fn), `page_table` int32 [B, max_pages], `kv_sizes` int64 [B].  THE
    DEFAULTS ARE THE DECODE MASK (`causal=True, align='end'`): the queries are the last T_b positions of a cache that
    already holds their keys.  The result is `attention` over the rows the table names gathered into a C container."""
    what = 'attention_paged'
    if cls_of(q) is None:
        raise RuaError(f'{what}: `q` is a container (C / L / P / R); got {type(q).__name__}')
    plan, scales = _paged_plan(what, q.data, hidden_of(q), n_seq(q), lambda: lay_hidden(q)[0],
                               lambda known_only: _known_bound(q) if known_only else _bound(q), k_pages, v_pages,
                               page_table, kv_sizes, causal, scale, window, align, k_scale, v_scale, False)
    out, lse = O.attention_paged(q.data, k_pages, v_pages, page_table, plan, *scales)
    return (rewrap(q, out), lse) if return_lse else rewrap(q, out)


def segment_attention_paged(q: T, q_sizes: T, k_pages: T, v_pages: T, page_table: T, kv_sizes: T, causal: bool = True,
                            scale=None, window=None, align: str = 'end', return_lse: bool = False, k_scale=None,
                            v_scale=None):
    """`attention_paged` of every run of `q_sizes` rows of `q` [N, heads, D]."""
    what = 'segment_attention_paged'
    for name, t in (('q', q), ('q_sizes', q_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')

    def bound(known_only):
        known = M.known_max_len(q_sizes) if q_sizes.numel() else 0
        return known if known is not None or known_only else M.max_len(q_sizes)

    plan, scales = _paged_plan(what, q, tuple(q.shape[1:]), int(q_sizes.numel()), lambda: cat_lay(q, q_sizes), bound,
                               k_pages, v_pages, page_table, kv_sizes, causal, scale, window, align, k_scale, v_scale,
                               False)
    out, lse = O.attention_paged(q, k_pages, v_pages, page_table, plan, *scales)
    return (out, lse) if return_lse else out


install(attention=attention, attention_decode=attention_decode, attention_decode_paged=attention_decode_paged,
        attention_paged=attention_paged)
