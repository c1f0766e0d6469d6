"""Per-sequence repeat_interleave over any container (C / L / P / R) — an extension, and the inverse direction of
`compress`: the ragged batch GROWS from the data.

    z.repeat_interleave(repeats)    the same container type, the same number of sequences B; sequence b is
                                    torch.repeat_interleave(seq_b, repeats_b, dim=0).  A count may be 0, so a sequence
                                    may become empty; all may.

This is the length regulator of duration-based TTS (FastSpeech), the upsampling of frame-level features to sample level,
a token -> sub-word alignment turned back into sub-word positions, the un-pooling after `seg`; it is the adjoint of
`seg(duration, segment_sum)`.  With the reference the spelling is `torch.repeat_interleave(c.data, counts, dim=0)` plus
a `segment_sum` of the counts and a new constructor — for a CattedSequence only — or a gather through an index built
with repeat_interleave / arange, with hand-rolled arithmetic for an L / R; a PackedSequence gets nothing (the sort order
of the result changes), and autograd keeps an int64 index per output token.

`repeats` is one of
  * a `torch.int64` tensor on the payload's device in the container's STORAGE layout of the token dimensions — [N] for
    C / P, [B, T_phys] for L / R; counts in padding rows of an L / R are never read;
  * a container of the same type whose `.data` is that tensor;
  * a Python int r >= 0: every token r times.
One value per token: counts with hidden dimensions are refused.  The counts are not differentiable.

The payload moves as BITS: every dtype of element size 1 / 2 / 4 / 8 (int64 token ids and bool included), 1-D payloads
and any hidden shape, any row width and alignment; a NaN keeps its bits.

The result is defined by commutation, as for `compress`.  For a C the data is the repeated rows in storage order and
`token_sizes` the new lengths (int64).  For every other layout X, `z.repeat_interleave(r)` equals
`z.cat().repeat_interleave(r_as_cat).X()` field by field and bit for bit, where `r_as_cat` is the counts cast like the
data: for a P that covers data, batch_sizes, sorted_indices and unsorted_indices, for an L / R the new T and zero padding
rows.  `z.repeat_interleave(r).cat()` equals `z.cat().repeat_interleave(r_as_cat)` likewise.  With a bool mask m,
`z.repeat_interleave(m.long()) == z.compress(m)`; `z.repeat_interleave(1) == z`; `z.repeat_interleave(0)` is empty.

INVALID COUNTS.  A negative count, or one above 2^31 - 1, raises RuaError (torch raises too).  The plan counts such
entries, takes them as 0 and leaves their number behind the new lengths, so the one read-back carries it.  A new
sequence longer than 2^31 - 1 tokens is refused after the read-back, before anything is allocated.  The one exception:
an int count on a C whose lengths the host never saw — that call never synchronises, so it cannot tell; its result is
sized N * r and the first cast that reads the lengths back sees them.

Three HIP kernels (csrc/rua_repeat.hip), identical for the four layouts.  The plan is a per-sequence exclusive scan of
the counts: `first`, the position of every token's first copy in its new sequence (int64 per storage row), and the new
lengths.  The move is DESTINATION-driven: the row of token (b, u) of the result reads the source token t, the largest t
with first[b, t] <= u — right with zero counts anywhere; a workgroup finds the source tokens of its block of consecutive
destination tokens once, stages their entries in LDS and searches there.  Padding rows of an L / R result are written as
zeros by the same launch.  The result's offsets and PackedSequence metadata come from the library's existing scan /
host-sort path over the new lengths.

SYNCHRONISATION.  With tensor counts the new lengths decide the allocation, so every call reads them back: ONE blocking
copy of [B + 1] int64 (torch.repeat_interleave synchronises too).  The host copy is attached to the result's lengths, so
a following `pack()` / `left()` / `size()` reads nothing back again.  With an int r the new lengths are r * len and the
source of output token u is u // r: no plan launch, no table; a C result never synchronises, an L / R / P result reads
the lengths back exactly when the corresponding cast would (not at all when they carry a host copy).

Autograd: `repeat` and its adjoint, the run sum (every token receives the sum of its copies' gradients, in ascending
order, accumulated in fp32 — fp64 for float64 — and rounded once; no atomics: the same bits from run to run and in every
layout), are two Functions that are each other's backward, so derivatives of every order exist.  Only `first` and the
caller's counts are saved (nothing for an int r) — no payload, no index per output token.  Gradients of tokens with
count 0 and of padding rows are exact zeros.  Integer and bool payloads pass through without a graph.  A very long run
(one count of 100 000) is summed by ONE thread group in the backward: correct, and slow.

Out of scope: per-column counts, fractional / interpolating upsampling, a caller-given capacity that never synchronises
(the follow-up `compress` names too), splitting long runs in the backward, differentiable durations, int32 counts.
"""
from typing import Tuple, Union

import torch
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.core import result_like
from torchrua_amd.layout import C, T, Z, cat_lay, check_per_token, install, lay_hidden, lead_shape, lens_of, side_payload

__all__ = ['segment_repeat_interleave', 'repeat_interleave']

MAX_COUNT = 2 ** 31 - 1


def _check_repeats(repeats, shape: Tuple[int, ...], data: Tensor, what: str) -> Union[int, Tensor]:
    """The counts as an int or a tensor, after the checks that need no device: int64, one value per token in the
    storage layout of the token dimensions, on the payload's device; an int is not negative."""
    if isinstance(repeats, int) and not isinstance(repeats, bool):
        if repeats < 0:
            raise K.RuaError(f'{what}: repeats is a negative int ({repeats}); it must be >= 0')
        if repeats > MAX_COUNT:
            raise K.RuaError(f'{what}: repeats is {repeats}; a count above 2^31 - 1 is invalid')
        return repeats
    if isinstance(repeats, Tensor) and repeats.dtype == torch.bool:
        raise K.RuaError(f'{what}: repeats has dtype torch.bool; keeping tokens by a mask is compress(mask)')
    return check_per_token(what, 'repeats', repeats, torch.int64, shape, data, or_form=', or an int')


def _too_long(new_sizes: Tensor, what: str) -> None:
    longest = M.known_max_len(new_sizes)
    if longest is not None and longest > MAX_COUNT:
        raise K.RuaError(f'{what}: a new sequence would hold {longest} tokens; the most is 2^31 - 1')


def _new_lengths(src: M.Lay, lens: Tensor, repeats: Union[int, Tensor], what: str):
    """(first, counts, uniform, new lengths).  Tensor counts: the plan and the call's ONE read-back — the new lengths
    and the number of invalid counts — with the host copy attached to the lengths.  An int: r * len, with the host copy
    when `lens` carries one; nothing is launched for the table and nothing is read back."""
    if isinstance(repeats, int):
        new_sizes = M._as_lens(lens) * repeats
        if M.host_known(lens):
            M.attach_host(new_sizes, M.private_host_copy(M.host_lens(lens) * repeats))
        _too_long(new_sizes, what)
        return None, None, repeats, new_sizes
    counts = O._plain(repeats).contiguous()
    first, buf = O.launch_repeat_plan(src, counts)
    host = M._read_back(buf)
    invalid = int(host[-1])
    if invalid:
        raise K.RuaError(f'{what}: {invalid} invalid count{"s" if invalid != 1 else ""} in repeats (negative, or above '
                         f'2^31 - 1)')
    # (the lengths are the first B words of the plan's [B + 1] buffer — a contiguous view at offset 0, not a tensor that
    # owns its storage as every other constructor's lengths do: the invalid-count word stays alive behind them.  A clone
    # would be one more launch per call for nothing a reader of `token_sizes` can see short of `untyped_storage()`)
    new_sizes = buf[:src.B]
    M.attach_host(new_sizes, host[:src.B])
    _too_long(new_sizes, what)
    return first, counts, 0, new_sizes


def segment_repeat_interleave(tensor: T, repeats, segment_sizes: T) -> Tuple[T, T]:
    """Row i of `tensor` [N, *hidden] `repeats[i]` times, and how many rows every run of `segment_sizes` rows becomes
    (the argument order of segment_compress): (tensor [N', *hidden], new_sizes [S] int64)."""
    repeats = _check_repeats(repeats, tuple(tensor.shape[:1]), tensor, 'segment_repeat_interleave')
    K.require_device(tensor, segment_sizes, repeats if isinstance(repeats, Tensor) else None)
    src, hidden = cat_lay(tensor, segment_sizes), tuple(tensor.shape[1:])
    first, counts, uniform, new_sizes = _new_lengths(src, segment_sizes, repeats, 'segment_repeat_interleave')
    n = int(tensor.size(0)) * uniform if first is None else M.total_len(new_sizes)
    dst = M.lay_cat(new_sizes, src.B, n)
    return O.repeat(tensor, first, counts, uniform, dst, src, hidden, (n,) + hidden, tuple(tensor.shape)), new_sizes


def repeat_interleave(sequence: Z, repeats) -> Z:
    """Every token `repeats[b, t]` (or `repeats`, an int) times in its own sequence; the same container type and number
    of sequences.  See the module docstring."""
    data = sequence.data
    repeats = side_payload(sequence, repeats, 'repeat_interleave: repeats given as a container must be a {want}; got {got}')
    repeats = _check_repeats(repeats, lead_shape(sequence), data, 'repeat_interleave')
    src, hidden = lay_hidden(sequence)
    first, counts, uniform, new_sizes = _new_lengths(src, lens_of(sequence), repeats, 'repeat_interleave')
    # (a C and an int count: N * r rows, known without a look at the lengths — a C result never synchronises)
    n = int(data.size(0)) * uniform if isinstance(sequence, C) and first is None else None
    if not isinstance(sequence, C):
        # (an int count and lengths the host never saw: the read-back the cast would do, BEFORE anything — batch_sizes
        # of a P, the storage of an L / R — is sized by it; the new lengths are known only now)
        M.max_len(new_sizes)
        _too_long(new_sizes, 'repeat_interleave')
    dst, shape, wrap = result_like(type(sequence), new_sizes, src.B, hidden, data, n)
    return wrap(O.repeat(data, first, counts, uniform, dst, src, hidden, shape, tuple(data.shape)))


install(repeat_interleave=repeat_interleave)
