"""Per-sequence cummax / cummin (with indices) and logcumsumexp over the tokens of any container (C / L / P / R) —
extensions, like cumsum: the running forms of `argmax` / `reduce_max` and of `segment_logsumexp`.  The stock spelling

    l = z.left(fill_value=-inf)
    v, i = torch.cummax(l.data, dim=1)                               # and a cast back

writes running values into the padding rows, is wrong for an R unless the fill is handled by hand and does not exist for
a PackedSequence; torch.logcumsumexp's own backward returns NaN as soon as a -inf is in a list.  Here each is ONE fused
HIP scan (csrc/rua_cumext.hip) on the cumsum's skeleton, identical for the four layouts.

    z.cummax(reverse=False), z.cummin(reverse=False)
        SeqCum(values, indices): torch.cummax(seq, dim=0) / torch.cummin(seq, dim=0) of every sequence on its own, per
        column, BIT FOR BIT in both outputs.  `values` has the container type, storage shape and dtype of z; `indices`
        the same container type and token layout, int64 — the token POSITION inside its own sequence, as in `sort` /
        `argmax`.  Both reuse z's `token_sizes` / PackedSequence metadata objects; nothing is read back.
        float32 / float64 / bfloat16 / float16 and int64.
    z.logcumsumexp(reverse=False)
        torch.logcumsumexp(seq, dim=0) of every sequence on its own; same container type, storage shape and dtype.
        The four float dtypes, fp32 accumulation (fp64 for float64), every output rounded once.
    segment_cummax / segment_cummin(tensor, sizes, reverse=False) -> (values, indices)
    segment_logcumsumexp(tensor, sizes, reverse=False)                 the `segment_*` argument style

Padding rows of an L / R result are zeros in every output and padding rows are never read; empty sequences contribute
nothing; other dtypes and CPU tensors raise RuaError before any launch (there is no CPU fallback).

TIES AND NaN (cummax / cummin) are torch's: among equal values the LATER position wins ([3, 3, 1, 3] -> indices
[0, 1, 1, 3]); -0.0 == +0.0 and the winner's bits are returned; once a NaN is met the value stays NaN and the index moves
on to every later NaN ([1, 1, 0, nan, 2, nan, 3] -> [0, 1, 1, 3, 3, 5, 5]).  This is the OPPOSITE of `argmax`'s "first
wins": `z.cummax().indices` at a sequence's last token is not `z.argmax()` when there are ties.  The state is
(value, position) under one total order, so the combine is associative and idempotent: every association order, layout
and kernel form gives the same bits.  The identity is "no element" (position -1), never a -inf that could beat a real
-inf at position 0.  `reverse=True` is the same scan on the mirrored token index, reported in un-mirrored positions:
z.cummax(reverse=True).values == z.rev().cummax().values.rev(), its indices are len - 1 - the mirrored ones, so among
equals the EARLIER position wins.

logcumsumexp folds the state (m, s), value m + log s, in the softmax kernels' convention and in cumsum's association
order (groups of 8, tiles of 32, blocks of 2 048, block bases added in block order): ONE order per (sequence, column,
direction), hence z.logcumsumexp().cat() == z.cat().logcumsumexp() bit for bit (L / R / P too) and
z.rev().logcumsumexp().rev() == z.logcumsumexp(reverse=True).  A prefix of only -inf gives -inf, not NaN; +inf gives
+inf from there on; a NaN poisons only the later tokens of its own sequence and column.  The identity (-inf, 0) is
absorbed exactly.

Autograd.  cummax / cummin: `values` is differentiable, `indices` is not; only the indices are saved; the backward is the
run sum of the cotangent at the run heads (rua_segment_cumextreme_backward: a segmented scan against the scan direction,
no atomics, one order), and the run sum and the per-element gather by the same indices are each other's backward, so
derivatives of every order exist; int64 payloads pass through without a graph.  logcumsumexp saves the input and the
output; the backward is one fused kernel, grad_in[s] = sum over t >= s of grad[t] * exp(x[s] - y[t]); a token with
x[s] = -inf gets gradient exactly 0 where torch gives NaN (a documented deviation: such a token takes no part in any
sum); create_graph=True raises (second derivatives are out of scope).  `cumprod` is out of scope.
"""
from typing import NamedTuple, Tuple

from torchrua_amd import _lib as K
from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, rewrap

__all__ = ['SeqCum', 'cummax', 'cummin', 'logcumsumexp', 'segment_cummax', 'segment_cummin', 'segment_logcumsumexp']


class SeqCum(NamedTuple):
    """What cummax / cummin return: two containers of the input's type."""
    values: Z
    indices: Z


def _segment(tensor: T, segment_sizes: T, op: int, reverse: bool) -> Tuple[T, T]:
    values, indices = O.cumextreme(tensor, cat_lay(tensor, segment_sizes), op, reverse, tuple(tensor.shape[1:]))
    return values, indices


def segment_cummax(tensor: T, segment_sizes: T, reverse: bool = False) -> Tuple[T, T]:
    """(values, indices) of the running max over every run of `segment_sizes` rows of `tensor`; both of its shape, the
    indices are positions inside the run."""
    return _segment(tensor, segment_sizes, K.MAX, reverse)


def segment_cummin(tensor: T, segment_sizes: T, reverse: bool = False) -> Tuple[T, T]:
    """(values, indices) of the running min over every run of `segment_sizes` rows of `tensor`."""
    return _segment(tensor, segment_sizes, K.MIN, reverse)


def segment_logcumsumexp(tensor: T, segment_sizes: T, reverse: bool = False) -> T:
    """logcumsumexp over every run of `segment_sizes` rows of `tensor`; same shape."""
    return O.logcumsumexp(tensor, cat_lay(tensor, segment_sizes), reverse, tuple(tensor.shape[1:]))


def _cumextreme(sequence: Z, op: int, reverse: bool) -> SeqCum:
    lay, hidden = lay_hidden(sequence)
    values, indices = O.cumextreme(sequence.data, lay, op, reverse, hidden)
    return SeqCum(rewrap(sequence, values), rewrap(sequence, indices))


def cummax(sequence: Z, reverse: bool = False) -> SeqCum:
    """SeqCum(values, indices): the running max of every sequence (from its end with `reverse`), torch's tie rule."""
    return _cumextreme(sequence, K.MAX, reverse)


def cummin(sequence: Z, reverse: bool = False) -> SeqCum:
    """SeqCum(values, indices): the running min of every sequence (from its end with `reverse`), torch's tie rule."""
    return _cumextreme(sequence, K.MIN, reverse)


def logcumsumexp(sequence: Z, reverse: bool = False) -> Z:
    """log of the running sum of exp over the tokens of every sequence; the same container type."""
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.logcumsumexp(sequence.data, lay, reverse, hidden))


install(cummax=cummax, cummin=cummin, logcumsumexp=logcumsumexp)
