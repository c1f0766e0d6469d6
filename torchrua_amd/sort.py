"""Per-sequence STABLE sort / argsort over any container (C / L / P / R), the permutation that goes with it, and top-k —
an extension: the library can say which token of a sequence is the largest (`argmax`) and keep tokens by a mask
(`compress`); this puts the tokens of every sequence in order.

    z.sort(descending=False)      SeqSort(values, indices): torch.sort(seq, dim=0, stable=True, descending=d) of every
                                  sequence on its own, per column.  `values` has the container type, storage shape and
                                  dtype of z; `indices` the same container type and token layout, int64 — the token
                                  POSITION inside its sequence (not a storage row) the value came from, so the indices
                                  mean the same in every layout.  Both reuse z's `token_sizes` / PackedSequence metadata
                                  objects: the raggedness does not change and nothing is read back.
    z.argsort(descending=False)   only the indices; no values are written.
    z.reorder(indices, inverse=False)
                                  a per-sequence permutation applied to another payload of the same raggedness.
                                  `indices` is int64, a tensor in the storage layout of the token dimensions or a
                                  container of z's type, of one of two shapes: the token dimensions alone — whole rows
                                  move, out[b, t, :] = z[b, indices[b, t], :] — or the token dimensions plus the full
                                  hidden shape — per element, out[b, t, h] = z[b, indices[b, t, h], h].
                                  inverse=True is the scatter out[b, indices[b, t], :] = z[b, t, :].
    z.topk(k, largest=True)       SeqSort of the first min(k, len) tokens of z.sort(descending=largest).
    segment_sort / segment_argsort(tensor, segment_sizes, descending=False)     the `segment_*` argument style

Listwise ranking losses over ragged candidate lists, top-k / top-p pruning before `compress`, per-utterance medians and
quantiles, NMS-style ordering of ragged detections, "reorder this batch by those scores" (`z.reorder(scores.argsort())`).
The stock spellings: `z.left(fill_value=inf)` + `torch.sort(dim=1)` + a cast back — a padded copy, wrong when the payload
holds inf or NaN, nothing for a PackedSequence — or two global stable sorts (by value, then by sequence id) over [N] and
an index rebuild.

THE ORDER is total on (key, position): NaN is greater than every number (ascending: NaNs last; descending: first),
-0.0 == +0.0, and equal keys — all NaNs among themselves too — keep ascending position in BOTH directions, which is what
stable=True gives with descending=True as well.  Because the order is total every kernel form and every layout gives
the same bits: `z.sort().values.cat() == z.cat().sort().values`, the same for `indices` and for L / R / P.  `values` are
the input elements bit for bit (a NaN keeps its payload, -0.0 stays -0.0).  float32 / float64 / bfloat16 / float16 and
int64.  An empty sequence contributes nothing; padding rows of L / R results are zeros in both outputs; a sequence of
2^31 or more tokens is refused.

`reorder` moves BITS: every dtype of element size 1 / 2 / 4 / 8 (bool included), 1-D payloads, any width and alignment.
CONTRACT: `indices` holds a permutation of [0, len[b]) per sequence (and per column) — what `argsort` returns; a
repeated position is undefined for the scatter.  A position outside [0, len[b]) is never dereferenced and produces
zeros, so the operator is memory-safe whatever it is given.  Padding rows of an L / R are never read and come back as
zeros.

Kernels (csrc/rua_sort.hip): sequences up to 64 tokens are sorted on the lanes of a wave by cross-lane
exchanges, several sequences per wave; up to 2 048 tokens by a bitonic network in LDS, a workgroup per (sequence,
column); longer ones block by block and then by rank-merge passes over a flat grid through a workspace.  The form goes
by the length BOUND the host knows without a look at the device: a CattedSequence whose lengths the host never saw is
bounded by its row count — correct, but short lists then take the block form and pay for empty merge launches; give
such a batch its lengths (`with_host_sizes`, `C.new`) or sort its padded / packed cast.

`topk` is a COMPOSITION, no kernel of its own: the full sort, then `unjoin` with the int size k — the library's closed
form for "the first min(k, len) tokens of every sequence".  It synchronises exactly when `unjoin` does (not at all when
the lengths carry a host copy).

Autograd: `values` is differentiable, `indices` is not; int64 payloads pass through without a graph.  sort's backward is
reorder(grad, indices, inverse=True) per element; reorder's gather and scatter are each other's backward, so derivatives
of every order exist.  Only the indices are saved.  Gradients of padding rows are exact zeros.  reorder's gradient
flows to the payload only.

Out of scope: sorting by a separate key container in one fused call, unstable or partial sorts, a fused top-k that
avoids the full sort, k-th value / quantile helpers, lexicographic row sorts, accumulating scatter for repeated indices.
"""
from numbers import Integral
from typing import NamedTuple, Tuple

import torch
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _ops as O
from torchrua_amd.layout import (T, Z, cat_lay, check_per_token, install, lay_hidden, lead_shape, require_container, rewrap,
                                 side_payload)

__all__ = ['SeqSort', 'sort', 'argsort', 'segment_sort', 'segment_argsort', 'reorder', 'topk']


class SeqSort(NamedTuple):
    """What sort / topk return: two containers of the input's type (segment_sort: two tensors)."""
    values: Z
    indices: Z


def _check_dtype(data: Tensor, what: str) -> None:
    if data.dtype not in K.SCAN_DTYPES:
        raise K.RuaError(f'{what} supports {[str(d) for d in K.SCAN_DTYPES]}; got {data.dtype}')


def segment_sort(tensor: T, segment_sizes: T, descending: bool = False) -> Tuple[T, T]:
    """Every run of `segment_sizes` rows of `tensor` [N, *hidden] sorted on its own, per column: (values, indices), both
    of the shape of `tensor`; the indices are positions inside the run."""
    _check_dtype(tensor, 'segment_sort')
    values, indices = O.sort(tensor, cat_lay(tensor, segment_sizes), descending, tuple(tensor.shape[1:]))
    return values, indices


def segment_argsort(tensor: T, segment_sizes: T, descending: bool = False) -> T:
    """The indices of segment_sort alone."""
    _check_dtype(tensor, 'segment_argsort')
    return O.sort(tensor, cat_lay(tensor, segment_sizes), descending, tuple(tensor.shape[1:]), want_values=False)[1]


def sort(sequence: Z, descending: bool = False) -> SeqSort:
    """SeqSort(values, indices): every sequence sorted stably on its own, per column.  See the module docstring."""
    require_container(sequence, 'sort')
    _check_dtype(sequence.data, 'sort')
    lay, hidden = lay_hidden(sequence)
    values, indices = O.sort(sequence.data, lay, descending, hidden)
    return SeqSort(rewrap(sequence, values), rewrap(sequence, indices))


def argsort(sequence: Z, descending: bool = False) -> Z:
    """The token positions that sort every sequence, as a container of the same type (int64)."""
    require_container(sequence, 'argsort')
    _check_dtype(sequence.data, 'argsort')
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.sort(sequence.data, lay, descending, hidden, want_values=False)[1])


def _check_indices(sequence: Z, indices, what: str) -> Tuple[Tensor, bool]:
    """(index tensor, per_row) after the checks that need no device: one index per token (whole rows), or — this
    operator's second form — one per element, in the full storage shape."""
    require_container(sequence, what)
    indices = side_payload(sequence, indices, what + ': indices given as a container must be a {want}; got {got}')
    lead, full = lead_shape(sequence), tuple(sequence.data.shape)
    per_row = not (isinstance(indices, Tensor) and tuple(indices.shape) == full != lead)
    check_per_token(what, 'indices', indices, torch.int64, lead if per_row else full, sequence.data, per_element=full)
    return indices, per_row


def reorder(sequence: Z, indices, inverse: bool = False) -> Z:
    """The tokens of every sequence permuted by `indices` (gather; inverse=True: scatter); the same container type."""
    indices, per_row = _check_indices(sequence, indices, 'reorder')
    if sequence.data.element_size() not in (1, 2, 4, 8):
        raise K.RuaError(f'reorder moves elements of 1, 2, 4 or 8 bytes; got {sequence.data.dtype}')
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.reorder(sequence.data, indices, lay, hidden, per_row, inverse))


def topk(sequence: Z, k: int, largest: bool = True) -> SeqSort:
    """SeqSort of the min(k, len) largest (smallest) tokens of every sequence, in sorted order, per column: the full
    stable sort followed by `unjoin` with the int size k — no kernel of its own; it synchronises exactly when `unjoin`
    does."""
    require_container(sequence, 'topk')
    if isinstance(k, bool) or not isinstance(k, Integral) or k < 0:
        raise K.RuaError(f'topk: k is {k!r}; it must be a non-negative int')
    out = sort(sequence, descending=bool(largest))
    return SeqSort(out.values.unjoin(int(k))[0], out.indices.unjoin(int(k))[0])


install(sort=sort, argsort=argsort, reorder=reorder, topk=topk)
