"""Per-sequence unique_consecutive (run-length encode) over any container (C / L / P / R) — an extension, and the inverse
of `repeat_interleave`: collapse every run of equal consecutive tokens INSIDE each sequence to one token and say how long
the run was.

    z.unique_consecutive(return_inverse=False, return_counts=False)
                           SeqRuns(values, inverse, counts).  For every sequence b on its own:
                           torch.unique_consecutive(seq_b, dim=0, return_inverse=True, return_counts=True).
                           A field that was not asked for is None and the launches that only produce it are skipped.
    segment_unique_consecutive(tensor, sizes, return_inverse=False, return_counts=False)
                           the `segment_*` argument style: (values [N', *hidden], new_sizes [S] int64,
                           inverse [N] int64 | None, counts [N'] int64 | None)

CTC greedy decoding (`argmax` ids, collapse repeats, then `compress` the blanks away), a frame-level alignment turned
into (phone, duration) pairs — the `duration` container `seg(duration, fn)` and `repeat_interleave` take —
de-duplicating repeated frames, run-level pooling (`z.seg(counts, segment_mean)`).  The stock spellings: a Python loop
of `torch.unique_consecutive` over the sequences (a global call merges a run across the border of two sequences), or a
mask built with `roll` and `!=` — `roll` wraps, so a sequence's first token meets its last; rows with hidden dims need an
`.all(-1)` over an [N, H] bool temporary; the counts a second pass; a PackedSequence a fresh host sort.

EQUALITY.  Two tokens are equal when all their elements are equal under the dtype's `==`.  For float32 / float64 /
bfloat16 / float16 that is IEEE equality: a NaN equals nothing, so a row that holds one is always a run of one, and
-0.0 == +0.0, so such rows merge.  For every other dtype of 1 / 2 / 4 / 8 bytes (int64 ids, int32, uint8, bool ...) it
is equality of bits.  Complex dtypes and other element sizes are refused.

`values`: the container type of z, the same B, dtype and hidden shape; sequence b holds the FIRST token of each of its
runs, moved as bits (a NaN keeps its payload, a leading -0.0 its sign).  An empty sequence stays empty; a non-empty one
has at least one run.  `counts`: a container of the same type and raggedness as `values` that shares its lengths /
PackedSequence metadata objects; int64, one value per run ([N'], or [B, T'] with zero padding).  `inverse`: a container
of z's type that reuses z's metadata objects; int64, one value per token — the index of the token's run inside its own
sequence, so like `sort`'s indices it means the same in every layout; padding rows of an L / R are zeros.

The result is defined by commutation, as for `compress`: `z.unique_consecutive(...)` equals
`z.cat().unique_consecutive(...).X()` field by field and bit for bit for all three outputs (X = left / right / pack; a
P's batch_sizes, sorted_indices and unsorted_indices, an L / R's new T' and zero padding included), and the same with
`.cat()` on the outside.

Kernels (csrc/rua_runs.hip).  `heads` is the only one that reads the payload: a byte per storage row,
whether the token starts a run — the token's predecessor is found through the layout's own row formula, so a sequence's
first token is compared with nothing and padding is never read.  That mask goes through `compress`'s plan (rank, new
lengths) and move (the values), unchanged.  `inverse` is the same offsets scan over the mask with an int64 result;
`counts` scatters the heads' positions into a table laid out like the result and subtracts neighbours — no atomics.

SYNCHRONISATION.  ONE blocking read-back of the [B] new lengths, as in `compress`; the host copy is attached to the
result, so a following `pack()` / `left()` / `seg(counts, fn)` reads nothing back (`repeat_interleave(counts)` reads
only what its own plan always reads: its new lengths).  The values are produced whichever flags are set.

Autograd: `values` is differentiable exactly as a `compress` by the "first of its run" mask is — the `_Compress` /
`_Expand` pair with the int32 rank table, nothing else saved, derivatives of every order.  The gradient of a run goes to
its first token; every other token and every padding row gets exact zeros, whatever the payload holds.  `inverse` and
`counts` carry no graph; integer and bool payloads pass through without one.

Out of scope: a variant with a caller-given capacity that never synchronises, run means (`z.seg(counts, segment_mean)`),
a tolerance for "nearly equal" frames, dropping a blank id in the same pass (`compress` after it).
"""
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.core import result_like
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, n_lead, require_container, rewrap

__all__ = ['SeqRuns', 'segment_unique_consecutive', 'unique_consecutive']


class SeqRuns(NamedTuple):
    """What unique_consecutive returns: `values` and `counts` share one raggedness, `inverse` has the input's."""
    values: Z
    inverse: Optional[Z]
    counts: Optional[Z]


def _check_dtype(data: Tensor, what: str) -> None:
    """Before the device check: the refusal names the dtype whatever device the payload is on."""
    if data.is_complex():
        raise K.RuaError(f'{what}: complex payloads are refused ({data.dtype})')
    if data.element_size() not in (1, 2, 4, 8):
        raise K.RuaError(f'{what} compares elements of 1, 2, 4 or 8 bytes; got {data.dtype}')


def _plan(big: M.Lay, data: Tensor, hidden: Tuple[int, ...], lead: Tuple[int, ...], want_inverse: bool):
    """(rank, new lengths, inverse | None): the heads, the compress plan over them, the optional inverse scan, then the
    call's ONE read-back, its host copy attached to the lengths."""
    if big.n_rows == 0:                                    # a storage without rows: B empty sequences, nothing to launch
        rank = torch.empty(0, dtype=torch.int32, device=data.device)
        new_sizes = torch.zeros(big.B, dtype=torch.int64, device=data.device)
        inverse = torch.zeros(lead, dtype=torch.int64, device=data.device) if want_inverse else None
    else:
        head = O.launch_runs_heads(big, data, hidden)
        rank, new_sizes = O.launch_compress_plan(big, head)
        inverse = O.launch_runs_inverse(big, head, lead) if want_inverse else None
    M.read_back_rows(new_sizes, [new_sizes])
    return rank, new_sizes, inverse


def segment_unique_consecutive(tensor: T, segment_sizes: T, return_inverse: bool = False, return_counts: bool = False
                               ) -> Tuple[T, T, Optional[T], Optional[T]]:
    """Every run of `segment_sizes` rows of `tensor` [N, *hidden] run-length encoded on its own: (values [N', *hidden],
    new_sizes [S] int64, inverse [N] int64 | None, counts [N'] int64 | None)."""
    _check_dtype(tensor, 'segment_unique_consecutive')
    K.require_device(tensor, segment_sizes)
    tensor = tensor.contiguous()
    big, hidden = cat_lay(tensor, segment_sizes), tuple(tensor.shape[1:])
    rank, new_sizes, inverse = _plan(big, tensor, hidden, tuple(tensor.shape[:1]), return_inverse)
    n = M.total_len(new_sizes)
    small = M.lay_cat(new_sizes, big.B, n)
    values = O.compress(tensor, rank, small, big, hidden, (n,) + hidden, tuple(tensor.shape))
    counts = O.launch_runs_counts(small, big, rank, (n,)) if return_counts else None
    return values, new_sizes, inverse, counts


def unique_consecutive(sequence: Z, return_inverse: bool = False, return_counts: bool = False) -> SeqRuns:
    """SeqRuns(values, inverse, counts): every sequence run-length encoded on its own.  See the module docstring."""
    require_container(sequence, 'unique_consecutive')
    _check_dtype(sequence.data, 'unique_consecutive')
    big, hidden = lay_hidden(sequence)
    data = sequence.data.contiguous()
    lead = n_lead(sequence)
    rank, new_sizes, inverse = _plan(big, data, hidden, tuple(data.shape[:lead]), return_inverse)
    small, shape, wrap = result_like(type(sequence), new_sizes, big.B, hidden, data)
    values = wrap(O.compress(data, rank, small, big, hidden, shape, tuple(data.shape)))
    counts = wrap(O.launch_runs_counts(small, big, rank, shape[:lead])) if return_counts else None
    return SeqRuns(values, None if inverse is None else rewrap(sequence, inverse), counts)


install(unique_consecutive=unique_consecutive)
