"""Per-sequence edit distance and alignment of the tokens of any container (C / L / P / R) of hypotheses against the tokens
of ANOTHER ragged container of references — an extension: the last step of the ragged speech / sequence-labelling
pipeline.  `ctc_loss` trains, `argmax` -> `unique_consecutive` -> `compress` (the CTC collapse), `crf_decode` and `sort` /
`topk` produce int64 containers of hypotheses on the GPU; the number people then report is WER / CER / token error rate,
the Levenshtein distance of every hypothesis against its reference, split into substitutions, insertions and deletions.
The stock spelling is `tolist()` and a Python loop on the host: one blocking copy of everything, and nothing at all for
a PackedSequence.  Here both are fused HIP kernels (csrc/rua_edit.hip), pure integer arithmetic, the same
bits for all 4 x 4 pairs of layouts.

`hyp` and `ref` are int64 containers WITHOUT hidden dimensions, with the same number of sequences, on the same device;
each may be any of the four types, independently of the other.  Sequence b is the same sequence in both (a P: the
original batch order).  Tokens are compared as 64-bit values: any int64 is a token, there is no vocabulary and no range
check.

    edit_distance(hyp, ref) -> Tensor [B] int64                          also hyp.edit_distance(ref)
        Unit costs, in the batch order of `reduce_sum`.  Never differentiable.
    segment_edit_distance(tensor, sizes, other, other_sizes) -> [B]      the `segment_*` style
    edit_align(hyp, ref) -> SeqEdit(positions, distance, substitutions, insertions, deletions)
                                                                         also hyp.edit_align(ref)
        `positions` is an int64 container of hyp's type and token layout that reuses its metadata objects: for hyp token
        t the index into the sequence's own `ref` of the token it is paired with (a match or a substitution), -1 for an
        inserted token (a hyp token without a partner), zeros in the padding rows of L / R.  The deleted ref tokens are
        the ones no position names.  The four [B] int64 tensors satisfy, per sequence,
            substitutions + insertions + deletions == distance
            matches + substitutions + insertions == len(hyp_b)
            matches + substitutions + deletions == len(ref_b)
        WER is `distance / ref_len`; no normalised variant is offered.

SEMANTICS — exactly one answer for every input.  D[0][j] = j, D[i][0] = i,
D[i][j] = min(D[i-1][j-1] + (hyp[i-1] != ref[j-1]), D[i-1][j] + 1, D[i][j-1] + 1).  The alignment is the backtrace from
(T, S), which takes the diagonal if it attains D[i][j], else up (an insertion), else left (a deletion); at i == 0 only
left exists, at j == 0 only up.  T = 0: distance = deletions = S and no tokens; S = 0: distance = insertions = T and all
positions -1; both empty: zeros.

LENGTHS.  The column bucket goes by the longest `ref` of the batch, so the host must know the ref lengths: with host
lengths (C.new, with_host_sizes, a P, an earlier read-back) nothing is read back; otherwise there is ONE blocking copy of
[B] int64, attached to the container.  The lengths of `hyp` are never needed on the host.  The longest `ref` allowed is
2 048 tokens; `hyp` is unbounded.  The limit is asymmetric on purpose: a caller with a long `ref` and a short `hyp` swaps
the arguments: the distance is symmetric and insertions and deletions trade places (insertions - deletions changes sign
exactly; where the two backtraces split a tie differently, a substitution of one is an insertion + deletion pair of the
other — 5 of 3 000 random pairs).

REFUSALS, all before any launch, each a RuaError naming the argument: a CPU tensor; something that is no container; a
dtype other than int64 on either side; hidden dimensions on either side; another number of sequences; another device; a
`ref` longer than 2 048 (from the host bound, before any device work, when the bound is known).

LIMITS: one long ref sends the whole batch to the workgroup form; one wave (one workgroup) walks all the tokens of a
hyp; `edit_align` keeps a code table of ONE BYTE per cell, [*hyp storage rows, S_max] (2 bits of information: packing
would not be free) — N x S_max bytes, 0.8 GB for 400 000 hyp tokens against refs of up to 2 048 — and walks it with one
thread per sequence; `edit_distance` allocates and writes no table.
"""
from typing import NamedTuple

import torch

from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import (P, T, Z, cat_lay, cls_of, hidden_of, install, lay_hidden, lead_shape, lens_of, n_seq,
                                 require_container, rewrap)
from torchrua_amd._lib import RuaError

__all__ = ['SeqEdit', 'edit_distance', 'segment_edit_distance', 'edit_align']


class SeqEdit(NamedTuple):
    """What edit_align returns: the ref position every hyp token is paired with (a container of hyp's type; -1: an
    insertion) and, per sequence, the distance and its split [B]."""
    positions: Z
    distance: T
    substitutions: T
    insertions: T
    deletions: T


def _known_bound(ref: Z):
    """The longest ref if the host can tell without a device (None: it cannot)."""
    if isinstance(ref, P):
        return int(ref.batch_sizes.numel())
    return M.known_max_len(ref.token_sizes) if ref.token_sizes.numel() else 0


def _plan(what: str, hyp: Z, ref: Z) -> O.EditPlan:
    require_container(hyp, what)
    if cls_of(ref) is None:
        raise RuaError(f'{what}: `ref` is a container (C / L / P / R) of int64 tokens; got {type(ref).__name__}')
    known = _known_bound(ref)
    O.edit_args(what, hyp.data, hidden_of(hyp), n_seq(hyp), ref.data, hidden_of(ref), n_seq(ref),
                before_device=None if known is None else (lambda: O.edit_ref_bound(what, known)))
    s_max = known if known is not None else O.edit_ref_bound(what, M.max_len(lens_of(ref)))
    return O.EditPlan(lay_hidden(hyp)[0], lay_hidden(ref)[0], s_max)


def edit_distance(hyp: Z, ref: Z) -> T:
    """The Levenshtein distance [B] int64 of every sequence of `hyp` against the same sequence of `ref` (unit costs),
    in the batch order of `reduce_sum`.  Never differentiable; no table is allocated."""
    plan = _plan('edit_distance', hyp, ref)
    return O.launch_edit_forward(plan, hyp.data.detach(), ref.data.detach())[0]


def segment_edit_distance(tensor: T, segment_sizes: T, other: T, other_sizes: T) -> T:
    """The distance of every run of `segment_sizes` tokens of `tensor` [N] against the run of `other_sizes` tokens of
    `other` [M]."""
    what = 'segment_edit_distance'
    for name, t in (('tensor', tensor), ('segment_sizes', segment_sizes), ('other', other), ('other_sizes', other_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')
    known = M.known_max_len(other_sizes) if other_sizes.numel() else 0
    O.edit_args(what, tensor, tuple(tensor.shape[1:]), int(segment_sizes.numel()), other, tuple(other.shape[1:]),
                int(other_sizes.numel()),
                before_device=None if known is None else (lambda: O.edit_ref_bound(what, known)))
    s_max = known if known is not None else O.edit_ref_bound(what, M.max_len(other_sizes))
    plan = O.EditPlan(cat_lay(tensor, segment_sizes), cat_lay(other, other_sizes), s_max)
    return O.launch_edit_forward(plan, tensor.detach(), other.detach())[0]


def edit_align(hyp: Z, ref: Z) -> SeqEdit:
    """SeqEdit(positions, distance, substitutions, insertions, deletions): the backtrace that prefers the diagonal,
    then up (an insertion), then left (a deletion)."""
    plan = _plan('edit_align', hyp, ref)
    distance, codes = O.launch_edit_forward(plan, hyp.data.detach(), ref.data.detach(), want_codes=True)
    positions, subs, ins, dels = O.launch_edit_backtrace(plan, codes, lead_shape(hyp))
    return SeqEdit(rewrap(hyp, positions), distance, subs, ins, dels)


install(edit_distance=edit_distance, edit_align=edit_align)
