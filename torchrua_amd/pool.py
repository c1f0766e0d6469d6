"""Per-sequence softmax-weighted sum — attention pooling — over the tokens of any container (C / L / P / R): an
extension, like softmax and reduce_*.  For every sequence b and hidden column h

    out[b, h] = sum over t < len[b] of softmax_t(scores[b, :, g(h)])[t] * values[b, t, h]

i.e. `(torch.softmax(s_seq, dim=0)[..., None] * v_seq).sum(0)` of every sequence on its own.  With the reference the
spelling is segment_logsumexp + repeat_interleave + exp, a broadcast multiply and segment_sum: three passes over [N, H],
one [N, H] allocation, two [N, H] tensors kept by autograd, and for a CattedSequence only.  Here it is ONE fused HIP
kernel per direction (rua_segment_softmax_pool, rua_segment_softmax_pool_backward; csrc/rua_pool.hip), identical for
the four layouts: the values are read once and [B, H] is written — the traffic of reduce_sum.

`scores` is a container of the same type over the same lengths, or a plain tensor in the container's storage layout.
Its shape is the storage's token dims ([N] for C / P, [B, T] for L / R) followed by a PREFIX of the values' hidden dims,
possibly empty or the whole hidden shape: with G = prod(prefix) and D = H / G, column h is weighted by score column
h // D.  hidden (512,) with scores [N] is ordinary attention pooling, hidden (heads, d) with scores [N, heads] multi-head
pooling, scores of the full hidden shape a per-column weighting.

The result is [B, *hidden] in the batch order of reduce_sum and has the dtype of the values.  float32 / float64 /
bfloat16 / float16, scores in the values' dtype; accumulation in fp32 (fp64 for float64), every output rounded once.  An
empty sequence gives zeros.  A NaN or +inf score, or a sequence with only -inf scores, makes that (sequence, score
column) NaN and touches nothing else; a non-finite value poisons its own (sequence, column) even at weight 0, as the
torch spelling does.  Padding rows of L / R values and scores are never read, padding rows of their gradients are zeros.
One fold order per (sequence, column), so the operator commutes with the casts bit for bit.

Autograd saves the two inputs, the [B, H] output and a [B, G] logsumexp; gradients flow to values and scores; second
derivatives are out of scope (the backward raises under create_graph=True).  Out of scope as well: scores that broadcast
over anything but a trailing part of the hidden shape, masks and temperature (fold both into the scores), returning the
weights, integer payloads.
"""
import torch
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _ops as O
from torchrua_amd.layout import P, T, Z, cat_lay, install, lay_hidden, n_lead, side_payload

__all__ = ['segment_softmax_pool', 'softmax_pool']


def _score_columns(values: Tensor, scores: Tensor, lead: int) -> int:
    """G: the number of score columns, after checking the scores against the values' storage shape."""
    if not isinstance(scores, Tensor):
        raise K.RuaError(f'softmax_pool: the scores are a tensor or a container; got {type(scores).__name__}')
    K.require_device(values, scores)
    if values.dtype not in K.DTYPES:
        raise K.RuaError(f'softmax_pool supports {list(K.DTYPES)}; got {values.dtype}')
    if scores.dtype != values.dtype:
        raise K.RuaError(f'softmax_pool: the scores have dtype {scores.dtype}, the values {values.dtype}')
    vs, ss = tuple(values.shape), tuple(scores.shape)
    if values.dim() < lead or len(ss) < lead or len(ss) > len(vs) or ss != vs[:len(ss)]:
        raise K.RuaError(f'softmax_pool: scores of shape {ss} do not fit values of storage shape {vs}: the token dims '
                         f'{vs[:lead]} followed by a prefix of the hidden dims {vs[lead:]}')
    return O._prod(ss[lead:])


def segment_softmax_pool(tensor: T, scores: T, segment_sizes: T) -> T:
    """The softmax-weighted sum over every run of `segment_sizes` rows of `tensor` [N, *hidden] (the signature of
    segment_sum plus the scores [N, *prefix of hidden]); returns [B, *hidden]."""
    lay = cat_lay(tensor, segment_sizes)
    return O.softmax_pool(tensor, scores, lay, tuple(tensor.shape[1:]), _score_columns(tensor, scores, 1))


def _scores_data(sequence: Z, scores) -> Tensor:
    """The scores as a tensor (of a container: its payload; the container types must agree)."""
    data = side_payload(sequence, scores, 'softmax_pool: the scores are a {got}, the sequence a {want}; cast one of them first')
    if data is not scores and isinstance(sequence, P) and not torch.equal(scores.batch_sizes, sequence.batch_sizes):
        raise K.RuaError('softmax_pool: the scores and the sequence are PackedSequences with different batch_sizes')
    return data


def softmax_pool(sequence: Z, scores) -> T:
    """sum_t softmax_t(scores)[t] * sequence[t] over the tokens of every sequence -> [B, *hidden] in batch order.  See
    the module docstring for the score shapes."""
    data = sequence.data
    K.require_device(data)
    scores = _scores_data(sequence, scores)
    G = _score_columns(data, scores, n_lead(sequence))
    lay, hidden = lay_hidden(sequence)
    return O.softmax_pool(data, scores, lay, hidden, G)


install(softmax_pool=softmax_pool)
