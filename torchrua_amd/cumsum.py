"""Per-sequence inclusive cumsum over the tokens of any container (C / L / P / R) — an extension, like softmax: the
reference has no prefix operator.  Its users spell it as

    l = z.left()
    y = l._replace(data=torch.cumsum(l.data, dim=1)).cat()           # and back to the container they came from

— three passes over the payload plus the padding, prefix values in the padding rows, and nothing at all for a
PackedSequence.  Here it is ONE fused HIP kernel (rua_segment_cumsum; csrc/rua_scan.hip), identical for the four
layouts:

    cumsum:                y[b,t,h] = sum over s <= t of x[b,s,h]
    cumsum(reverse=True):  y[b,t,h] = sum over s >= t of x[b,s,h]

— torch.cumsum(seq, dim=0) of every sequence on its own (a NaN or an infinity poisons only the later tokens of its own
sequence and column; with `reverse`, only the earlier ones).  float32 / float64 / bfloat16 / float16 (fp32 accumulation,
every output rounded once) and int64 (wraps).  The result has the container type, storage shape and dtype of the input;
padding rows of an L / R result are zeros.  The operator commutes with the casts bit for bit (z.cumsum().cat() ==
z.cat().cumsum()) and `reverse` is the same association order on the mirrored token index (z.rev().cumsum().rev() ==
z.cumsum(reverse=True)).  Autograd saves nothing: the backward is the scan in the other direction.
"""
from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import C, L, P, R, T, Z, describe

__all__ = ['segment_cumsum', 'cumsum']


def segment_cumsum(tensor: T, segment_sizes: T, reverse: bool = False) -> T:
    """cumsum over every run of `segment_sizes` rows of `tensor` (the signature of segment_sum); same shape."""
    K.require_device(tensor, segment_sizes)
    lay = M.lay_cat(segment_sizes, segment_sizes.numel(), int(tensor.size(0)))
    return O.cumsum(tensor, lay, reverse, tuple(tensor.shape[1:]))


def cumsum(sequence: Z, reverse: bool = False) -> Z:
    """Inclusive prefix sums (suffix sums with `reverse`) over the tokens of every sequence; the same container type."""
    data = sequence.data
    K.require_device(data)
    if isinstance(sequence, P):
        lay = M.lay_pack(sequence)
        y = O.cumsum(data, lay, reverse, tuple(data.shape[1:]))
        out = P(data=y, batch_sizes=sequence.batch_sizes, sorted_indices=sequence.sorted_indices,
                unsorted_indices=sequence.unsorted_indices)
        M.adopt_pack(out, M.pack_lens(sequence), M.pack_boff(sequence), M.pack_bsz_dev(sequence))
        return out
    hidden = tuple(data.shape[1:]) if isinstance(sequence, C) else tuple(data.shape[2:])
    return sequence._replace(data=O.cumsum(data, describe(sequence), reverse, hidden))


for _cls in (C, L, P, R):
    _cls.cumsum = cumsum
