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
from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, rewrap

__all__ = ['segment_cumsum', 'cumsum']


def segment_cumsum(tensor: T, segment_sizes: T, reverse: bool = False) -> T:
    """cumsum over every run of `segment_sizes` rows of `tensor` (the signature of segment_sum); same shape."""
    return O.cumsum(tensor, cat_lay(tensor, segment_sizes), reverse, tuple(tensor.shape[1:]))


def cumsum(sequence: Z, reverse: bool = False) -> Z:
    """Inclusive prefix sums (suffix sums with `reverse`) over the tokens of every sequence; the same container type."""
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.cumsum(sequence.data, lay, reverse, hidden))


install(cumsum=cumsum)
