"""Per-sequence softmax and log_softmax over the tokens of any container (C / L / P / R) — an extension, like reduce_*
and pack_reduce: the reference has no such operator.  Its users spell it, for a CattedSequence only, as

    lse = torchrua.segment_logsumexp(x, sizes)                       # reduce.py:56-61
    y   = (x - torch.repeat_interleave(lse, sizes, dim=0)).exp()     # log variant: without .exp()

with [N, H] temporaries that autograd keeps.  Here it is ONE fused HIP kernel per direction (rua_segment_softmax,
rua_segment_softmax_backward; csrc/rua_softmax.hip), identical for the four layouts:

    softmax:      y[b,t,h] = exp(x[b,t,h] - lse[b,h])       lse[b,h] = logsumexp_t x[b,t,h]
    log_softmax:  y[b,t,h] =      x[b,t,h] - lse[b,h]

— torch.softmax(seq, dim=0) / torch.log_softmax(seq, dim=0) of every sequence on its own (a NaN stays inside its
sequence and column; the global `initial` of segment_logsumexp is NOT inherited).  The result has the container type,
storage shape and dtype of the input; padding rows of an L / R result are zeros.  The operator commutes with the casts
bit for bit: z.softmax().cat() == z.cat().softmax().  Autograd saves only y.
"""
from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, rewrap

__all__ = ['segment_softmax', 'segment_log_softmax', 'softmax', 'log_softmax']


def _segment(tensor: T, segment_sizes: T, log: bool) -> T:
    return O.softmax(tensor, cat_lay(tensor, segment_sizes), log, tuple(tensor.shape[1:]))


def segment_softmax(tensor: T, segment_sizes: T) -> T:
    """softmax over every run of `segment_sizes` rows of `tensor` (the signature of segment_logsumexp); same shape."""
    return _segment(tensor, segment_sizes, False)


def segment_log_softmax(tensor: T, segment_sizes: T) -> T:
    """log_softmax over every run of `segment_sizes` rows of `tensor`; same shape."""
    return _segment(tensor, segment_sizes, True)


def _seq(sequence: Z, log: bool) -> Z:
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.softmax(sequence.data, lay, log, hidden))


def softmax(sequence: Z) -> Z:
    """softmax over the tokens of every sequence; returns the same container type."""
    return _seq(sequence, False)


def log_softmax(sequence: Z) -> Z:
    """log_softmax over the tokens of every sequence; returns the same container type."""
    return _seq(sequence, True)


install(softmax=softmax, log_softmax=log_softmax)
