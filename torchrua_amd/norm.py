"""Per-sequence mean / variance and standardize over the tokens of any container (C / L / P / R) — an extension, like
softmax and reduce_*: the reference has no second moment.  Its users spell it, for a CattedSequence only, as

    mean = torchrua.segment_mean(x, sizes)                                    # reduce.py:44-49
    dev  = x - torch.repeat_interleave(mean, sizes, dim=0)
    var  = torchrua.segment_mean(dev * dev, sizes)                            # correction = 0
    y    = dev * torch.repeat_interleave((var + eps).rsqrt(), sizes, dim=0)

— five passes over [N, H] and three [N, H] temporaries that autograd keeps.  Here it is ONE fused HIP kernel per
direction (rua_segment_var_mean, rua_segment_standardize and their backwards; csrc/rua_norm.hip), identical for the
four layouts.  With n = len[b] and c = correction:

    mean[b,h] = (1/n) sum_t x[b,t,h]        var[b,h] = sum_t (x[b,t,h] - mean[b,h])^2 / (n - c)
    standardize:  y[b,t,h] = (x[b,t,h] - mean[b,h]) / sqrt(var[b,h] + eps)

— torch.var_mean(seq, dim=0, correction=c) and (seq - mean) * rsqrt(var + eps) of every sequence on its own: per-utterance
CMVN, instance normalisation over time, per-episode advantage normalisation.  float32 / float64 / bfloat16 / float16;
fp32 accumulation (fp64 for float64), a numerically stable (Welford / Chan) fold, every output rounded once.  `var` and
`mean` are [B, *hidden] in the batch order of reduce_sum; standardize returns the container type, storage shape and
dtype of its input, padding rows of an L / R result are zeros.  n - c <= 0 gives NaN (an empty sequence: NaN var and
mean, and it owns no row); a NaN or an infinity stays inside its sequence and column; a constant column has var == 0
exactly.  One fold order per (sequence, column), so the operators commute with the casts bit for bit:
z.standardize().cat() == z.cat().standardize().  Autograd saves only y and a [B, H] rstd (standardize), the input and
the [B, H] mean (var_mean); both differentiate twice.

Out of scope: std (`var(z).sqrt()` on [B, H] is cheap), an affine weight and bias, statistics over the hidden dimension
(layer norm proper), running statistics, masks.
"""
from typing import Tuple

from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, rewrap

__all__ = ['segment_var_mean', 'segment_var', 'segment_standardize', 'var_mean', 'var', 'standardize']


def segment_var_mean(tensor: T, segment_sizes: T, correction: int = 1) -> Tuple[T, T]:
    """(var, mean) over every run of `segment_sizes` rows of `tensor` [N, *hidden] (the signature of segment_mean);
    each [B, *hidden]."""
    return O.var_mean(tensor, cat_lay(tensor, segment_sizes), tuple(tensor.shape[1:]), correction)


def segment_var(tensor: T, segment_sizes: T, correction: int = 1) -> T:
    """The variance over every run of `segment_sizes` rows of `tensor`; [B, *hidden]."""
    return O.var_mean(tensor, cat_lay(tensor, segment_sizes), tuple(tensor.shape[1:]), correction, want_mean=False)[0]


def segment_standardize(tensor: T, segment_sizes: T, eps: float = 1e-5, correction: int = 0) -> T:
    """(x - mean) / sqrt(var + eps) over every run of `segment_sizes` rows of `tensor`; same shape."""
    return O.standardize(tensor, cat_lay(tensor, segment_sizes), tuple(tensor.shape[1:]), eps, correction)


def var_mean(sequence: Z, correction: int = 1) -> Tuple[T, T]:
    """(var, mean) over the tokens of every sequence -> two [B, *hidden] tensors in batch order."""
    lay, hidden = lay_hidden(sequence)
    return O.var_mean(sequence.data, lay, hidden, correction)


def var(sequence: Z, correction: int = 1) -> T:
    """The variance over the tokens of every sequence -> [B, *hidden] in batch order."""
    lay, hidden = lay_hidden(sequence)
    return O.var_mean(sequence.data, lay, hidden, correction, want_mean=False)[0]


def standardize(sequence: Z, eps: float = 1e-5, correction: int = 0) -> Z:
    """Every sequence minus its own mean, over its own standard deviation; returns the same container type."""
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.standardize(sequence.data, lay, hidden, eps, correction))


install(var_mean=var_mean, var=var, standardize=standardize)
