"""Per-sequence causal depthwise convolution over the tokens of any container (C / L / P / R) — an extension, the
neighbour of `linear_scan`: the short convolution over time that sits next to the state update of diagonal linear RNNs
and SSMs (Mamba, H3, Hyena), RWKV's token shift, Conformer-style depthwise convolutions.  Per sequence and per column h:

    causal_conv:                y[t] = bias[h] + sum_{k=0..K-1, t-(K-1)+k >= 0}   weight[k,h] * x[t-(K-1)+k]
    causal_conv(reverse=True):  y[t] = bias[h] + sum_{k=0..K-1, t+(K-1)-k < len}  weight[k,h] * x[t+(K-1)-k]

`weight` is [K, *hidden], tap-major — weight[K-1] multiplies the current token — and `bias` is [*hidden] or None; both
have the payload's dtype and device.  1 <= K <= 8.  For finite weights this is

    F.conv1d(x_seq.T[None], weight.reshape(K, H).T[:, None, :], bias, padding=K-1, groups=H)[..., :len]

of every sequence on its own; `reverse=True` is the anti-causal (look-ahead) mirror, and the adjoint the backward
needs.  With the reference the only spelling is `z.left()`, a transpose to [B, H, T], that conv1d, a slice, a transpose
and a cast back — five passes over the padded tensor, wrong for an R unless the padding is handled by hand, and nothing
at all for a PackedSequence.  Here it is ONE fused HIP kernel (rua_segment_causal_conv; csrc/rua_conv.hip), identical
for the four layouts: the payload is read once and written once, padding is never read.

The one difference from zero padding: a tap that falls outside the sequence is NOT EVALUATED rather than multiplied by
zero, so a non-finite weight does not poison the first K - 1 tokens.  Sequences and columns are independent: a NaN
reaches exactly the K outputs that depend on it.

float32 / float64 / bfloat16 / float16; bf16 and f16 accumulate in fp32 and every output is rounded once.  The result
has the container type, storage shape and dtype of the input; padding rows of an L / R result are zeros (in the
gradient too); an empty sequence contributes nothing; 1-D payloads take a weight of shape [K].  ONE evaluation order per
(token, column) — the accumulator starts at the bias (+0 without one), the taps that exist are added in ascending k
with a fused multiply-add — whatever the layout, the kernel form or the alignment, so, bit for bit: the operator
commutes with the casts (z.causal_conv(w, b).cat() == z.cat().causal_conv(w, b)), `reverse` is the mirrored forward
(z.rev().causal_conv(w, b).rev() == z.causal_conv(w, b, reverse=True)), and K == 1 with w == 1 and no bias returns the
input (but for the sign of a zero: the accumulator starts at +0).

Autograd saves the weight, and the payload only when the weight needs a gradient.  The backward is one fused entry
point: grad_input is the same kernel run the other way, and the same walk sums grad_weight and grad_bias per workgroup,
which a small finish launch adds up in a fixed order — no float atomics, so both are bitwise reproducible from run to run
for the same container (they are NOT the same bits across layouts: the order over the sequences follows the storage).
Derivatives of any order exist (composed from the convolution and its weight gradient, each the other's adjoint).

Out of scope: a fused activation (SiLU), an initial state or a streaming decode cache, dilation and stride, K > 8,
non-depthwise (channel-mixing) convolutions, weights that differ per sequence, integer payloads.
"""
from typing import Optional

from torch import Tensor

from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, hidden_of, install, lay_hidden, rewrap

__all__ = ['segment_causal_conv', 'causal_conv']


def segment_causal_conv(tensor: T, weight: T, segment_sizes: T, bias: Optional[Tensor] = None,
                        reverse: bool = False) -> T:
    """The convolution over every run of `segment_sizes` rows of `tensor` [N, *hidden] (the signature of
    segment_cumsum, plus the filter [K, *hidden] and the optional bias [*hidden]); same shape."""
    hidden = tuple(tensor.shape[1:])
    O._conv_args(tensor, weight, bias, hidden)
    return O.causal_conv(tensor, weight, bias, cat_lay(tensor, segment_sizes), reverse, hidden)


def causal_conv(sequence: Z, weight: T, bias: Optional[Tensor] = None, reverse: bool = False) -> Z:
    """y_t = bias + sum_k weight[k] * x_(t-(K-1)+k) over the tokens of every sequence (the taps look ahead with
    `reverse`); the same container type.  See the module docstring."""
    O._conv_args(sequence.data, weight, bias, hidden_of(sequence))       # (no device needed: the argument checks come first)
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.causal_conv(sequence.data, weight, bias, lay, reverse, hidden))


install(causal_conv=causal_conv)
