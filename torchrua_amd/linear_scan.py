"""Per-sequence gated linear recurrence over the tokens of any container (C / L / P / R) — an extension, like cumsum:

    linear_scan:                h[b,0]     = x[b,0]                           h[b,t] = a[b,t] * h[b,t-1] + x[b,t]
    linear_scan(reverse=True):  h[b,len-1] = x[b,len-1]                       h[b,t] = a[b,t] * h[b,t+1] + x[b,t]

per sequence and per column: discounted returns and GAE over episodes of unequal length (`reverse` is the return
recursion G_t = r_t + a_t * G_(t+1); a = gamma, or gamma * (1 - done)), exponential moving averages, gated and decayed
cumulative sums, the state update of diagonal linear RNNs and SSMs.  With the reference the only spelling is
`z.left()`, a Python loop over the time steps on the padded tensor and a cast back — T launches and traffic over the
padding, and nothing at all for a PackedSequence.  Here it is ONE fused HIP kernel (rua_segment_linear_scan;
csrc/rua_linear_scan.hip), identical for the four layouts.  `cumsum` is the special case a = 1.

The gate at scan position 0 is never used (forward: the gate of the FIRST token; reverse: of the LAST): a NaN or an
infinity there reaches no output and its gradient is exactly 0.  Sequences and columns are independent: a NaN stays in
its own sequence and column, at or after the position where it entered.

The gate is
  - a tensor with exactly the storage shape of `sequence.data`, or a container of the same type whose `.data` has it
    (same dtype and device as the payload); or
  - a Python float, a constant discount: passed to the kernel by value and held in the accumulator type.  No gate tensor
    is materialised or read, and it is not differentiable.
Out of scope: gates that broadcast over hidden dimensions (expand them), an initial state (fold it into x_0: x_0 + a_0 *
h_init), gradients for scalar gates.

float32 / float64 / bfloat16 / float16; bf16 and f16 accumulate in fp32, gate included, and every output is rounded
once.  The result has the container type, storage shape and dtype of the input; padding rows of an L / R result are
zeros.  ONE association order (the blocked order of the cumsum: groups of 8, tiles of 32, blocks of 2 048 positions)
whatever the layout, the kernel form or the alignment, so the operator commutes with the casts bit for bit
(z.linear_scan(a).cat() == z.cat().linear_scan(a.cat())), `reverse` is the mirrored forward scan
(z.rev().linear_scan(a.rev()).rev() == z.linear_scan(a, reverse=True)), a gate that is exactly 1 gives z.cumsum() bit for
bit, and a scalar gate equals a tensor filled with it.

LIMIT: a blocked scan forms partial gate products.  The result is finite only if the product of the gates over any
aligned group, tile or block of positions is representable in the accumulator type: gates whose running product
overflows or underflows to 0 inside a block lose what a sequential evaluation would have kept.

Autograd saves the gate and the output (not the payload); the backward is one fused kernel — the same recurrence run
the other way, grad_gate = grad_x * the neighbouring h — and second derivatives exist (composed from the scan and roll).
"""
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _ops as O
from torchrua_amd.layout import T, Z, cat_lay, install, lay_hidden, rewrap, side_payload

__all__ = ['segment_linear_scan', 'linear_scan']


def segment_linear_scan(tensor: T, gate, segment_sizes: T, reverse: bool = False) -> T:
    """The recurrence over every run of `segment_sizes` rows of `tensor` (the signature of segment_cumsum, plus the
    gate: a tensor of the shape of `tensor`, or a Python float); same shape."""
    return O.linear_scan(tensor, gate, cat_lay(tensor, segment_sizes), reverse, tuple(tensor.shape[1:]))


def linear_scan(sequence: Z, gate, reverse: bool = False) -> Z:
    """h_t = gate_t * h_(t-1) + x_t over the tokens of every sequence (h_t = gate_t * h_(t+1) + x_t with `reverse`);
    the same container type.  See the module docstring for the gate forms and the documented limit."""
    K.require_device(sequence.data)
    # the gate as a tensor (of a container: its payload; the container types must agree) or a Python number
    gate = side_payload(sequence, gate, 'linear_scan: the gate is a {got}, the sequence a {want}; cast one of them first')
    if isinstance(gate, Tensor):
        K.require_device(sequence.data, gate)
    lay, hidden = lay_hidden(sequence)
    return rewrap(sequence, O.linear_scan(sequence.data, gate, lay, reverse, hidden))


install(linear_scan=linear_scan)
