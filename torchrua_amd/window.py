"""Per-sequence sliding-window max / mean / sum pooling over any container (C / L / P / R) — an extension, and the first
operator that shortens a ragged batch along time BY A RULE: the new lengths are a closed form of the old ones.

    window_pool(z, kernel_size, stride=None, mode='max', ceil_mode=False)      mode: 'max' | 'mean' | 'sum'
    max_pool(z, kernel_size, stride=None, ceil_mode=False)                     window_pool(..., mode='max')
    avg_pool(z, kernel_size, stride=None, ceil_mode=False)                     window_pool(..., mode='mean')
    segment_window_pool(tensor, segment_sizes, kernel_size, stride=None, mode='max', ceil_mode=False)
                                                                               -> (tensor, new_sizes)
    z.window_pool(...), z.max_pool(...), z.avg_pool(...)

Frame subsampling in front of a Conformer or Transformer encoder, max-over-time and average pooling with a stride,
`z[::s]` (kernel_size=1), bringing frame features down to a coarser rate — the opposite direction of
`repeat_interleave`.  The stock spelling is `z.left()`, a transpose to [B, H, T], `F.max_pool1d` / `F.avg_pool1d`, a
hand-computed length formula, a transpose and a cast back: windows at a sequence's end then read the padding (a max
against fill 0 is wrong for negative data, a mean divides by the wrong count), an R needs its padding shifted by hand,
and a PackedSequence gets nothing.

SEMANTICS, the same for every layout.  With K = kernel_size (1 .. 64), S = stride (default K; 1 .. 2^31 - 1; S > K skips
tokens) and a sequence of n tokens, the number of windows is

    n <= 0:            0
    ceil_mode False:   (n - K) // S + 1  if n >= K, else 0
    ceil_mode True:    m = ceil(max(n - K, 0) / S) + 1;  m - 1 if (m - 1) * S >= n, else m

(ceil mode: a sequence shorter than K gives ONE clipped window) and window u covers the tokens [u*S, min(u*S + K, n)) —
never empty, never reaching into padding or into the next sequence.  Per column: `sum` over the window; `mean`, that sum
divided by the number of tokens actually IN the window (never by K where it is clipped); `max`, the maximum in
`argmax`'s total order on (value, position): a NaN beats every number, the first NaN or the first maximal position wins,
-0.0 == +0.0, and the output holds the winner's bits.  Wherever torch accepts the input the lengths and values are those
of `F.max_pool1d(ceil_mode=...)` / `F.avg_pool1d(ceil_mode=..., count_include_pad=False)`; torch refuses n < K, here
that case is defined as above.

float32 / float64 / bfloat16 / float16 for all three modes; int64 for `max` and `sum` (the sum wraps; no graph).  sum and
mean accumulate in fp32 (fp64 for float64), starting at the window's first token and adding the others in ascending
position; mean divides once, in the accumulator type; every output is rounded once.  ONE evaluation order per (window,
column), whatever the layout, the kernel form, the alignment or a block border, so the operator commutes with the
casts bit for bit.

The result has the container type of z and the same B and is defined by commutation, field by field and bit for bit:
`z.window_pool(...) == z.cat().window_pool(...).X()` for X = left / right / pack — a P's data, batch_sizes,
sorted_indices and unsorted_indices, an L / R's new T and zero padding — and `z.window_pool(...).cat() ==
z.cat().window_pool(...)`.  Padding rows of an L / R input are never read; a sequence may become empty, and all may.

Kernels (csrc/rua_window.hip): the pool is destination-driven — a window reads its at most K rows through
the source layout's own row formula and writes one row — and its adjoint, the spread, a source-driven gather without
atomics.  The result's offsets and PackedSequence metadata come from the library's existing scan / host-sort path over
the new lengths, which is what makes the commutation hold.

SYNCHRONISATION, `unjoin`'s policy.  When the container's lengths have a host copy (`C.new`, `with_host_sizes`, anything
an earlier read-back has touched) the formula is applied to that copy as well and attached to the new length tensor:
nothing is read back, for any container type.  Otherwise ONE blocking copy brings the new lengths and the container's own
over together, and both are attached, so the casts that follow read nothing — for a C too: the new lengths size its
storage.  Host copies assume well-formed containers: lengths within their storages.

Autograd: the pool and the spread are two Functions that are each other's backward; given its table of winners `max` is
linear (a take and a put by that table), so derivatives of every order exist.  sum and mean hold only the length vectors
and layout metadata; max keeps a uint8 table — one byte per output element, the winner's offset inside its window — and
no payload, no int64 index.  The gradient of a max window goes whole to the winning token (the first-position tie rule);
tokens in no window (the gaps of S > K, a dropped tail) and padding rows get exact zeros, whatever the payload holds.
int64 payloads pass through without a graph.

Out of scope: return_indices, padding or dilation arguments, min pooling, Lp pooling, pooling over hidden dimensions, a
no-read-back variant with a caller-given capacity, non-float mean, dtypes that merely move as bits.
"""
from numbers import Integral
from typing import Optional, Tuple

import numpy as np
import torch

from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.core import result_like
from torchrua_amd.layout import (C, T, Z, cls_of, device_tensors, hidden_of, install, lay_hidden, lens_lay, lens_of, n_seq,
                                 require_container)

__all__ = ['window_pool', 'max_pool', 'avg_pool', 'segment_window_pool', 'window_out_lens']

MAX_K = K.WINDOW_MAX_K
MAX_S = 2 ** 31 - 1


def window_out_lens(lens, kernel_size: int, stride: int, ceil_mode: bool = False) -> np.ndarray:
    """The number of windows of sequences of `lens` tokens (host integers): the closed form of the module docstring, as
    the kernel computes it."""
    n = np.maximum(np.asarray(lens, dtype=np.int64), 0)
    k, s = int(kernel_size), int(stride)
    if ceil_mode:
        m1 = (np.maximum(n - k, 0) + (s - 1)) // s                   # m - 1
        return np.where(n <= 0, 0, np.where(m1 * s >= n, m1, m1 + 1)).astype(np.int64)
    return np.where(n >= k, (n - k) // s + 1, 0).astype(np.int64)


def _window_int(value, name: str, most: int) -> int:
    if isinstance(value, bool) or not isinstance(value, Integral):
        raise K.RuaError(f'window_pool: {name} is {value!r} ({type(value).__name__}); it is an int in 1 .. {most}')
    if not 1 <= value <= most:
        raise K.RuaError(f'window_pool: {name} is {value}; it is an int in 1 .. {most}')
    return int(value)


def _check_args(sequence, kernel_size, stride, mode) -> Tuple[int, int, int]:
    """(K, S, mode code) after every check that needs no device — each refusal names the offending value."""
    require_container(sequence, 'window_pool')
    if not isinstance(mode, str) or mode not in O.WINDOW_MODES:
        raise K.RuaError(f'window_pool: mode is {mode!r}; it is one of {sorted(O.WINDOW_MODES)}')
    k = _window_int(kernel_size, 'kernel_size', MAX_K)
    s = k if stride is None else _window_int(stride, 'stride', MAX_S)
    dtype = sequence.data.dtype
    if dtype not in K.SCAN_DTYPES:
        raise K.RuaError(f'window_pool supports {list(K.SCAN_DTYPES)}; got {dtype}')
    if dtype == torch.int64 and mode == 'mean':
        raise K.RuaError(f"window_pool: mode 'mean' of a {dtype} payload is refused (max and sum take int64)")
    return k, s, O.WINDOW_MODES[mode]


def window_pool(sequence: Z, kernel_size: int, stride: Optional[int] = None, mode: str = 'max',
                ceil_mode: bool = False) -> Z:
    """Every sequence pooled over windows of `kernel_size` tokens every `stride` tokens; a container of the same type
    with the new lengths.  See the module docstring."""
    k, s, code = _check_args(sequence, kernel_size, stride, mode)
    dev = K.require_device(*device_tensors(sequence))
    cls, B, hidden = cls_of(sequence), n_seq(sequence), hidden_of(sequence)
    own = lens_of(sequence)
    if M.host_known(own):
        # the lengths have a host copy: the formula is applied to it as well — no read-back for any container type
        big, _ = lay_hidden(sequence)
        sizes = O.launch_window_lens(big, k, s, ceil_mode, dev)[0]
        M.attach_host(sizes, M.own_host(window_out_lens(M.host_array(own, B), k, s, ceil_mode)))
    else:
        # ONE read-back: the new lengths and the container's own, both attached — the casts that follow read nothing
        buf = O.launch_window_lens(lens_lay(sequence), k, s, ceil_mode, dev, want_own=True)
        sizes = buf[0]
        M.read_back_rows(buf, [sizes, own])
        big, _ = lay_hidden(sequence)
    small, shape, wrap = result_like(cls, sizes, B, hidden, sequence.data)
    plan = O.WindowPlan(small, big, hidden, shape, tuple(sequence.data.shape), k, s)
    return wrap(O.window_pool(sequence.data, plan, code))


def max_pool(sequence: Z, kernel_size: int, stride: Optional[int] = None, ceil_mode: bool = False) -> Z:
    """window_pool(..., mode='max')."""
    return window_pool(sequence, kernel_size, stride, 'max', ceil_mode)


def avg_pool(sequence: Z, kernel_size: int, stride: Optional[int] = None, ceil_mode: bool = False) -> Z:
    """window_pool(..., mode='mean'): every window divided by the number of tokens in it."""
    return window_pool(sequence, kernel_size, stride, 'mean', ceil_mode)


def segment_window_pool(tensor: T, segment_sizes: T, kernel_size: int, stride: Optional[int] = None, mode: str = 'max',
                        ceil_mode: bool = False) -> Tuple[T, T]:
    """`window_pool` of the runs of `segment_sizes` rows of `tensor` [N, *hidden]: (tensor [N', *hidden], new_sizes [S]
    int64)."""
    if not isinstance(tensor, torch.Tensor) or not isinstance(segment_sizes, torch.Tensor):
        raise K.RuaError(f'segment_window_pool takes a tensor and its segment sizes; got {type(tensor).__name__} and '
                         f'{type(segment_sizes).__name__}')
    out = window_pool(C(data=tensor, token_sizes=segment_sizes), kernel_size, stride, mode, ceil_mode)
    return out.data, out.token_sizes


install(window_pool=window_pool, max_pool=max_pool, avg_pool=avg_pool)
