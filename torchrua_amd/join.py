"""Per-sequence join and unjoin over any container (C / L / P / R) — an extension: glue ragged batches together along
time, and cut one batch at per-sequence boundaries.

    join([z_1 ... z_k])           1 <= k <= 8 parts with the same B, dtype and hidden shape; ONE container of the
                                  parts' type.  Sequence b of the result is sequence b of z_1, then of z_2, ... in list
                                  order; its length is the sum of the parts' lengths.
    unjoin(z, [s_1 ... s_k])      the inverse and the adjoint: k containers of z's type.  s_j is an int64 [B] tensor, or
                                  a Python int (the same count for every sequence).  Part j holds the tokens
                                  [pre_j[b], pre_j[b] + s_j[b]) of every sequence, pre_j[b] = s_1[b] + ... + s_(j-1)[b].
                                  The sizes need not add up: tokens beyond the last part are dropped, and a part that
                                  would run past the end of its sequence is clamped to it.
    z.join(*others), z.unjoin(*sizes), segment_join(tensors, sizes_list), segment_unjoin(tensor, sizes, sizes_list)

Prompt + response, BOS embedding + tokens + EOS, retrieved context + query, history + new frames, the observation and
action segments of an episode.  With the reference the spelling leaves the library — a Python loop of `torch.cat` over B
pairs, or a gather through an index built with `repeat_interleave`, and a constructor again — for a CattedSequence
only: an L / R needs its padding handled by hand, a PackedSequence gets nothing (the sort order of the result follows
the SUMMED lengths and matches neither input).  The row mover cannot express it: its shift is one scalar per launch,
a join needs one per sequence.

A part of `join` may be a plain tensor [B, *hidden]: one token per sequence (a BOS / CLS embedding, a per-sequence
conditioning vector).  It needs no device work of its own — it is the LEFT layout with T = 1 and every length 1 — and
gradients flow to it.  At least one part is a container; it fixes the result type, and containers of different types
in one call are refused.  `join` of one part is a copy.

The payload moves as BITS: every dtype of element size 1 / 2 / 4 / 8 (int64 token ids and bool included), 1-D payloads
and any hidden shape, any row width and alignment; a NaN keeps its bits.  Padding rows of L / R parts are never read;
padding rows of an L / R result are zeros, written by the kernel.  Sequences may be empty in any part and in the result.

The result is defined by commutation, field by field and bit for bit: for X = left / pack / right,
`join([z_i]) == join([z_i.cat()]).X()` and `join([z_i]).cat() == join([z_i.cat()])` — for a P that covers data,
batch_sizes, sorted_indices and unsorted_indices (empty sequences exactly as `C.pack()` treats them) — and the same for
every part of `unjoin`.  `unjoin(join(parts), [lengths of the parts]) == parts`.

One HIP kernel (csrc/rua_join.hip) for both directions and the four layouts on either side.  Every token's place has a
closed form — token u of the joined sequence is token u - pre_k[b] of the part k with pre_k[b] <= u < pre_(k+1)[b] — so
there is NO per-token table: no rank, no index, no workspace.  The result's offsets and PackedSequence metadata come
from the library's existing scan / host-sort path over the new lengths, which is what makes the commutation hold.

SYNCHRONISATION: a call reads back exactly when the corresponding cast would.  `join` into a C never synchronises (the
storage is the sum of the parts' storages, the lengths are summed on the device).  An L / R / P result needs the new
lengths on the host (T', the host sort): when every part's lengths have a host copy (`C.new`, `with_host_sizes`, an
earlier read-back) they are added on the host — no read-back; otherwise ONE blocking copy brings the new lengths and
the parts' own over together, and all of them are attached, so the casts that follow read nothing.  `unjoin` sizes
its parts from their lengths, so it reads them back once for a C too unless the host can compute them (the container's
lengths have a host copy and every size is a Python int or has one); that one copy brings the container's own lengths
over as well, so a right-aligned batch with device-only lengths costs ONE read-back, not a second for its longest
sequence.  Host copies assume well-formed containers: lengths within their storages.

Autograd: `join` and `unjoin` are two Functions that are each other's backward, so derivatives of every order exist.
They hold only the length vectors and layout metadata — no payload, no index.  Gradients of padding rows and of the
tokens an `unjoin` dropped are exact zeros, whatever the payload holds there.  Integer and bool payloads pass through
without a graph.

`.split` exists on the containers with another meaning (the list of sequences); hence `unjoin`.
"""
from numbers import Integral
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.core import result_like
from torchrua_amd.layout import (NAMES, C, T, Z, cls_of, device_tensors, hidden_of, install, is_container, lay_hidden, lens_lay,
                                 lens_of, n_seq, require_container)

__all__ = ['join', 'unjoin', 'segment_join', 'segment_unjoin']

MAX_PARTS = K.JOIN_MAX_PARTS


def _same_device(tensors: Sequence[Tensor], what: str) -> None:
    devs = {str(t.device) for t in tensors}
    if len(devs) > 1:
        raise K.RuaError(f'{what}: tensors on different devices: {sorted(devs)}')


def _check_parts(sequences) -> Tuple[list, type, int, Tuple[int, ...]]:
    """The parts as a list, the result type, B and the hidden shape — after every check that needs no device."""
    if is_container(sequences) or isinstance(sequences, Tensor) or not isinstance(sequences, (list, tuple)):
        raise K.RuaError(f'join takes a list of parts; got {type(sequences).__name__} (one part is join([z]), or z.join())')
    parts = list(sequences)
    if not 1 <= len(parts) <= MAX_PARTS:
        raise K.RuaError(f'join takes 1 to {MAX_PARTS} parts; got {len(parts)}')
    for k, x in enumerate(parts):
        if not is_container(x) and not isinstance(x, Tensor):
            raise K.RuaError(f'join: part {k} is a {type(x).__name__}; a part is a container or a tensor [B, *hidden]')
    containers = [x for x in parts if is_container(x)]
    if not containers:
        raise K.RuaError('join: no container among the parts — at least one part must be a C / L / P / R; it fixes the '
                         'result type')
    cls = cls_of(containers[0])
    for x in containers:
        if cls_of(x) is not cls:
            raise K.RuaError(f'join: mixed container types in one call ({NAMES[cls]} and {NAMES[cls_of(x)]}); cast the '
                             f'parts to one type first')
    first = containers[0]
    B, hidden, dtype = n_seq(first), hidden_of(first), first.data.dtype
    for k, x in enumerate(parts):
        if isinstance(x, Tensor):
            if x.dim() < 1 or tuple(x.shape) != (B,) + hidden:
                raise K.RuaError(f'join: part {k} is a tensor of shape {tuple(x.shape)}; a tensor part holds one token '
                                 f'per sequence, shape [B, *hidden] = {(B,) + hidden}')
            data = x
        else:
            if n_seq(x) != B:
                raise K.RuaError(f'join: part {k} has {n_seq(x)} sequences, the first container has {B}: the number of '
                                 f'sequences B differs')
            if hidden_of(x) != hidden:
                raise K.RuaError(f'join: part {k} has hidden shape {hidden_of(x)}, the first container has {hidden}: the '
                                 f'hidden shape differs')
            data = x.data
        if data.dtype != dtype:
            raise K.RuaError(f'join: part {k} has dtype {data.dtype}, the first container has {dtype}: the dtype differs')
    _same_device([t for x in parts for t in device_tensors(x)], 'join')
    return parts, cls, B, hidden


def _check_sizes(sizes, B: int) -> list:
    if isinstance(sizes, (Tensor, Integral)) or not isinstance(sizes, (list, tuple)):
        raise K.RuaError(f'unjoin takes a list of sizes; got {type(sizes).__name__}')
    sizes = list(sizes)
    if not 1 <= len(sizes) <= MAX_PARTS:
        raise K.RuaError(f'unjoin takes 1 to {MAX_PARTS} sizes; got {len(sizes)}')
    for k, s in enumerate(sizes):
        if isinstance(s, Tensor):
            if s.dtype != torch.int64 or tuple(s.shape) != (B,):
                raise K.RuaError(f'unjoin: size {k} is a {s.dtype} tensor of shape {tuple(s.shape)}; sizes are int64 [B] '
                                 f'tensors (B = {B}) or non-negative ints')
        elif isinstance(s, bool) or not isinstance(s, Integral) or s < 0:
            raise K.RuaError(f'unjoin: size {k} is {s!r}; sizes are int64 [B] tensors (B = {B}) or non-negative ints')
    return sizes


def _part_lay(x, B: int, lens_only: bool = False) -> M.Lay:
    """A part's layout (lens_only: for the length launch alone, layout.lens_lay).  A tensor part [B, *hidden] is LEFT
    with T_phys = 1, no length vector, every length 1."""
    if isinstance(x, Tensor):
        return M.lay_padded(K.LEFT, None, B, 1, 1, len_add=1)
    return lens_lay(x) if lens_only else lay_hidden(x)[0]


def join(sequences: Sequence[Union[Z, T]]) -> Z:
    """The parts glued together along time, sequence by sequence; a container of the parts' type.  See the module
    docstring."""
    parts, cls, B, hidden = _check_parts(sequences)
    datas = [x if isinstance(x, Tensor) else x.data for x in parts]
    dev = K.require_device(*[t for x in parts for t in device_tensors(x)])
    lens = [None if isinstance(x, Tensor) else lens_of(x) for x in parts]
    n = None
    if all(M.host_known(v) for v in lens):
        # every part's lengths have a host copy: added on the host — no read-back for any result type
        lays = [_part_lay(x, B) for x in parts]
        sizes = O.launch_join_lens(lays, dev)[0]
        # (the device adds the lengths CLAMPED to their storages, the host the lengths as given: the same numbers for
        # well-formed containers — lengths within their storages — which is what every host mirror here assumes)
        M.attach_host(sizes, M.own_host(sum(M.host_array(v, B) for v in lens)))
    elif cls is C:
        # a C never synchronises: the storage is the sum of the parts' storages, the offsets come from the device scan
        # (a part whose storage holds more rows than its lengths add up to leaves spare rows at the end: zeros)
        lays = [_part_lay(x, B) for x in parts]
        sizes = O.launch_join_lens(lays, dev)[0]
        n = sum(int(d.size(0)) for d in datas)
    else:
        # ONE read-back: the new lengths and the parts' own, all attached — the casts that follow read nothing
        buf = O.launch_join_lens([_part_lay(x, B, lens_only=True) for x in parts], dev, want_parts=True)
        sizes = buf[0]
        M.read_back_rows(buf, [sizes] + [None if M.host_known(v) else v for v in lens])
        lays = [_part_lay(x, B) for x in parts]
    joined, shape, wrap = result_like(cls, sizes, B, hidden, datas[0], n)
    plan = O.JoinPlan(joined, lays, hidden, shape, [tuple(d.shape) for d in datas])
    return wrap(O.join(datas, plan))


def unjoin(sequence: Z, sizes: Sequence[Union[T, int]]) -> List[Z]:
    """Cut every sequence at the given sizes; one container of the same type per size.  See the module docstring."""
    cls, B, hidden = require_container(sequence, 'unjoin'), n_seq(sequence), hidden_of(sequence)
    sizes = _check_sizes(sizes, B)
    n = len(sizes)
    given = [s for s in sizes if isinstance(s, Tensor)]
    _same_device(device_tensors(sequence) + given, 'unjoin')
    dev = K.require_device(*(device_tensors(sequence) + given))
    own = lens_of(sequence)
    if M.host_known(own) and all(not isinstance(s, Tensor) or M.host_known(s) for s in sizes):
        joined, _ = lay_hidden(sequence)
        buf = O.launch_unjoin_lens(joined, sizes, dev)
        rest = np.maximum(M.host_array(own, B), 0)
        rows = []
        for s in sizes:
            want = M.host_array(s, B) if isinstance(s, Tensor) else np.full(B, int(s), dtype=np.int64)
            rows.append(np.minimum(np.maximum(want, 0), rest))
            rest = rest - rows[-1]
        part_sizes = [buf[k] for k in range(n)]   # (ONE tensor object per part: the memo lives on the object)
        M.attach_rows(M.own_host(np.stack(rows)), part_sizes)
    else:
        # the call's ONE read-back: the parts' lengths size their storages; the container's own lengths come over
        # with them and are attached, so a right-aligned batch is described (its longest sequence) without another
        buf = O.launch_unjoin_lens(lens_lay(sequence), sizes, dev, want_own=not M.host_known(own))
        part_sizes = [buf[k] for k in range(n)]
        M.read_back_rows(buf, part_sizes + [None if M.host_known(own) else own])
        joined, _ = lay_hidden(sequence)
    plans = [result_like(cls, s, B, hidden, sequence.data) for s in part_sizes]
    plan = O.JoinPlan(joined, [p[0] for p in plans], hidden, tuple(sequence.data.shape), [p[1] for p in plans])
    outs = O.unjoin(sequence.data, plan)
    return [p[2](out) for p, out in zip(plans, outs)]


def segment_join(tensors: Sequence[T], sizes_list: Sequence[T]) -> Tuple[T, T]:
    """`join` in the argument style of the `segment_*` forms: tensors[k] [N_k, *hidden] holds runs of sizes_list[k] rows
    (int64 [S]).  Returns (tensor [sum N_k, *hidden], sizes [S] int64)."""
    if not isinstance(tensors, (list, tuple)) or not isinstance(sizes_list, (list, tuple)) or len(tensors) != len(sizes_list):
        raise K.RuaError('segment_join takes a list of tensors and a list with the segment sizes of each')
    out = join([C(data=t, token_sizes=s) for t, s in zip(tensors, sizes_list)])
    return out.data, out.token_sizes


def segment_unjoin(tensor: T, segment_sizes: T, sizes_list: Sequence[Union[T, int]]) -> List[Tuple[T, T]]:
    """`unjoin` of the runs of `segment_sizes` rows of `tensor`: a list of (tensor, sizes), one per entry of sizes_list."""
    return [(c.data, c.token_sizes) for c in unjoin(C(data=tensor, token_sizes=segment_sizes), sizes_list)]


def _join_method(self: Z, *others) -> Z:
    """z.join(a, b) == join([z, a, b])."""
    return join((self,) + tuple(others))


def _unjoin_method(self: Z, *sizes) -> List[Z]:
    """z.unjoin(s1, s2) == unjoin(z, [s1, s2])."""
    return unjoin(self, list(sizes))


install(join=_join_method, unjoin=_unjoin_method)
