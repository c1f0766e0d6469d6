"""Kernel launches with autograd: the row mover and the segmented reduce.

Backward of a move is the adjoint move (layouts swapped, token map inverted, zero fill for rows
nothing maps to) — the same kernel.  Backward of a segmented reduce is one fused kernel
(rua_segment_reduce_backward), which also serves scatter_* through the bucket indirection.
"""
import ctypes
import threading
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from torchrua_amd import _lib as L
from torchrua_amd import _meta as M

# optional hook bench.py installs to bracket named kernels with HIP events on the launch stream
_kernel_hook: Optional[Callable[[str, bool], None]] = None


def set_kernel_hook(fn) -> None:
    global _kernel_hook
    _kernel_hook = fn


def _prod(shape) -> int:
    n = 1
    for d in shape:
        n *= d
    return n


def _plain(t: Tensor) -> Tensor:
    """`t` without its graph (no copy)."""
    return t.detach() if t.requires_grad else t


def _acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def _require_dtype(data: Tensor, table, what: str) -> int:
    """The ABI code of the payload's dtype; a host tensor is refused first, then a dtype outside `table`."""
    L.require_device(data)
    if data.dtype not in table:
        raise L.RuaError(f'{what} {list(table)}; got {data.dtype}')
    return table[data.dtype]


def _call(name: str, symbol: str, dev, *args) -> None:
    """One named launch: the kernel hook opens, the entry point `symbol` runs on torch's current stream of `dev` (its
    last argument, L.stream_ptr: evaluated right before the call) and is checked, the hook closes."""
    if _kernel_hook:
        _kernel_hook(name, True)
    L.check(getattr(L.load(), symbol)(*args, L.stream_ptr(dev)), symbol)
    if _kernel_hook:
        _kernel_hook(name, False)


_LIKE_PAYLOAD = ' target must be contiguous, of the payload dtype and of the payload shape'


def _target(out: Optional[Tensor], like_shape, dtype: torch.dtype, dev, what: str) -> Tensor:
    """`out`, or a new tensor where the caller gave none; `what` is the message that refuses an unfit one."""
    if out is None:
        return torch.empty(tuple(like_shape), dtype=dtype, device=dev)
    if not out.is_contiguous() or out.dtype != dtype or tuple(out.shape) != tuple(like_shape):
        raise L.RuaError(what)
    return out


def _workspace(ws_bytes_fn: str, lay: 'M.Lay', H: Optional[int], code: Optional[int], dev, cut: bool = True,
               taps: Optional[int] = None) -> Optional[Tensor]:
    """What the cut form of a per-sequence operator needs (> 0 bytes: few but long sequences get cut), or None.
    `taps`: the size function also takes a filter length (the causal conv's backward sums).  H is None: it takes the
    layout alone (the compress plan counts a mask: no row width, no dtype)."""
    args = (lay.ref(), H, code) if taps is None else (lay.ref(), H, taps, code)
    if H is None:
        args = (lay.ref(),)
    nbytes = getattr(L.load(), ws_bytes_fn)(*args) if cut else 0
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None


_fill_cache = {}


def _fill16(value, dtype: torch.dtype) -> bytes:
    """The fill element replicated to 16 bytes (as the kernel's uint4 pattern); memoised per (value, dtype)."""
    key = (value, dtype) if isinstance(value, (int, float, bool, bytes)) else None
    hit = _fill_cache.get(key) if key is not None else None
    if hit is not None:
        return hit
    raw = value if isinstance(value, bytes) else torch.tensor([value], dtype=dtype).view(torch.uint8).numpy().tobytes()
    if len(raw) > 16:
        raise L.RuaError(f'fill element wider than 16 bytes ({dtype})')
    out = (raw * (16 // len(raw)))[:16]
    if key is not None and len(_fill_cache) < 256:
        _fill_cache[key] = out
    return out


class MovePlan:
    """Everything one rua_move_rows launch needs except the payload pointers."""
    __slots__ = ('dst', 'src', 'tmap', 'arg', 'out_shape', 'fill', 'pad_row', 'flags', 'name')

    def __init__(self, dst: M.Lay, src: M.Lay, out_shape: Sequence[int], tmap: int = L.T_SHIFT, arg: int = 0,
                 fill=0, pad_row: int = -1, flags: int = 0, name: str = 'move'):
        self.dst, self.src, self.tmap, self.arg = dst, src, tmap, arg
        self.out_shape, self.fill, self.pad_row, self.flags, self.name = tuple(out_shape), fill, pad_row, flags, name

    def adjoint(self, src_shape: Sequence[int]) -> 'MovePlan':
        inv = {L.T_SHIFT: (L.T_SHIFT, -self.arg), L.T_ROLL: (L.T_ROLL, -self.arg), L.T_REV_S: (L.T_REV_D, 0),
               L.T_REV_D: (L.T_REV_S, 0)}
        if self.tmap not in inv or self.dst.kind == L.LIST or self.flags:
            raise L.RuaError('this move has no adjoint move')
        tmap, arg = inv[self.tmap]
        return MovePlan(self.src, self.dst, src_shape, tmap, arg, fill=0, name=self.name + '_bwd')


def launch_move(plan: MovePlan, src_data: Tensor, out: Optional[Tensor] = None) -> Tensor:
    dev = L.require_device(src_data)
    src_data = src_data.contiguous()
    if out is None:
        out = torch.empty(plan.out_shape, dtype=src_data.dtype, device=dev)
    elif not out.is_contiguous() or out.dtype != src_data.dtype:
        raise L.RuaError('move target must be contiguous and of the payload dtype')
    # rows are equally wide on both sides; size them on the side the layout `dst` enumerates
    enumerated = src_data if (plan.flags & L.MOVE_SCATTER) else out
    rb = (enumerated.numel() // plan.dst.n_rows) * enumerated.element_size() if plan.dst.n_rows else 0
    fill = _fill16(plan.fill, src_data.dtype)
    _call(plan.name, 'rua_move_rows', dev, plan.dst.ref(), plan.src.ref(), plan.tmap, plan.arg, L.ptr(out),
          L.ptr(src_data), rb, fill, plan.pad_row, plan.flags)
    return out


class _Move(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src_data: Tensor, plan: MovePlan):
        ctx.plan = plan
        ctx.src_shape = tuple(src_data.shape)
        return launch_move(plan, src_data)

    @staticmethod
    def backward(ctx, grad: Tensor):
        return _Move.apply(grad.contiguous(), ctx.plan.adjoint(ctx.src_shape)), None


def move(src_data: Tensor, plan: MovePlan) -> Tensor:
    if src_data.requires_grad and torch.is_grad_enabled():
        return _Move.apply(src_data, plan)
    return launch_move(plan, _plain(src_data))


class _ListGather(torch.autograd.Function):
    """X[batch_ptr, token_ptr] (core/get.py tuple keys): rows may repeat, so the adjoint accumulates."""

    @staticmethod
    def forward(ctx, src_data: Tensor, plan: MovePlan, flat_fn, lead: int = 1):
        ctx.flat_fn = flat_fn
        ctx.src_shape = tuple(src_data.shape)
        ctx.lead = lead                 # leading dims of src_data that enumerate storage rows (2 for [B, T, *H])
        return launch_move(plan, src_data)

    @staticmethod
    def backward(ctx, grad: Tensor):
        """d/d src = the rows of `grad` summed into the storage rows they were gathered from.  Rows may repeat, so this
        is a scatter-sum: bucket the flat row numbers (stable radix sort, rua_index_buckets) and fold every bucket in
        ascending entry order with the segmented reducer — no float atomics, bitwise reproducible (torch's index_add_
        is neither).  [r4] Twice differentiable, like the reference's `data[key]`: the scatter-sum's own adjoint is the
        gather again (_ScatterSumRows / _GatherRows)."""
        flat = ctx.flat_fn().reshape(-1)
        grad = grad.contiguous()
        hidden = tuple(ctx.src_shape[ctx.lead:])
        n_rows = _prod(ctx.src_shape[:ctx.lead])
        flat = torch.where(flat < 0, flat + n_rows, flat)          # negative rows wrapped in the forward (like torch)
        g = scatter_sum(grad.reshape((flat.numel(),) + hidden), flat, n_rows)
        return g.reshape(ctx.src_shape), None, None, None


# ------------------------------------------------------------------ reductions
# max / min / logsumexp track the reference's global `initial` through a small scratch (rua.h: `extreme`).  One
# persistent, zeroed scratch per (device, stream): the reduce needs no initialising launch (RUA_OP_SCRATCH_CLEAN) and
# rua_fill_empty hands it back zeroed — stream order makes that safe for one stream, hence the key.
_scratch = {}
# the reduce and its trailing rua_fill_empty share the scratch and must reach the stream back to back: ctypes drops the
# GIL around each call, so a second host thread enqueueing on the SAME stream could slip its own reduce in between
_scratch_pair = threading.Lock()


def extreme_scratch(dev) -> Tuple[Tensor, int]:
    key = (dev.index, torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if dev.index is None else dev.index))
    if torch.cuda.is_current_stream_capturing():
        # inside a graph capture ALWAYS a buffer of the capture's own (zeroed by the legacy initialising launch), even
        # when this stream already has a persistent one: a graph that baked the shared scratch in could be replayed on
        # another stream while eager max / min runs on this one, and the two would race on its flag and ticket words
        return torch.empty(L.EXTREME_WORDS, dtype=torch.long, device=dev), 0
    buf = _scratch.get(key)
    if buf is None:
        buf = _scratch[key] = torch.zeros(L.EXTREME_WORDS, dtype=torch.long, device=dev)
    return buf, L.OP_SCRATCH_CLEAN


def forget_extreme_scratch(dev) -> None:
    for key in [k for k in _scratch if k[0] == dev.index]:
        del _scratch[key]


_EMPTY = {L.SUM: 0.0, L.MEAN: 0.0, L.PROD: 1.0, L.MAX: 0.0, L.MIN: 0.0, L.LOGSUMEXP: float('-inf')}


def _bits(value: float, dtype: torch.dtype) -> int:
    raw = _fill16(value, dtype)[:dtype.itemsize]
    return int.from_bytes(raw, 'little')


def split_workspace(lay: M.Lay, H: int, dtype: torch.dtype, dev, team_ok: bool = True,
                    tail_ok: bool = True) -> Tuple[int, Optional[Tensor]]:
    """(split_rows, workspace) for the reducer's long-sequence splitting (0, None when it is off)."""
    split = M.reduce_split_rows(lay, H * dtype.itemsize, team_ok, tail_ok)
    if not split:
        return 0, None
    nbytes = L.load().rua_reduce_ws_bytes(lay.n_rows, H, L.DTYPES[dtype], split)
    return split, torch.empty(nbytes, dtype=torch.uint8, device=dev)


def int_split_workspace(n_rows: int, H: int, dtype: torch.dtype, dev) -> Tuple[int, Optional[Tensor]]:
    """(split_rows, workspace) of the INTEGER reducer's long-bucket split (rua_reduce_int.hip).  Always armed from a few
    thousand rows on: the bucket sizes live on the device, a skewed histogram is the ordinary case, and when no bucket
    is long the machinery costs two launches of at most ~1 024 waves that find nothing to do."""
    if n_rows < 4096:
        return 0, None
    # about a thousand parts, but no part beyond ~2 MB of payload: a part is ONE wave's walk (profiles/r04_skew.txt)
    split = max(1024, min(n_rows // 1024, (2 << 20) // max(1, H * dtype.itemsize)))
    nbytes = L.load().rua_reduce_ws_bytes(n_rows, H, L.INT_DTYPES[dtype], split)
    return split, torch.empty(nbytes, dtype=torch.uint8, device=dev)


def short_seqs_hint(lay: M.Lay, row_bytes: int) -> int:
    """RUA_OP_SHORT_SEQS for a reduce over a CattedSequence whose lengths the host knows and none of which is far above
    the average (at most 8 x, or 64 rows).  One wave (= one workgroup) per sequence is bound by the workgroup dispatch
    rate when the sequences are short (4 M singletons: 3 ms at any row width; 500 000 sequences of 16 rows: 0.4 ms where
    the payload takes 0.06) and by a chain of dependent loads per sequence when the rows are narrow; with the hint the
    launcher gives every row slot of a wave a sequence of its own up to 16 .. 64 rows on average by row width
    (profiles/r04_cat_ranks_ab.txt).  The wave walks to the longest of its sequences, hence the bound — and no hint at
    all when the lengths live on the device only.  (Four sequences per wave at rows of <= 32 bytes need no hint: that
    form checks its own lengths, wave by wave — and so, since round 5, does every-row-slot-its-own-sequence when the hint
    is withheld: the hint only saves the waves that check.)"""
    if lay.kind != L.CAT or lay.max_len is None or lay.B <= 0 or not 0 < row_bytes <= 512:
        return 0
    avg = lay.n_rows / lay.B
    return L.OP_SHORT_SEQS if lay.max_len <= max(64, 8 * avg) else 0


def launch_reduce(lay: M.Lay, data: Tensor, op: int, out: Optional[Tensor] = None, include_self: int = 0,
                  perm: Optional[Tensor] = None, hidden: Tuple[int, ...] = (), reference_initial: bool = True,
                  name: str = 'reduce', ties_out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_reduce (+ rua_fill_empty for the reference's global-extreme `initial`)."""
    code = _require_dtype(data, L.DTYPES, 'reductions support')
    dev = data.device
    data = data.contiguous()
    H = _prod(hidden)
    out = _target(out, (lay.B,) + tuple(hidden), data.dtype, dev,
                  'reduce target must be a contiguous [B, *hidden] tensor of the payload dtype')
    extreme, op_bits = None, 0
    if reference_initial and op in (L.MAX, L.MIN, L.LOGSUMEXP) and include_self == 0:
        extreme, op_bits = extreme_scratch(dev)
    tail_ok = include_self != 1 and (data.data_ptr() | out.data_ptr()) % 8 == 0      # the launcher's own condition
    split, ws = split_workspace(lay, H, data.dtype, dev, tail_ok=tail_ok)
    short = short_seqs_hint(lay, H * data.dtype.itemsize) if perm is None and not split else 0
    # (the reduce leaves the global extreme in the scratch — every wave folds the opposite extreme of the rows it reads —
    # so the trailing rua_fill_empty needs no second walk: every workgroup patches its share of the batch, whether or
    # not the host knows how many sequences are empty)
    paired = extreme is not None
    if paired:
        _scratch_pair.acquire()
    try:
        _call(name, 'rua_segment_reduce', dev, lay.ref(), L.ptr(perm), L.ptr(data), L.ptr(out), H, code,
              op | op_bits | short | (L.OP_NO_EMPTY if extreme is not None and lay.no_empty else 0), include_self,
              _bits(_EMPTY[op], data.dtype), L.ptr(extreme), split, L.ptr(ws), L.ptr(ties_out))
        if extreme is not None:               # (outside the hook's bracket: the name times the reduce alone)
            L.check(L.load().rua_fill_empty(lay.ref(), L.ptr(out), H, code, op | (op_bits & L.OP_SCRATCH_CLEAN),
                                            L.ptr(extreme), L.stream_ptr(dev)), 'rua_fill_empty')
    except L.RuaError:
        forget_extreme_scratch(dev)        # a refused launch may have left the flags raised
        raise
    finally:
        if paired:
            _scratch_pair.release()
    return out


class _Reduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, op: int, hidden, lens: Optional[Tensor]):
        ties = None
        if op in (L.MAX, L.MIN):
            # the forward counts, per output element, the elements equal to it (free in the pass that reads the payload
            # anyway): the backward is then ONE walk instead of a counting walk plus an applying walk
            ties = torch.empty((lay.B,) + tuple(hidden), dtype=_acc_dtype(data.dtype), device=data.device)
        out = launch_reduce(lay, data, op, hidden=hidden, ties_out=ties)
        ctx.lay, ctx.op, ctx.lens, ctx.ties = lay, op, lens, ties
        ctx.save_for_backward(data, out)      # (reduce() hands a contiguous payload: the saved tensor IS the input)
        return out

    @staticmethod
    def backward(ctx, grad: Tensor):
        data, out = ctx.saved_tensors
        if torch.is_grad_enabled() and ctx.op in (L.MAX, L.MIN, L.LOGSUMEXP):
            # [r5] a graph of this backward is being recorded (create_graph=True).  The reference's reductions are ATen
            # compositions and differentiate any number of times (reduce.py:34-61: torch.segment_reduce; logsumexp = detached
            # max, exp, segment sum, log); the fused kernel's output carries no graph, so HERE the gradient is spelled with
            # differentiable pieces: the per-sequence broadcast (the backward of sum, whose own adjoint is the reduction)
            # and torch's elementwise ops — [N, H] temporaries, paid only by callers who ask for second derivatives
            return _composed_reduce_grad(grad, data, out, ctx.lay, ctx.op, ctx.ties), None, None, None, None
        return _ReduceBwd.apply(grad, data, out, ctx.lay, ctx.op, ctx.ties), None, None, None, None


def _composed_reduce_grad(grad: Tensor, data: Tensor, out: Tensor, lay: M.Lay, op: int, ties: Optional[Tensor]) -> Tensor:
    """d reduce / d data as a differentiable function of (grad, data, out): max / min / logsumexp under create_graph."""
    spread, live = _spread_live(data, lay, out.shape[1:], want_live=op == L.LOGSUMEXP)
    if op == L.LOGSUMEXP:
        # padding rows of a padded layout may hold anything (inf, NaN, 1e9): exp(pad - 0) would turn their zero into
        # NaN, so the exponent is taken on live rows only (0 elsewhere — its gradient there is then exactly 0 as well)
        return spread(grad) * torch.where(live, data - spread(out), torch.zeros_like(data)).exp()
    o = spread(out.detach())
    x = data.detach()
    hit = (x == o) | ((x != x) & (o != o))
    g32 = grad.to(ties.dtype)
    share = torch.where(g32 > 0, g32 / ties.clamp_min(1), g32).to(grad.dtype)     # torch.segment_reduce's tie rule
    return spread(share) * hit


def _spread_live(ref: Tensor, lay: M.Lay, hidden, want_live: bool = True):
    """What the composed (twice differentiable) gradients share: spread(v) lays every sequence's row of a [B, *hidden]
    `v` over the sequence's storage rows (the backward of the per-sequence sum: differentiable, its adjoint is the sum),
    and `live` is the mask of the storage rows of `ref` that hold a token."""
    ref = ref.detach()

    def spread(v: Tensor) -> Tensor:
        return _ReduceBwd.apply(v.contiguous(), ref, v.detach(), lay, L.SUM, None)

    if not want_live:
        return spread, None
    return spread, spread(torch.ones((lay.B,) + tuple(hidden), dtype=ref.dtype, device=ref.device)) != 0


class _ReduceBwd(torch.autograd.Function):
    """The backward of a segmented reduce as a function of the cotangent.  One fused kernel
    (rua_segment_reduce_backward): reads the payload once (max/min: the forward already counted the ties), writes the
    gradient once — no [N, H] temporaries.  [r4] For SUM and MEAN the map cotangent -> gradient is linear (a broadcast
    of every segment's row over the segment's rows, divided by the length for MEAN) and its adjoint is the reduction
    itself, so these two are differentiable any number of times, like the reference's (torch.segment_reduce,
    reduce.py:44-49).  [r5] max / min / logsumexp: under create_graph=True _Reduce.backward composes the gradient from
    differentiable pieces instead of calling this kernel (_composed_reduce_grad), so they are twice differentiable too;
    prod differentiates once (the reference's does not: a stated gap)."""

    @staticmethod
    def forward(ctx, grad: Tensor, data: Tensor, out: Tensor, lay: M.Lay, op: int, ties: Optional[Tensor]):
        dev = L.require_device(data)
        lib = L.load()
        grad = grad.contiguous()
        g = torch.empty(data.shape, dtype=data.dtype, device=dev)   # padding rows: zeroed by the call (BWD_FILL_PADDING)
        H = _prod(out.shape[1:])
        split, ws = split_workspace(lay, H, data.dtype, dev, team_ok=False)      # (the backward walk has no wave teams)
        # max/min: `ties` counted by the forward -> apply only (TIES_FINAL).  segment_max/min are torch.segment_reduce in
        # the reference (reduce.py:34-41), whose backward lets tied extrema share a positive gradient and hands each of
        # them a non-positive one whole (BWD_TIES_POSITIVE)
        L.check(lib.rua_segment_reduce_backward(lay.ref(), None, L.ptr(data), L.ptr(out), L.ptr(grad), L.ptr(g), H,
                                                L.DTYPES[data.dtype], op,
                                                (L.TIES_FINAL if ties is not None else 0) | L.BWD_FILL_PADDING | L.BWD_TIES_POSITIVE,
                                                split, L.ptr(ws), L.ptr(ties), None, L.stream_ptr(dev)),
                'rua_segment_reduce_backward')
        ctx.lay, ctx.op, ctx.hidden = lay, op, tuple(out.shape[1:])
        return g

    @staticmethod
    def backward(ctx, gg: Tensor):
        if ctx.op not in (L.SUM, L.MEAN):
            raise RuntimeError('torchrua_amd: prod (and the fused max / min / logsumexp kernel outside create_graph) '
                               'differentiate once; second-order gradients exist for sum, mean, max, min and logsumexp '
                               '(and for every cast, select and gather)')
        return reduce(gg.contiguous(), ctx.lay, ctx.op, ctx.hidden, None), None, None, None, None, None


def reduce(data: Tensor, lay: M.Lay, op: int, hidden, lens: Optional[Tensor]) -> Tensor:
    if data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, inside the graph: the Function saves its own input, so a second derivative (create_graph)
        # reaches d/d data through it — a copy made inside forward() would carry no history
        return _Reduce.apply(data.contiguous(), lay, op, tuple(hidden), lens)
    return launch_reduce(lay, _plain(data), op, hidden=tuple(hidden))


# ------------------------------------------------------------------ pack() that keeps the sums of its one pass
# pack(keep_sums=...) runs the fused pack + sum (rua_pack_sums): the PackedSequence AND the fp32 per-sequence sums in one
# pass over the payload.  The sums ride on the returned payload tensor (the per-tensor memo, keyed by its version), and
# reduce_sum(p) rounds them to the payload dtype (rua_sums_cast) instead of reading the payload a third time.
SUMS_DTYPES = (torch.float32, torch.bfloat16, torch.float16)      # payloads the fused kernel accumulates in fp32
_SUMS_KEY = 'pack_sums'


def pack_sums_can(data: Tensor, hidden: Tuple[int, ...]) -> bool:
    """Can rua_pack_sums take this payload?  (Its own conditions: anything else is packed by the mover, without sums.)"""
    return (data.dtype in SUMS_DTYPES and data.is_contiguous() and data.data_ptr() % 16 == 0 and data.numel() > 0
            and (_prod(hidden) * data.element_size()) % 16 == 0)


def launch_pack_sums(data: Tensor, src: M.Lay, dst: M.Lay, hidden: Tuple[int, ...]) -> Tuple[Tensor, Tensor]:
    dev = data.device
    H = _prod(hidden)
    pdata = torch.empty((dst.n_rows,) + tuple(hidden), dtype=data.dtype, device=dev)
    sums = torch.empty((src.B,) + tuple(hidden), dtype=torch.float32, device=dev)
    split, ws = split_workspace(src, H, data.dtype, dev, team_ok=False)      # (the fused kernel has no wave teams)
    _call('to_pack', 'rua_pack_sums', dev, src.ref(), dst.ref(), L.ptr(data), L.ptr(pdata), L.ptr(sums), H,
          L.DTYPES[data.dtype], split, L.ptr(ws))
    return pdata, sums


def launch_sums_cast(x: Tensor, dtype: torch.dtype, to_f32: bool, name: Optional[str] = None) -> Tensor:
    """fp32 [B, *H] -> `dtype` (rounded as the reducer rounds its accumulators), or `dtype` -> fp32: a fresh tensor."""
    dev = L.require_device(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32 if to_f32 else dtype, device=dev)
    args = (L.ptr(x), L.ptr(out), x.numel(), L.DTYPES[dtype], 1 if to_f32 else 0)
    if name is None:
        L.check(L.load().rua_sums_cast(*args, L.stream_ptr(dev)), 'rua_sums_cast')
    else:
        _call(name, 'rua_sums_cast', dev, *args)
    return out


class _SumsCast(torch.autograd.Function):
    """The kept fp32 sums as reduce_sum's output; its adjoint widens the cotangent back (exact)."""

    @staticmethod
    def forward(ctx, sums: Tensor, dtype: torch.dtype):
        ctx.dtype = dtype
        return launch_sums_cast(sums, dtype, False, name='reduce')

    @staticmethod
    def backward(ctx, grad: Tensor):
        if torch.is_grad_enabled():          # create_graph: torch's own cast carries the graph on
            return grad.to(torch.float32), None
        return launch_sums_cast(grad, ctx.dtype, True), None


class _PackSums(torch.autograd.Function):
    """(payload of the PackedSequence, fp32 sums) = rua_pack_sums(source).  The adjoint takes whichever cotangents
    arrive: the payload's alone is the adjoint move P -> source; the sums' alone is the reduce's backward over the SOURCE
    layout (a broadcast of every sequence's row over its rows: one write of the payload); both at once are ONE kernel
    (rua_pack_sums_backward: one read, one write).  Under create_graph the same is spelled with the differentiable
    two-op pieces (_Move, _ReduceBwd): the fused kernels differentiate once."""

    @staticmethod
    def forward(ctx, data: Tensor, src: M.Lay, dst: M.Lay, hidden: Tuple[int, ...]):
        ctx.src, ctx.dst, ctx.hidden, ctx.shape, ctx.dtype = src, dst, tuple(hidden), tuple(data.shape), data.dtype
        ctx.set_materialize_grads(False)
        return launch_pack_sums(data, src, dst, hidden)

    @staticmethod
    def backward(ctx, g_pack: Optional[Tensor], g_sums: Optional[Tensor]):
        if g_pack is None and g_sums is None:
            return None, None, None, None
        src, dst, hidden = ctx.src, ctx.dst, ctx.hidden
        to_src = MovePlan(src, dst, ctx.shape, name='to_pack_bwd')
        if torch.is_grad_enabled():
            g = None
            if g_pack is not None:
                g = _Move.apply(g_pack.contiguous(), to_src)
            if g_sums is not None:
                gs = g_sums.to(ctx.dtype).contiguous()
                # (sum reads neither x nor out: `ref` only carries the source's shape and dtype — one element, expanded)
                ref = torch.empty((1,) * len(ctx.shape), dtype=ctx.dtype, device=gs.device).expand(ctx.shape)
                spread = _ReduceBwd.apply(gs, ref, gs.detach(), src, L.SUM, None)
                g = spread if g is None else g + spread
            return g, None, None, None
        if g_sums is None:
            return launch_move(to_src, g_pack), None, None, None
        dev = g_sums.device
        g_sums = g_sums.contiguous()
        H = _prod(hidden)
        if g_pack is not None:
            g_pack = g_pack.contiguous()
            if (H * g_pack.element_size()) % 16 == 0 and (g_pack.data_ptr() | g_sums.data_ptr()) % 16 == 0:
                g = torch.empty(ctx.shape, dtype=ctx.dtype, device=dev)
                L.check(L.load().rua_pack_sums_backward(src.ref(), dst.ref(), L.ptr(g_pack), L.ptr(g_sums), L.ptr(g), H,
                                                        L.DTYPES[ctx.dtype], L.stream_ptr(dev)), 'rua_pack_sums_backward')
                return g, None, None, None
        # the sums' cotangent alone: its rows in the payload dtype, spread over the source rows by the reduce's backward
        gs = g_sums if ctx.dtype == torch.float32 else launch_sums_cast(g_sums, ctx.dtype, False)
        g = torch.empty(ctx.shape, dtype=ctx.dtype, device=dev)
        split, ws = split_workspace(src, H, ctx.dtype, dev, team_ok=False)
        # (sum reads neither x nor out: both stand-ins are the read-only cotangent, never the buffer being written)
        L.check(L.load().rua_segment_reduce_backward(src.ref(), None, L.ptr(gs), L.ptr(gs), L.ptr(gs), L.ptr(g), H,
                                                     L.DTYPES[ctx.dtype], L.SUM, L.BWD_FILL_PADDING, split, L.ptr(ws),
                                                     None, None, L.stream_ptr(dev)), 'rua_segment_reduce_backward')
        if g_pack is not None:        # (rows off 16 bytes cannot get here: the forward would not have run)
            g += launch_move(to_src, g_pack)
        return g, None, None, None


def pack_sums(data: Tensor, src: M.Lay, dst: M.Lay, hidden: Tuple[int, ...]) -> Tuple[Tensor, Tensor]:
    """(payload of the PackedSequence `dst`, fp32 [B, *hidden] sums) of the source `src`, recorded by autograd."""
    if data.requires_grad and torch.is_grad_enabled():
        return _PackSums.apply(data, src, dst, tuple(hidden))
    return launch_pack_sums(_plain(data), src, dst, tuple(hidden))


def keep_sums(p, sums: Tensor) -> None:
    """Record `sums` as the per-sequence sums of the PackedSequence `p` whose payload this pass just wrote: on the payload
    tensor, under its version (an in-place write invalidates them), with the metadata objects they belong to."""
    M._memo_put(p.data, _SUMS_KEY, (sums, p.batch_sizes, p.sorted_indices, p.unsorted_indices))


def kept_sums(p) -> Optional[Tensor]:
    """The fp32 sums pack() left on this very PackedSequence — same payload tensor at the same version, same
    batch_sizes / index tensors — or None (a sliced, re-built or foreign PackedSequence; a payload written since)."""
    hit = M._memo_get(p.data, _SUMS_KEY)
    if hit is None or hit[1] is not p.batch_sizes or hit[2] is not p.sorted_indices or hit[3] is not p.unsorted_indices:
        return None
    return hit[0]


def reduce_kept_sums(sums: Tensor, dtype: torch.dtype) -> Tensor:
    """reduce_sum from the kept sums: ONE small launch (fp32 [B, H] -> dtype), a fresh tensor every call."""
    if sums.requires_grad and torch.is_grad_enabled():
        return _SumsCast.apply(sums, dtype)
    return launch_sums_cast(_plain(sums), dtype, False, name='reduce')


# ------------------------------------------------------------------ per-sequence softmax / log_softmax (an extension)
_SOFTMAX_SUPPORT = 'softmax / log_softmax support'


def launch_softmax(lay: M.Lay, data: Tensor, log: bool, hidden: Tuple[int, ...], out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_softmax: one launch (two for cut sequences), no [N, H] temporary.  `out` may be `data` itself."""
    code = _require_dtype(data, L.DTYPES, _SOFTMAX_SUPPORT)
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_softmax_ws_bytes', lay, H, code, dev)
    data = data.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'softmax' + _LIKE_PAYLOAD)      # padding rows: zeroed by the call
    _call('log_softmax' if log else 'softmax', 'rua_segment_softmax', dev, lay.ref(), L.ptr(data), L.ptr(out), H, code,
          int(bool(log)), L.ptr(ws))
    return out


def launch_softmax_backward(lay: M.Lay, y: Tensor, grad: Tensor, log: bool, hidden: Tuple[int, ...],
                            out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_softmax_backward: the gradient from the forward's output alone.  `out` may be `grad` itself."""
    code = _require_dtype(y, L.DTYPES, _SOFTMAX_SUPPORT)
    dev, H = y.device, _prod(hidden)
    ws = _workspace('rua_softmax_ws_bytes', lay, H, code, dev)
    L.require_device(grad)
    if grad.dtype != y.dtype or grad.shape != y.shape:
        raise L.RuaError('softmax backward: the cotangent must have the dtype and shape of the output')
    y, grad = y.contiguous(), grad.contiguous()
    out = _target(out, y.shape, y.dtype, dev, 'softmax backward' + _LIKE_PAYLOAD)
    _call('log_softmax_bwd' if log else 'softmax_bwd', 'rua_segment_softmax_backward', dev, lay.ref(), L.ptr(y),
          L.ptr(grad), L.ptr(out), H, code, int(bool(log)), L.ptr(ws))
    return out


class _Softmax(torch.autograd.Function):
    """y = softmax / log_softmax of every sequence.  Saves ONLY y; the backward is one fused kernel."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, log: bool, hidden):
        y = launch_softmax(lay, data, log, hidden)
        ctx.lay, ctx.log, ctx.hidden = lay, log, tuple(hidden)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad: Tensor):
        y, = ctx.saved_tensors
        if torch.is_grad_enabled():
            # a graph of this backward is being recorded (create_graph=True): the gradient spelled with the library's
            # differentiable pieces — the per-sequence sum (twice differentiable) and its broadcast — as
            # _composed_reduce_grad does; [N, H] temporaries, paid only by callers who ask for second derivatives
            return _composed_softmax_grad(grad, y, ctx.lay, ctx.log, ctx.hidden), None, None, None
        return launch_softmax_backward(ctx.lay, y, grad, ctx.log, ctx.hidden), None, None, None


def _composed_softmax_grad(grad: Tensor, y: Tensor, lay: M.Lay, log: bool, hidden) -> Tensor:
    """d softmax / d data as a differentiable function of (grad, y)."""
    spread, live = _spread_live(y, lay, hidden)
    zero = torch.zeros_like(y)
    # padding rows of a padded layout: y is 0 there, but the cotangent may hold anything (inf, NaN) and exp(0) is 1 —
    # both variants are evaluated on live rows only and are exactly 0 elsewhere (the mask comes BEFORE the exp)
    g = torch.where(live, grad, zero)
    if log:
        e = torch.where(live, y, zero).exp()
        return torch.where(live, g - e * spread(reduce(g.contiguous(), lay, L.SUM, hidden, None)), zero)
    return torch.where(live, y * (g - spread(reduce((g * y).contiguous(), lay, L.SUM, hidden, None))), zero)


def softmax(data: Tensor, lay: M.Lay, log: bool, hidden) -> Tensor:
    _require_dtype(data, L.DTYPES, _SOFTMAX_SUPPORT)
    if data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, inside the graph (as in reduce()): a copy made inside forward() would carry no history
        return _Softmax.apply(data.contiguous(), lay, bool(log), tuple(hidden))
    return launch_softmax(lay, _plain(data), bool(log), tuple(hidden))


# ------------------------------------------------------------------ per-sequence softmax-weighted sum (an extension)
def _pool_check(values: Tensor, scores: Tensor) -> torch.device:
    dev = L.require_device(values, scores)
    _require_dtype(values, L.DTYPES, 'softmax_pool supports')
    if scores.dtype != values.dtype:
        raise L.RuaError(f'softmax_pool: the scores have dtype {scores.dtype}, the values {values.dtype}')
    if scores.device != values.device:
        raise L.RuaError('softmax_pool: scores and values live on different devices')
    return dev


def launch_softmax_pool(lay: M.Lay, values: Tensor, scores: Tensor, hidden: Tuple[int, ...], G: int,
                        out_acc: bool = False) -> Tuple[Tensor, Tensor]:
    """rua_segment_softmax_pool: (out [B, *hidden], lse [B, G] in the accumulator type) in one launch; the values are
    read once, no [N, H] temporary exists.  out_acc: `out` comes unrounded, in the accumulator type (RUA_POOL_OUT_ACC) —
    what autograd keeps for a bf16 / f16 payload."""
    dev = _pool_check(values, scores)
    H = _prod(hidden)
    D = H // G if G else 1
    values, scores = values.contiguous(), scores.contiguous()
    acc = _acc_dtype(values.dtype)
    out_dtype = acc if out_acc else values.dtype
    if lay.B == 0 or lay.n_rows == 0 or H == 0:
        # (the entry point returns without a launch: every sequence is empty)
        return (torch.zeros((lay.B,) + tuple(hidden), dtype=out_dtype, device=dev),
                torch.full((lay.B, G), float('-inf'), dtype=acc, device=dev))
    out = torch.empty((lay.B,) + tuple(hidden), dtype=out_dtype, device=dev)
    lse = torch.empty((lay.B, G), dtype=acc, device=dev)
    _call('softmax_pool', 'rua_segment_softmax_pool', dev, lay.ref(), L.ptr(values), L.ptr(scores), L.ptr(out),
          L.ptr(lse), H, D, L.DTYPES[values.dtype] | (L.POOL_OUT_ACC if out_acc else 0), None)
    return out, lse


def launch_softmax_pool_backward(lay: M.Lay, grad: Tensor, values: Tensor, scores: Tensor, out: Tensor, lse: Tensor,
                                 hidden: Tuple[int, ...], G: int, want_values: bool = True,
                                 want_scores: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """rua_segment_softmax_pool_backward: (grad_values or None, grad_scores or None) in one launch, from the inputs, the
    [B, H] output (in the payload dtype, or unrounded in the accumulator type) and the [B, G] lse.  Padding rows of both
    are zeros."""
    dev = _pool_check(values, scores)
    L.require_device(grad, out, lse)
    out_acc = out.dtype != values.dtype
    if out.dtype not in (values.dtype, _acc_dtype(values.dtype)) or not out.is_contiguous() or not lse.is_contiguous():
        raise L.RuaError('softmax_pool backward: `out` is the contiguous forward output, in the payload or accumulator dtype')
    if grad.dtype != values.dtype or grad.shape != out.shape:
        raise L.RuaError('softmax_pool backward: the cotangent must have the dtype and shape of the output')
    H = _prod(hidden)
    D = H // G if G else 1
    grad, values, scores = grad.contiguous(), values.contiguous(), scores.contiguous()
    if lay.B == 0 or lay.n_rows == 0 or H == 0:
        # (no launch, as in the forward: nothing depends on either input, so both gradients are zeros)
        return (torch.zeros(values.shape, dtype=values.dtype, device=dev) if want_values else None,
                torch.zeros(scores.shape, dtype=scores.dtype, device=dev) if want_scores else None)
    gv = torch.empty(values.shape, dtype=values.dtype, device=dev) if want_values else None
    gs = torch.empty(scores.shape, dtype=scores.dtype, device=dev) if want_scores else None
    _call('softmax_pool_bwd', 'rua_segment_softmax_pool_backward', dev, lay.ref(), L.ptr(grad), L.ptr(values),
          L.ptr(scores), L.ptr(out), L.ptr(lse), L.ptr(gv), L.ptr(gs), H, D,
          L.DTYPES[values.dtype] | (L.POOL_OUT_ACC if out_acc else 0), None)
    return gv, gs


class _SoftmaxPool(torch.autograd.Function):
    """out[b] = sum_t softmax_t(scores[b])[t] * values[b, t].  Saves the two inputs, the [B, H] output and the [B, G]
    lse — nothing else of [N, H] size; the backward is one fused kernel and differentiates once.  For a bf16 / f16
    payload the kernel hands the output unrounded (fp32): that is what is saved — the backward subtracts sum(out * g)
    from a per-token dot, and a rounded `out` would put 2^-9 of it into grad_scores — and the result is its one rounding."""

    @staticmethod
    def forward(ctx, values: Tensor, scores: Tensor, lay: M.Lay, hidden, G: int):
        half = values.dtype in (torch.bfloat16, torch.float16)
        kept, lse = launch_softmax_pool(lay, values, scores, hidden, G, out_acc=half)
        out = kept.to(values.dtype) if half else kept
        ctx.lay, ctx.hidden, ctx.G = lay, tuple(hidden), G
        ctx.save_for_backward(values, scores, kept, lse)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad: Tensor):
        values, scores, out, lse = ctx.saved_tensors
        gv, gs = launch_softmax_pool_backward(ctx.lay, grad, values, scores, out, lse, ctx.hidden, ctx.G,
                                              ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gv, gs, None, None, None


def softmax_pool(values: Tensor, scores: Tensor, lay: M.Lay, hidden, G: int) -> Tensor:
    _pool_check(values, scores)
    if torch.is_grad_enabled() and (values.requires_grad or scores.requires_grad):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _SoftmaxPool.apply(values.contiguous(), scores.contiguous(), lay, tuple(hidden), int(G))
    return launch_softmax_pool(lay, _plain(values), _plain(scores), tuple(hidden), int(G))[0]


# ------------------------------------------------------------------ per-sequence var_mean / standardize (an extension)
_NORM_SUPPORT = 'var_mean / standardize support'


def _norm_args(lay: M.Lay, data: Tensor, hidden, correction, eps=0.0, cut: bool = True):
    code = _require_dtype(data, L.DTYPES, _NORM_SUPPORT)
    if isinstance(correction, bool) or not isinstance(correction, int) or correction < 0:
        raise L.RuaError(f'var_mean / standardize: correction is a non-negative integer; got {correction!r}')
    if not float(eps) >= 0.0:
        raise L.RuaError(f'standardize: eps is a non-negative float; got {eps!r}')
    H = _prod(hidden)
    return data.device, code, H, _workspace('rua_norm_ws_bytes', lay, H, code, data.device, cut)


def launch_var_mean(lay: M.Lay, data: Tensor, hidden: Tuple[int, ...], correction: int = 1, want_var: bool = True,
                    want_mean: bool = True, mean_acc: bool = False) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """rua_segment_var_mean: (var, mean), each [B, *hidden] of the payload dtype, from ONE read of the payload.
    mean_acc: `mean` comes unrounded, in the accumulator type (RUA_NORM_MEAN_ACC) — what autograd keeps for bf16 / f16."""
    dev, code, H, ws = _norm_args(lay, data, hidden, correction)
    data = data.contiguous()
    shape = (lay.B,) + tuple(hidden)
    mean_dtype = _acc_dtype(data.dtype) if mean_acc else data.dtype
    if lay.B == 0 or lay.n_rows == 0 or H == 0:
        # (the entry point returns without a launch: every sequence is empty)
        return (torch.full(shape, float('nan'), dtype=data.dtype, device=dev) if want_var else None,
                torch.full(shape, float('nan'), dtype=mean_dtype, device=dev) if want_mean else None)
    var = torch.empty(shape, dtype=data.dtype, device=dev) if want_var else None
    mean = torch.empty(shape, dtype=mean_dtype, device=dev) if want_mean else None
    _call('var_mean', 'rua_segment_var_mean', dev, lay.ref(), L.ptr(data), L.ptr(var), L.ptr(mean), H,
          code | (L.NORM_MEAN_ACC if mean_acc else 0), correction, L.ptr(ws))
    return var, mean


def launch_var_mean_backward(lay: M.Lay, data: Tensor, mean: Tensor, grad_var: Optional[Tensor],
                             grad_mean: Optional[Tensor], hidden: Tuple[int, ...], correction: int = 1,
                             out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_var_mean_backward: one token-parallel launch; `mean` in the payload or the accumulator dtype."""
    dev, code, H, _ = _norm_args(lay, data, hidden, correction, cut=False)
    L.require_device(mean, grad_var, grad_mean)
    mean_acc = mean.dtype != data.dtype
    shape = (lay.B,) + tuple(hidden)
    if mean.dtype not in (data.dtype, _acc_dtype(data.dtype)) or tuple(mean.shape) != shape:
        raise L.RuaError('var_mean backward: `mean` is the forward\'s [B, *hidden], in the payload or accumulator dtype')
    for g in (grad_var, grad_mean):
        if g is not None and (g.dtype != data.dtype or tuple(g.shape) != shape):
            raise L.RuaError('var_mean backward: a cotangent must have the dtype and shape of its output')
    data, mean = data.contiguous(), mean.contiguous()
    grad_var = None if grad_var is None else grad_var.contiguous()
    grad_mean = None if grad_mean is None else grad_mean.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'var_mean backward' + _LIKE_PAYLOAD)     # padding rows: zeroed by the call
    _call('var_mean_bwd', 'rua_segment_var_mean_backward', dev, lay.ref(), L.ptr(data), L.ptr(mean), L.ptr(grad_var),
          L.ptr(grad_mean), L.ptr(out), H, code | (L.NORM_MEAN_ACC if mean_acc else 0), correction)
    return out


def launch_standardize(lay: M.Lay, data: Tensor, hidden: Tuple[int, ...], eps: float = 1e-5, correction: int = 0,
                       out: Optional[Tensor] = None, want_rstd: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """rua_segment_standardize: (y, rstd [B, *hidden] in the accumulator type or None); one launch (two for cut
    sequences), no [N, H] temporary.  `out` may be `data` itself."""
    dev, code, H, ws = _norm_args(lay, data, hidden, correction, eps)
    data = data.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'standardize' + _LIKE_PAYLOAD)      # padding rows: zeroed by the call
    rstd = None
    if want_rstd:
        shape, acc = (lay.B,) + tuple(hidden), _acc_dtype(data.dtype)
        if lay.B == 0 or lay.n_rows == 0 or H == 0:                      # (no launch then: every sequence is empty)
            rstd = torch.full(shape, float('nan'), dtype=acc, device=dev)
        else:
            rstd = torch.empty(shape, dtype=acc, device=dev)
    _call('standardize', 'rua_segment_standardize', dev, lay.ref(), L.ptr(data), L.ptr(out), L.ptr(rstd), H, code,
          correction, float(eps), L.ptr(ws))
    return out, rstd


def launch_standardize_backward(lay: M.Lay, y: Tensor, rstd: Tensor, grad: Tensor, hidden: Tuple[int, ...],
                                correction: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_standardize_backward: the gradient from the forward's output and rstd alone.  `out` may be `grad`."""
    dev, code, H, ws = _norm_args(lay, y, hidden, correction)
    L.require_device(grad, rstd)
    if grad.dtype != y.dtype or grad.shape != y.shape:
        raise L.RuaError('standardize backward: the cotangent must have the dtype and shape of the output')
    if rstd.dtype != _acc_dtype(y.dtype) or tuple(rstd.shape) != (lay.B,) + tuple(hidden):
        raise L.RuaError('standardize backward: `rstd` is the forward\'s [B, *hidden] in the accumulator dtype')
    y, grad, rstd = y.contiguous(), grad.contiguous(), rstd.contiguous()
    out = _target(out, y.shape, y.dtype, dev, 'standardize backward' + _LIKE_PAYLOAD)
    _call('standardize_bwd', 'rua_segment_standardize_backward', dev, lay.ref(), L.ptr(y), L.ptr(rstd), L.ptr(grad),
          L.ptr(out), H, code, correction, L.ptr(ws))
    return out


def _norm_pieces(ref: Tensor, lay: M.Lay, hidden, correction: int):
    """_spread_live, and the [B, *hidden] counts n and n - c (NaN where n - c <= 0, as the kernels give)."""
    spread, live = _spread_live(ref, lay, hidden)
    n = launch_reduce(lay, live.to(ref.dtype), L.SUM, hidden=tuple(hidden), reference_initial=False)
    dof = n - correction
    dof = torch.where(dof > 0, dof, torch.full_like(dof, float('nan')))
    return spread, live, n, dof


class _Standardize(torch.autograd.Function):
    """(y, rstd) = standardize of every sequence.  Saves ONLY y and the [B, H] rstd — both outputs of this node, so a
    recorded backward (create_graph=True) differentiates through them; the caller keeps y alone."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, hidden, eps: float, correction: int):
        y, rstd = launch_standardize(lay, data, hidden, eps, correction, want_rstd=True)
        ctx.lay, ctx.hidden, ctx.correction = lay, tuple(hidden), correction
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y, rstd)
        return y, rstd

    @staticmethod
    def backward(ctx, grad: Optional[Tensor], grad_rstd: Optional[Tensor]):
        y, rstd = ctx.saved_tensors
        if grad is None and grad_rstd is None:
            return None, None, None, None, None
        if torch.is_grad_enabled() or grad_rstd is not None or grad is None:
            # a graph of this backward is being recorded (create_graph=True), or rstd itself carries a cotangent (it
            # only does inside such a graph): the gradient spelled with the library's differentiable pieces, as
            # _composed_softmax_grad does; [N, H] temporaries, paid only by callers who ask for second derivatives
            return _composed_standardize_grad(grad, grad_rstd, y, rstd, ctx.lay, ctx.hidden, ctx.correction), None, None, None, None
        return launch_standardize_backward(ctx.lay, y, rstd, grad, ctx.hidden, ctx.correction), None, None, None, None


def _composed_standardize_grad(grad: Optional[Tensor], grad_rstd: Optional[Tensor], y: Tensor, rstd: Tensor, lay: M.Lay,
                               hidden, correction: int) -> Tensor:
    """d standardize / d data as a differentiable function of (grad, grad_rstd, y, rstd):
    rstd * (g - mean_t g - y * sum_t(g y) / (n - c))  -  y * grad_rstd * rstd^2 / (n - c)."""
    spread, live, n, dof = _norm_pieces(y, lay, hidden, correction)
    zero = torch.zeros_like(y)
    r = rstd.to(y.dtype)
    yl = torch.where(live, y, zero)
    total = zero
    if grad is not None:
        # padding rows of a padded layout: the cotangent may hold anything (inf, NaN) — masked BEFORE it is used
        g = torch.where(live, grad, zero)
        s1 = reduce(g.contiguous(), lay, L.SUM, hidden, None) / n
        s2 = reduce((g * yl).contiguous(), lay, L.SUM, hidden, None) / dof
        total = total + spread(r) * (g - spread(s1) - yl * spread(s2))
    if grad_rstd is not None:
        total = total - yl * spread(grad_rstd.to(y.dtype) * r * r / dof)
    return torch.where(live, total, zero)


class _VarMean(torch.autograd.Function):
    """(var, mean) of every sequence.  Saves the input and the [B, H] mean — for a bf16 / f16 payload the unrounded fp32
    mean the kernel hands out (x - mean is a difference; the result is its one rounding)."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, hidden, correction: int):
        half = data.dtype in (torch.bfloat16, torch.float16)
        var, kept = launch_var_mean(lay, data, hidden, correction, mean_acc=half)
        mean = kept.to(data.dtype) if half else kept
        ctx.lay, ctx.hidden, ctx.correction = lay, tuple(hidden), correction
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(data, kept)
        return var, mean

    @staticmethod
    def backward(ctx, grad_var: Optional[Tensor], grad_mean: Optional[Tensor]):
        data, mean = ctx.saved_tensors
        if grad_var is None and grad_mean is None:
            return None, None, None, None
        if torch.is_grad_enabled():
            return _composed_var_mean_grad(grad_var, grad_mean, data, ctx.lay, ctx.hidden, ctx.correction), None, None, None
        return launch_var_mean_backward(ctx.lay, data, mean, grad_var, grad_mean, ctx.hidden, ctx.correction), None, None, None


def _composed_var_mean_grad(grad_var: Optional[Tensor], grad_mean: Optional[Tensor], data: Tensor, lay: M.Lay, hidden,
                            correction: int) -> Tensor:
    """d var_mean / d data as a differentiable function of (grad_var, grad_mean, data); the mean is recomputed with the
    library's (twice differentiable) reduce_mean."""
    spread, live, n, dof = _norm_pieces(data, lay, hidden, correction)
    zero = torch.zeros_like(data)
    total = zero
    if grad_var is not None:
        mean = reduce(data, lay, L.MEAN, hidden, None)
        dev = torch.where(live, data - spread(mean), zero)      # (padding rows may hold anything)
        total = total + spread(grad_var * 2 / dof) * dev
    if grad_mean is not None:
        total = total + spread(grad_mean / n)
    return torch.where(live, total, zero)


def var_mean(data: Tensor, lay: M.Lay, hidden, correction: int = 1, want_var: bool = True,
             want_mean: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    _require_dtype(data, L.DTYPES, _NORM_SUPPORT)
    if data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, inside the graph (as in reduce()): a copy made inside forward() would carry no history
        return _VarMean.apply(data.contiguous(), lay, tuple(hidden), correction)
    return launch_var_mean(lay, _plain(data), tuple(hidden), correction, want_var=want_var, want_mean=want_mean)


def standardize(data: Tensor, lay: M.Lay, hidden, eps: float = 1e-5, correction: int = 0) -> Tensor:
    _require_dtype(data, L.DTYPES, _NORM_SUPPORT)
    if data.requires_grad and torch.is_grad_enabled():
        return _Standardize.apply(data.contiguous(), lay, tuple(hidden), float(eps), correction)[0]
    return launch_standardize(lay, _plain(data), tuple(hidden), eps, correction)[0]


# ------------------------------------------------------------------ per-sequence cumsum (an extension)
def launch_cumsum(lay: M.Lay, data: Tensor, reverse: bool, hidden: Tuple[int, ...], out: Optional[Tensor] = None,
                  cut: bool = True) -> Tensor:
    """rua_segment_cumsum: one launch (two for cut sequences), one read and one write of the payload.  `out` may be
    `data` itself.  cut=False withholds the workspace (the same bits from one workgroup per unit: a developer A/B)."""
    code = _require_dtype(data, L.SCAN_DTYPES, 'cumsum supports')
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_cumsum_ws_bytes', lay, H, code, dev, cut)
    data = data.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'cumsum' + _LIKE_PAYLOAD)      # padding rows: zeroed by the call
    _call('cumsum_rev' if reverse else 'cumsum', 'rua_segment_cumsum', dev, lay.ref(), L.ptr(data), L.ptr(out), H, code,
          int(bool(reverse)), L.ptr(ws))
    return out


class _Cumsum(torch.autograd.Function):
    """y = the inclusive prefix sums of every sequence.  Saves NOTHING: the map is linear and the adjoint of the forward
    scan is the reverse scan, so the backward is this Function with `reverse` flipped — any order of derivative."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, reverse: bool, hidden):
        ctx.lay, ctx.reverse, ctx.hidden = lay, reverse, tuple(hidden)
        return launch_cumsum(lay, data, reverse, hidden)

    @staticmethod
    def backward(ctx, grad: Tensor):
        return cumsum(grad, ctx.lay, not ctx.reverse, ctx.hidden), None, None, None


def cumsum(data: Tensor, lay: M.Lay, reverse: bool, hidden) -> Tensor:
    _require_dtype(data, L.SCAN_DTYPES, 'cumsum supports')
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _Cumsum.apply(data.contiguous(), lay, bool(reverse), tuple(hidden))
    return launch_cumsum(lay, _plain(data), bool(reverse), tuple(hidden))


# ------------------------------------------------------------------ per-sequence cummax / cummin / logcumsumexp (extensions)
_CUMEXT_SUPPORT = 'cummax / cummin support'
_LCSE_SUPPORT = 'logcumsumexp supports'


def launch_cumextreme(lay: M.Lay, data: Tensor, op: int, reverse: bool, hidden: Tuple[int, ...],
                      want_values: bool = True, want_indices: bool = True,
                      cut: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """rua_segment_cumextreme: (values or None, indices or None), both of the payload's storage shape — one launch (two
    for cut sequences), one read of the payload.  cut=False withholds the workspace (the same bits: a developer A/B)."""
    code = _require_dtype(data, L.SCAN_DTYPES, _CUMEXT_SUPPORT)
    if op not in (L.MAX, L.MIN):
        raise L.RuaError('cumextreme: the operator is MAX or MIN')
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_cumextreme_ws_bytes', lay, H, code, dev, cut)
    data = data.contiguous()
    values = torch.empty(data.shape, dtype=data.dtype, device=dev) if want_values else None      # padding rows: zeroed
    indices = torch.empty(data.shape, dtype=torch.int64, device=dev) if want_indices else None   # by the call
    name = ('cummax' if op == L.MAX else 'cummin') + ('_rev' if reverse else '')
    _call(name, 'rua_segment_cumextreme', dev, lay.ref(), L.ptr(data), L.ptr(values), L.ptr(indices), H, code, op,
          int(bool(reverse)), L.ptr(ws))
    return values, indices


def _cum_indices(grad: Tensor, indices: Tensor, what: str) -> Tensor:
    L.require_device(grad, indices)
    if indices.dtype != torch.int64 or indices.shape != grad.shape:
        raise L.RuaError(f'{what}: the indices are an int64 tensor of the storage shape of the cotangent')
    return _plain(indices).contiguous()


def launch_cumextreme_backward(lay: M.Lay, grad: Tensor, indices: Tensor, reverse: bool, hidden: Tuple[int, ...],
                               cut: bool = True) -> Tensor:
    """rua_segment_cumextreme_backward: the run sums of `grad` at the run heads of `indices` — the adjoint of the
    gather by `indices`; zeros elsewhere and in padding rows."""
    code = _require_dtype(grad, L.DTYPES, _CUMEXT_SUPPORT + ' (gradients)')
    indices = _cum_indices(grad, indices, 'cummax / cummin backward')
    dev, H = grad.device, _prod(hidden)
    ws = _workspace('rua_cumextreme_ws_bytes', lay, H, code, dev, cut)
    grad = grad.contiguous()
    out = torch.empty(grad.shape, dtype=grad.dtype, device=dev)
    _call('cumextreme_rev_bwd' if reverse else 'cumextreme_bwd', 'rua_segment_cumextreme_backward', dev, lay.ref(),
          L.ptr(grad), L.ptr(indices), L.ptr(out), H, code, int(bool(reverse)), L.ptr(ws))
    return out


class _CumRunSum(torch.autograd.Function):
    """grad -> its run sums at the run heads of `indices` (rua_segment_cumextreme_backward).  Linear; its adjoint is
    the gather by the same indices (_CumGather), whose adjoint is this again: derivatives of every order exist.  Saves
    ONLY the indices."""

    @staticmethod
    def forward(ctx, grad: Tensor, indices: Tensor, lay: M.Lay, reverse: bool, hidden):
        ctx.args = (lay, bool(reverse), tuple(hidden))
        ctx.save_for_backward(indices)
        return launch_cumextreme_backward(lay, grad, indices, reverse, hidden)

    @staticmethod
    def backward(ctx, grad: Tensor):
        indices, = ctx.saved_tensors
        lay, reverse, hidden = ctx.args
        return cum_gather(grad, indices, lay, reverse, hidden), None, None, None, None


class _CumGather(torch.autograd.Function):
    """payload -> out[b, t, h] = payload[b, indices[b, t, h], h]: the per-element gather of rua_segment_reorder, which
    takes repeated positions (its scatter does not: this never routes through _Reorder).  Saves ONLY the indices."""

    @staticmethod
    def forward(ctx, data: Tensor, indices: Tensor, lay: M.Lay, reverse: bool, hidden):
        ctx.args = (lay, bool(reverse), tuple(hidden))
        ctx.save_for_backward(indices)
        return launch_reorder(lay, data, indices, hidden, per_row=False, inverse=False)

    @staticmethod
    def backward(ctx, grad: Tensor):
        indices, = ctx.saved_tensors
        lay, reverse, hidden = ctx.args
        return cum_run_sum(grad, indices, lay, reverse, hidden), None, None, None, None


def cum_run_sum(grad: Tensor, indices: Tensor, lay: M.Lay, reverse: bool, hidden) -> Tensor:
    if _wants_grad(grad):
        return _CumRunSum.apply(grad.contiguous(), indices, lay, bool(reverse), tuple(hidden))
    return launch_cumextreme_backward(lay, _plain(grad), indices, bool(reverse), tuple(hidden))


def cum_gather(data: Tensor, indices: Tensor, lay: M.Lay, reverse: bool, hidden) -> Tensor:
    if _wants_grad(data):
        return _CumGather.apply(data.contiguous(), indices, lay, bool(reverse), tuple(hidden))
    return launch_reorder(lay, _plain(data), indices, tuple(hidden), per_row=False, inverse=False)


class _CumExtreme(torch.autograd.Function):
    """(values, indices) = the running max / min of every sequence.  Saves ONLY the indices; the backward is the run
    sum of the cotangent (cum_run_sum), itself differentiable."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, op: int, reverse: bool, hidden):
        values, indices = launch_cumextreme(lay, data, op, reverse, hidden)
        ctx.args = (lay, bool(reverse), tuple(hidden))
        ctx.save_for_backward(indices)
        ctx.mark_non_differentiable(indices)
        return values, indices

    @staticmethod
    def backward(ctx, grad: Tensor, _grad_indices):
        indices, = ctx.saved_tensors
        lay, reverse, hidden = ctx.args
        return cum_run_sum(grad, indices, lay, reverse, hidden), None, None, None, None


def cumextreme(data: Tensor, lay: M.Lay, op: int, reverse: bool, hidden) -> Tuple[Tensor, Tensor]:
    _require_dtype(data, L.SCAN_DTYPES, _CUMEXT_SUPPORT)
    if _wants_grad(data):
        # contiguous HERE, before the Function (as in cumsum()): a copy made inside forward() would carry no history
        return _CumExtreme.apply(data.contiguous(), lay, op, bool(reverse), tuple(hidden))
    return launch_cumextreme(lay, _plain(data), op, bool(reverse), tuple(hidden))


def launch_logcumsumexp(lay: M.Lay, data: Tensor, reverse: bool, hidden: Tuple[int, ...], cut: bool = True) -> Tensor:
    """rua_segment_logcumsumexp: one launch (two for cut sequences), one read and one write of the payload."""
    code = _require_dtype(data, L.DTYPES, _LCSE_SUPPORT)
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_logcumsumexp_ws_bytes', lay, H, code, dev, cut)
    data = data.contiguous()
    out = torch.empty(data.shape, dtype=data.dtype, device=dev)      # padding rows: zeroed by the call
    _call('logcumsumexp_rev' if reverse else 'logcumsumexp', 'rua_segment_logcumsumexp', dev, lay.ref(), L.ptr(data),
          L.ptr(out), H, code, int(bool(reverse)), L.ptr(ws))
    return out


def launch_logcumsumexp_backward(lay: M.Lay, grad: Tensor, data: Tensor, out: Tensor, reverse: bool,
                                 hidden: Tuple[int, ...], cut: bool = True) -> Tensor:
    """rua_segment_logcumsumexp_backward: grad_in[s] = sum over t >= s (scan order) of grad[t] * exp(x[s] - y[t])."""
    code = _require_dtype(grad, L.DTYPES, _LCSE_SUPPORT)
    L.require_device(grad, data, out)
    if not (grad.dtype == data.dtype == out.dtype) or not (grad.shape == data.shape == out.shape):
        raise L.RuaError('logcumsumexp backward: cotangent, input and output share one dtype and one storage shape')
    dev, H = grad.device, _prod(hidden)
    ws = _workspace('rua_logcumsumexp_ws_bytes', lay, H, code, dev, cut)
    grad, data, out = grad.contiguous(), data.contiguous(), out.contiguous()
    gx = torch.empty(grad.shape, dtype=grad.dtype, device=dev)
    _call('logcumsumexp_rev_bwd' if reverse else 'logcumsumexp_bwd', 'rua_segment_logcumsumexp_backward', dev, lay.ref(),
          L.ptr(grad), L.ptr(data), L.ptr(out), L.ptr(gx), H, code, int(bool(reverse)), L.ptr(ws))
    return gx


class _LogCumSumExp(torch.autograd.Function):
    """y = logcumsumexp of every sequence.  Saves the input and the output; the backward is one fused kernel (the same
    weighted log-space scan run the other way).  Second derivatives are out of scope."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, reverse: bool, hidden):
        out = launch_logcumsumexp(lay, data, reverse, hidden)
        ctx.args = (lay, bool(reverse), tuple(hidden))
        ctx.save_for_backward(data, out)
        return out

    @staticmethod
    def backward(ctx, grad: Tensor):
        if torch.is_grad_enabled():
            raise L.RuaError('logcumsumexp: second derivatives (create_graph=True) are out of scope')
        data, out = ctx.saved_tensors
        lay, reverse, hidden = ctx.args
        return launch_logcumsumexp_backward(lay, grad, data, out, reverse, hidden), None, None, None


def logcumsumexp(data: Tensor, lay: M.Lay, reverse: bool, hidden) -> Tensor:
    _require_dtype(data, L.DTYPES, _LCSE_SUPPORT)
    if data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, before the Function (as in cumsum()): a copy made inside forward() would carry no history
        return _LogCumSumExp.apply(data.contiguous(), lay, bool(reverse), tuple(hidden))
    return launch_logcumsumexp(lay, _plain(data), bool(reverse), tuple(hidden))


# ------------------------------------------------------------------ per-sequence linear-chain CRF (an extension)
_CRF_SUPPORT = 'crf: the emissions are one of'


def crf_args(what: str, data: Tensor, hidden: Tuple[int, ...], transitions, start, end,
             before_device: Optional[Callable[[], None]] = None) -> int:
    """K, after the checks that come before any launch, each naming its argument: a float payload with exactly one hidden
    dimension of 1 <= K <= CRF_MAX_TAGS; `transitions` [K, K], `start` / `end` [K] or None, all of the payload's dtype
    and device; and last (so that every other refusal can be met without a GPU) the payload on a HIP device."""
    if data.dtype not in L.DTYPES:
        raise L.RuaError(f'{what}: the emissions are one of {list(L.DTYPES)}; got {data.dtype}')
    if len(hidden) != 1:
        raise L.RuaError(f'{what}: the emissions have exactly ONE hidden dimension (the K tags); got hidden dimensions '
                         f'{tuple(hidden)}')
    K = int(hidden[0])
    if not 1 <= K <= L.CRF_MAX_TAGS:
        raise L.RuaError(f'{what}: the emissions have K = {K} tags; 1 <= K <= {L.CRF_MAX_TAGS}')
    for name, t, shape in (('transitions', transitions, (K, K)), ('start', start, (K,)), ('end', end, (K,))):
        if t is None and name != 'transitions':
            continue
        if not isinstance(t, Tensor):
            raise L.RuaError(f'{what}: `{name}` is a tensor of shape {shape}; got {type(t).__name__}')
        if tuple(t.shape) != shape:
            raise L.RuaError(f'{what}: `{name}` has shape {tuple(t.shape)}; with K = {K} tags it must be {shape}')
        if t.dtype != data.dtype:
            raise L.RuaError(f'{what}: `{name}` has dtype {t.dtype}, the emissions {data.dtype}')
        if t.device != data.device:
            raise L.RuaError(f'{what}: `{name}` lives on {t.device}, the emissions on {data.device}')
    if before_device is not None:
        before_device()
    if not data.is_cuda:
        raise L.RuaError(f'{what}: the emissions live on {data.device}; move them to a HIP device (there is no CPU '
                         f'fallback by design)')
    return K


def _crf_small(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else _plain(t).contiguous()


def launch_crf_forward(lay: M.Lay, data: Tensor, transitions: Tensor, start: Optional[Tensor], end: Optional[Tensor],
                       K: int, viterbi: bool = False, want_alpha: bool = False):
    """rua_segment_crf_forward: ONE launch.  (out [B], alpha [*storage, K] or None, backptr or None, last or None), the
    per-sequence results and alpha in the accumulator type.  B == 0: empty results without a launch."""
    code = _require_dtype(data, L.DTYPES, _CRF_SUPPORT)
    dev, acc = data.device, _acc_dtype(data.dtype)
    data, transitions, start, end = data.contiguous(), _crf_small(transitions), _crf_small(start), _crf_small(end)
    out = torch.empty(lay.B, dtype=acc, device=dev)
    alpha = torch.empty(data.shape, dtype=acc, device=dev) if want_alpha and not viterbi else None
    backptr = torch.empty(data.shape, dtype=torch.uint8, device=dev) if viterbi else None
    last = torch.empty(lay.B, dtype=torch.int64, device=dev) if viterbi else None
    if lay.B:
        _call('crf_viterbi' if viterbi else 'crf_partition', 'rua_segment_crf_forward', dev, lay.ref(), L.ptr(data),
              L.ptr(transitions), L.ptr(start), L.ptr(end), L.ptr(alpha), L.ptr(backptr), L.ptr(out), L.ptr(last), K, code,
              L.CRF_MAX if viterbi else L.CRF_LOG)
    return out, alpha, backptr, last


def launch_crf_backtrace(lay: M.Lay, backptr: Tensor, last: Tensor, lead_shape: Sequence[int], K: int) -> Tensor:
    """rua_segment_crf_backtrace: a launch of its own on the same stream; the int64 tags, one per row of the storage."""
    dev = backptr.device
    tags = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)       # padding rows: zeroed by the call
    if lay.B and tags.numel():
        _call('crf_backtrace', 'rua_segment_crf_backtrace', dev, lay.ref(), L.ptr(backptr), L.ptr(last), L.ptr(tags), K)
    return tags


def launch_crf_backward(lay: M.Lay, grad: Tensor, data: Tensor, transitions: Tensor, end: Optional[Tensor], alpha: Tensor,
                        logz: Tensor, K: int, want_emissions: bool = True, want_transitions: bool = True,
                        want_start: bool = True, want_end: bool = True):
    """rua_segment_crf_backward: (grad_emissions, grad_transitions, grad_start, grad_end), None where not wanted — one
    walk, plus the finish launch when one of the parameter sums is wanted."""
    code = _require_dtype(data, L.DTYPES, _CRF_SUPPORT)
    dev, acc = data.device, _acc_dtype(data.dtype)
    L.require_device(grad, data, transitions, end, alpha, logz)
    if grad.dtype != acc or tuple(grad.shape) != (lay.B,):
        raise L.RuaError(f'crf backward: the cotangent of logZ is a {acc} tensor of shape ({lay.B},)')
    params = want_transitions or want_start or want_end
    # (no sequence: the entry point returns without a launch, and an empty sum is 0)
    small = torch.zeros if lay.B == 0 else torch.empty
    gx = torch.empty(data.shape, dtype=data.dtype, device=dev) if want_emissions else None
    gt = small((K, K), dtype=data.dtype, device=dev) if want_transitions else None
    gs = small((K,), dtype=data.dtype, device=dev) if want_start else None
    ge = small((K,), dtype=data.dtype, device=dev) if want_end else None
    if lay.B and (want_emissions or params):
        nbytes = L.load().rua_crf_ws_bytes(lay.ref(), K, code) if params else 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        # bound to names until the launch is queued: a copy whose only owner is an argument expression goes back to the
        # allocator before the next copy is made, which then lands on it (the cotangent of .sum() is a stride-0 view)
        grad, data, alpha, logz = grad.contiguous(), data.contiguous(), alpha.contiguous(), logz.contiguous()
        transitions, end = _crf_small(transitions), _crf_small(end)
        _call('crf_partition_bwd', 'rua_segment_crf_backward', dev, lay.ref(), L.ptr(grad), L.ptr(data),
              L.ptr(transitions), L.ptr(end), L.ptr(alpha), L.ptr(logz), L.ptr(gx), L.ptr(gt), L.ptr(gs), L.ptr(ge), K, code,
              L.ptr(ws))
    return gx, gt, gs, ge


class _CrfPartition(torch.autograd.Function):
    """logZ [B] of every sequence.  Saves the forward table alpha ([rows, K], accumulator type, the emissions' storage
    layout), logZ and the inputs; the backward is one fused walk plus the finish launch of the parameter sums.  Second
    derivatives are out of scope."""

    @staticmethod
    def forward(ctx, data: Tensor, transitions: Tensor, start: Optional[Tensor], end: Optional[Tensor], lay: M.Lay, K: int):
        logz, alpha, _, _ = launch_crf_forward(lay, data, transitions, start, end, K, want_alpha=True)
        ctx.lay, ctx.K, ctx.has_end = lay, K, end is not None
        ctx.save_for_backward(*((data, transitions, alpha, logz) + ((end,) if end is not None else ())))
        return logz

    @staticmethod
    def backward(ctx, grad: Tensor):
        if torch.is_grad_enabled():
            raise L.RuaError('crf_partition: second derivatives (create_graph=True) are out of scope')
        data, transitions, alpha, logz = ctx.saved_tensors[:4]
        end = ctx.saved_tensors[4] if ctx.has_end else None
        want = ctx.needs_input_grad
        gx, gt, gs, ge = launch_crf_backward(ctx.lay, grad, data, transitions, end, alpha, logz, ctx.K, want[0], want[1],
                                             want[2], want[3])
        return gx, gt, gs, ge, None, None


def crf_partition(data: Tensor, transitions: Tensor, start: Optional[Tensor], end: Optional[Tensor], lay: M.Lay,
                  K: int) -> Tensor:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (data, transitions, start, end)):
        # contiguous HERE, before the Function (as in cumsum()): a copy made inside forward() would carry no history
        return _CrfPartition.apply(data.contiguous(), transitions, start, end, lay, K)
    return launch_crf_forward(lay, _plain(data), transitions, start, end, K)[0]


# ------------------------------------------------------------------ per-sequence CTC (an extension)
_CTC_SUPPORT = 'ctc: the log-probabilities are one of'


def ctc_args(what: str, data: Tensor, hidden: Tuple[int, ...], n_seq: int, labels, label_hidden, n_target_seq: int,
             blank, before_device: Optional[Callable[[], None]] = None) -> int:
    """V, after the checks that come before any launch and need no lengths, each naming its argument: float
    `log_probs` with exactly one hidden dimension (the V classes); int64 `targets` without hidden dimensions, with the
    same number of sequences, on the same device; `blank` in [0, V); and last (so that every other refusal can be met
    without a GPU) the log-probabilities on a HIP device."""
    if data.dtype not in L.DTYPES:
        raise L.RuaError(f'{what}: `log_probs` is one of {list(L.DTYPES)}; got {data.dtype}')
    if len(hidden) != 1:
        raise L.RuaError(f'{what}: `log_probs` has exactly ONE hidden dimension (the V classes); got hidden dimensions '
                         f'{tuple(hidden)}')
    V = int(hidden[0])
    if not isinstance(labels, Tensor) or labels.dtype != torch.int64:
        raise L.RuaError(f'{what}: `targets` holds torch.int64 labels; got '
                         f'{labels.dtype if isinstance(labels, Tensor) else type(labels).__name__}')
    if len(label_hidden):
        raise L.RuaError(f'{what}: `targets` holds ONE label per token; got hidden dimensions {tuple(label_hidden)}')
    if n_target_seq != n_seq:
        raise L.RuaError(f'{what}: `targets` holds {n_target_seq} sequences, `log_probs` {n_seq}')
    if labels.device != data.device:
        raise L.RuaError(f'{what}: `targets` lives on {labels.device}, `log_probs` on {data.device}')
    if isinstance(blank, bool) or not isinstance(blank, int) or not 0 <= blank < V:
        raise L.RuaError(f'{what}: `blank` = {blank!r} is not a class of [0, {V})')
    if before_device is not None:
        before_device()
    if not data.is_cuda:
        raise L.RuaError(f'{what}: `log_probs` lives on {data.device}; move it to a HIP device (there is no CPU fallback '
                         f'by design)')
    return V


def ctc_target_bound(what: str, s_max: int) -> int:
    """The longest target of the batch, which sizes the launch.  Longer than CTC_MAX_TARGET: refused, before any launch."""
    if s_max > L.CTC_MAX_TARGET:
        raise L.RuaError(f'{what}: the longest of `targets` has {s_max} labels; at most {L.CTC_MAX_TARGET} '
                         f'(2 S + 1 <= {2 * L.CTC_MAX_TARGET + 1} states)')
    return max(s_max, 0)


class CtcPlan(NamedTuple):
    """What every CTC launch of one call shares: both layouts, V, the state bound and blank."""
    frames: M.Lay
    targets: M.Lay
    V: int
    S_max: int
    blank: int


def launch_ctc_forward(plan: CtcPlan, data: Tensor, labels: Tensor, viterbi: bool = False, want_alpha: bool = False,
                       zero_infinity: bool = False):
    """rua_segment_ctc_forward: ONE launch.  (out [B], logZ [B] or None, alpha [*storage, 2 S_max + 1] or None, codes or
    None, last or None), in the accumulator type.  B == 0: empty results without a launch."""
    code = _require_dtype(data, L.DTYPES, _CTC_SUPPORT)
    dev, acc = data.device, _acc_dtype(data.dtype)
    lay = plan.frames
    data, labels = data.contiguous(), labels.contiguous()
    table = tuple(data.shape[:-1]) + (2 * plan.S_max + 1,)
    out = torch.empty(lay.B, dtype=acc, device=dev)
    logz = torch.empty(lay.B, dtype=acc, device=dev) if not viterbi else None
    alpha = torch.empty(table, dtype=acc, device=dev) if want_alpha and not viterbi else None
    codes = torch.empty(table, dtype=torch.uint8, device=dev) if viterbi else None
    last = torch.empty(lay.B, dtype=torch.int64, device=dev) if viterbi else None
    if lay.B:
        _call('ctc_align' if viterbi else 'ctc_loss', 'rua_segment_ctc_forward', dev, lay.ref(), plan.targets.ref(),
              L.ptr(data), L.ptr(labels), L.ptr(alpha), L.ptr(codes), L.ptr(out), L.ptr(logz), L.ptr(last), plan.V,
              plan.S_max, plan.blank, code, L.CRF_MAX if viterbi else L.CRF_LOG, int(bool(zero_infinity)))
    return out, logz, alpha, codes, last


def launch_ctc_backtrace(plan: CtcPlan, labels: Tensor, codes: Tensor, last: Tensor, lead_shape: Sequence[int]):
    """rua_segment_ctc_backtrace: a launch of its own on the same stream; (labels, positions), int64, one per row."""
    dev = codes.device
    out_labels = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)     # padding rows: zeroed by the call
    out_positions = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)
    if plan.frames.B and out_labels.numel():
        labels = labels.contiguous()
        _call('ctc_backtrace', 'rua_segment_ctc_backtrace', dev, plan.frames.ref(), plan.targets.ref(), L.ptr(labels),
              L.ptr(codes), L.ptr(last), L.ptr(out_labels), L.ptr(out_positions), plan.V, plan.S_max, plan.blank)
    return out_labels, out_positions


def launch_ctc_backward(plan: CtcPlan, grad: Tensor, data: Tensor, labels: Tensor, alpha: Tensor, logz: Tensor) -> Tensor:
    """rua_segment_ctc_backward: the gradient of the log-probabilities, every row written once by ONE launch."""
    code = _require_dtype(data, L.DTYPES, _CTC_SUPPORT)
    dev, acc = data.device, _acc_dtype(data.dtype)
    lay = plan.frames
    L.require_device(grad, data, labels, alpha, logz)
    if grad.dtype != acc or tuple(grad.shape) != (lay.B,):
        raise L.RuaError(f'ctc backward: the cotangent of the loss is a {acc} tensor of shape ({lay.B},)')
    gx = torch.empty(data.shape, dtype=data.dtype, device=dev)
    if lay.B and gx.numel():
        # bound to names until the launch is queued (see launch_crf_backward)
        grad, data, labels, alpha, logz = (grad.contiguous(), data.contiguous(), labels.contiguous(), alpha.contiguous(),
                                           logz.contiguous())
        _call('ctc_loss_bwd', 'rua_segment_ctc_backward', dev, lay.ref(), plan.targets.ref(), L.ptr(grad), L.ptr(data),
              L.ptr(labels), L.ptr(alpha), L.ptr(logz), L.ptr(gx), plan.V, plan.S_max, plan.blank, code)
    return gx


class _CtcLoss(torch.autograd.Function):
    """The negative log-likelihood [B] of every sequence.  Saves the forward table alpha ([rows, 2 S_max + 1],
    accumulator type, the frames' storage layout), logZ, the log-probabilities and the labels; the backward is one
    fused walk.  Second derivatives are out of scope."""

    @staticmethod
    def forward(ctx, data: Tensor, labels: Tensor, plan: CtcPlan, zero_infinity: bool):
        loss, logz, alpha, _, _ = launch_ctc_forward(plan, data, labels, want_alpha=True, zero_infinity=zero_infinity)
        ctx.plan = plan
        ctx.save_for_backward(data, labels, alpha, logz)
        return loss

    @staticmethod
    def backward(ctx, grad: Tensor):
        if torch.is_grad_enabled():
            raise L.RuaError('ctc_loss: second derivatives (create_graph=True) are out of scope')
        data, labels, alpha, logz = ctx.saved_tensors
        return launch_ctc_backward(ctx.plan, grad, data, labels, alpha, logz), None, None, None


def ctc_loss(data: Tensor, labels: Tensor, plan: CtcPlan, zero_infinity: bool) -> Tensor:
    if torch.is_grad_enabled() and data.requires_grad:
        # contiguous HERE, before the Function (as in cumsum()): a copy made inside forward() would carry no history
        return _CtcLoss.apply(data.contiguous(), labels, plan, bool(zero_infinity))
    return launch_ctc_forward(plan, _plain(data), labels, zero_infinity=zero_infinity)[0]


# ------------------------------------------------------------------ per-sequence edit distance (an extension)
def edit_args(what: str, hyp, hyp_hidden, n_seq: int, ref, ref_hidden, n_ref_seq: int,
              before_device: Optional[Callable[[], None]] = None) -> None:
    """The checks that come before any launch and need no lengths, each naming its argument: int64 `hyp` and `ref`
    without hidden dimensions, with the same number of sequences, on the same device; and last (so that every other
    refusal can be met without a GPU) the tokens on a HIP device."""
    for name, t, hidden in (('hyp', hyp, hyp_hidden), ('ref', ref, ref_hidden)):
        if not isinstance(t, Tensor) or t.dtype != torch.int64:
            raise L.RuaError(f'{what}: `{name}` holds torch.int64 tokens; got '
                             f'{t.dtype if isinstance(t, Tensor) else type(t).__name__}')
        if len(hidden):
            raise L.RuaError(f'{what}: `{name}` holds ONE token per position; got hidden dimensions {tuple(hidden)}')
    if n_ref_seq != n_seq:
        raise L.RuaError(f'{what}: `ref` holds {n_ref_seq} sequences, `hyp` {n_seq}')
    if ref.device != hyp.device:
        raise L.RuaError(f'{what}: `ref` lives on {ref.device}, `hyp` on {hyp.device}')
    if before_device is not None:
        before_device()
    if not hyp.is_cuda:
        raise L.RuaError(f'{what}: `hyp` lives on {hyp.device}; move it to a HIP device (there is no CPU fallback by '
                         f'design)')


def edit_ref_bound(what: str, s_max: int) -> int:
    """The longest reference of the batch, which sizes the launch.  Longer than EDIT_MAX_REF: refused, before any launch."""
    if s_max > L.EDIT_MAX_REF:
        raise L.RuaError(f'{what}: the longest of `ref` has {s_max} tokens; at most {L.EDIT_MAX_REF} (`hyp` is unbounded: '
                         f'swap the arguments — the distance is symmetric, insertions and deletions trade places)')
    return max(s_max, 0)


class EditPlan(NamedTuple):
    """What both edit-distance launches of one call share: the two layouts and the column bound."""
    hyp: M.Lay
    ref: M.Lay
    S_max: int


def launch_edit_forward(plan: EditPlan, hyp: Tensor, ref: Tensor, want_codes: bool = False):
    """rua_segment_edit_forward: ONE launch.  (distance [B] int64, codes [*hyp storage, S_max] uint8 or None).  The
    distance-only launch allocates and writes no table.  B == 0: empty results without a launch."""
    dev = L.require_device(hyp, ref)
    hyp, ref = hyp.contiguous(), ref.contiguous()
    dist = torch.empty(plan.hyp.B, dtype=torch.int64, device=dev)
    codes = torch.empty(tuple(hyp.shape) + (plan.S_max,), dtype=torch.uint8, device=dev) if want_codes else None
    if plan.hyp.B:
        # (a table without an element has no address: the launch then writes none)
        _call('edit_align' if want_codes else 'edit_distance', 'rua_segment_edit_forward', dev, plan.hyp.ref(),
              plan.ref.ref(), L.ptr(hyp), L.ptr(ref), L.ptr(dist), L.ptr(codes) if want_codes and codes.numel() else 0,
              plan.S_max)
    return dist, codes


def launch_edit_backtrace(plan: EditPlan, codes: Tensor, lead_shape: Sequence[int]):
    """rua_segment_edit_backtrace: a launch of its own on the same stream; (positions, one per row of the hyp storage,
    substitutions, insertions, deletions [B]), all int64."""
    dev = codes.device
    positions = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)      # padding rows: zeroed by the call
    subs, ins, dels = (torch.empty(plan.hyp.B, dtype=torch.int64, device=dev) for _ in range(3))
    if plan.hyp.B:
        _call('edit_backtrace', 'rua_segment_edit_backtrace', dev, plan.hyp.ref(), plan.ref.ref(),
              L.ptr(codes) if codes.numel() else 0, L.ptr(positions) if positions.numel() else 0, L.ptr(subs),
              L.ptr(ins), L.ptr(dels), plan.S_max)
    return positions, subs, ins, dels


# ------------------------------------------------------------------ per-sequence gated linear recurrence (an extension)
def _gate_arg(data: Tensor, gate) -> Tuple[Optional[Tensor], float]:
    """(the gate tensor or None, the scalar gate): a tensor of the payload's storage shape, dtype and device, or ONE
    Python number — checked before any launch."""
    if isinstance(gate, Tensor):
        L.require_device(data, gate)
        if gate.dtype != data.dtype:
            raise L.RuaError(f'linear_scan: the gate has dtype {gate.dtype}, the payload {data.dtype}')
        if gate.shape != data.shape:
            raise L.RuaError(f'linear_scan: the gate has shape {tuple(gate.shape)}, the payload\'s storage '
                             f'{tuple(data.shape)} (gates do not broadcast)')
        return gate, 0.0
    if isinstance(gate, bool) or not isinstance(gate, (int, float)):
        raise L.RuaError('linear_scan: the gate is a tensor of the payload\'s storage shape, a container of the same type '
                         f'or a Python float; got {type(gate).__name__}')
    return None, float(gate)


def launch_linear_scan(lay: M.Lay, data: Tensor, gate, reverse: bool, hidden: Tuple[int, ...],
                       out: Optional[Tensor] = None, cut: bool = True) -> Tensor:
    """rua_segment_linear_scan: h_u = a_u * h_(u-1) + x_u in one launch (two for cut sequences); payload and gate are
    read once, the result is written once.  `gate` is a tensor or a Python float (passed by value: no gate tensor
    exists).  `out` may be `data` itself, never the gate.  cut=False withholds the workspace (the same bits from one
    workgroup per unit: a developer A/B)."""
    code = _require_dtype(data, L.DTYPES, 'linear_scan supports')
    gt, gs = _gate_arg(data, gate)
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_linear_scan_ws_bytes', lay, H, code, dev, cut)
    data = data.contiguous()
    gt = None if gt is None else gt.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'linear_scan' + _LIKE_PAYLOAD)      # padding rows: zeroed by the call
    _call('linear_scan_rev' if reverse else 'linear_scan', 'rua_segment_linear_scan', dev, lay.ref(), L.ptr(data),
          L.ptr(gt), gs, L.ptr(out), H, code, int(bool(reverse)), L.ptr(ws))
    return out


def launch_linear_scan_backward(lay: M.Lay, grad: Tensor, gate, h: Optional[Tensor], reverse: bool,
                                hidden: Tuple[int, ...], want_gate: bool = True,
                                cut: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """rua_segment_linear_scan_backward: (grad_x, grad_gate or None) of the scan whose direction was `reverse`, from the
    cotangent, the gate and the saved output `h` — one launch (two for cut sequences).  Padding rows of both are zeros."""
    code = _require_dtype(grad, L.DTYPES, 'linear_scan supports')
    dev = grad.device
    gt, gs = _gate_arg(grad, gate)
    want_gate = bool(want_gate) and gt is not None
    if want_gate:
        L.require_device(grad, h)
        if h is None or h.dtype != grad.dtype or h.shape != grad.shape:
            raise L.RuaError('linear_scan backward: the saved output must have the dtype and shape of the cotangent')
        h = h.contiguous()
    H = _prod(hidden)
    ws = _workspace('rua_linear_scan_ws_bytes', lay, H, code, dev, cut)
    grad = grad.contiguous()
    gt = None if gt is None else gt.contiguous()
    gx = torch.empty(grad.shape, dtype=grad.dtype, device=dev)
    ga = torch.empty(grad.shape, dtype=grad.dtype, device=dev) if want_gate else None
    _call('linear_scan_rev_bwd' if reverse else 'linear_scan_bwd', 'rua_segment_linear_scan_backward', dev, lay.ref(),
          L.ptr(grad), L.ptr(gt), gs, L.ptr(h if want_gate else None), L.ptr(gx), L.ptr(ga), H, code, int(bool(reverse)),
          L.ptr(ws))
    return gx, ga


class _LinearScan(torch.autograd.Function):
    """h = the gated linear recurrence of every sequence.  Saves the gate and the OUTPUT (not the payload); the
    backward is one fused kernel: the same recurrence run the other way, and grad_gate = grad_x * the neighbouring h."""

    @staticmethod
    def forward(ctx, data: Tensor, gate: Optional[Tensor], gate_scalar: float, lay: M.Lay, reverse: bool, hidden):
        h = launch_linear_scan(lay, data, gate_scalar if gate is None else gate, reverse, hidden)
        ctx.lay, ctx.reverse, ctx.hidden, ctx.gate_scalar, ctx.has_gate = lay, reverse, tuple(hidden), gate_scalar, gate is not None
        if gate is None:
            ctx.save_for_backward(h)
        else:
            ctx.save_for_backward(h, gate)
        return h

    @staticmethod
    def backward(ctx, grad: Tensor):
        h = ctx.saved_tensors[0]
        gate = ctx.saved_tensors[1] if ctx.has_gate else None
        want_gate = ctx.has_gate and ctx.needs_input_grad[1]
        if torch.is_grad_enabled():
            # a graph of this backward is being recorded (create_graph=True): the gradient spelled with the library's
            # differentiable pieces (the scan itself and the roll), as _composed_softmax_grad does
            gx, ga = _composed_linear_scan_grad(grad, gate, ctx.gate_scalar, h, ctx.lay, ctx.reverse, ctx.hidden, want_gate)
        else:
            gx, ga = launch_linear_scan_backward(ctx.lay, grad, ctx.gate_scalar if gate is None else gate, h, ctx.reverse,
                                                 ctx.hidden, want_gate)
        return gx, ga, None, None, None, None


def _composed_linear_scan_grad(grad: Tensor, gate: Optional[Tensor], gate_scalar: float, h: Tensor, lay: M.Lay,
                               reverse: bool, hidden, want_gate: bool):
    """(d / d payload, d / d gate) as differentiable functions of (grad, gate, h).  roll(a, -1) puts the wrapped-around
    gate exactly on the position the reverse scan ignores, so dx = linear_scan(g, roll(a, -1), reverse=True); and
    da = dx * roll(h, 1) with position 0 masked (mirrored for the reverse scan)."""
    def roll(v: Tensor, shifts: int) -> Tensor:
        return move(v.contiguous(), MovePlan(lay, lay, tuple(v.shape), L.T_ROLL, shifts, fill=0, name='roll'))

    if gate is None:
        return linear_scan(grad.contiguous(), gate_scalar, lay, not reverse, hidden), None
    step = 1 if reverse else -1
    dx = linear_scan(grad.contiguous(), roll(gate, step), lay, not reverse, hidden)
    if not want_gate:
        return dx, None
    # the token whose gate the scan ignored: the first one (the last one for `reverse`)
    ones = torch.ones((lay.B,) + tuple(hidden), dtype=h.dtype, device=h.device)
    zero_pos = torch.zeros((lay.B,) + tuple(hidden), dtype=torch.int64, device=h.device)
    ignored = launch_put(lay, ones, zero_pos, tuple(hidden), tuple(h.shape))
    if reverse:
        ignored = launch_move(MovePlan(lay, lay, tuple(h.shape), L.T_ROLL, -1, fill=0, name='roll'), ignored)
    da = torch.where(ignored != 0, torch.zeros_like(dx), dx * roll(h, -step))
    return dx, da


def linear_scan(data: Tensor, gate, lay: M.Lay, reverse: bool, hidden) -> Tensor:
    _require_dtype(data, L.DTYPES, 'linear_scan supports')
    gt, gs = _gate_arg(data, gate)
    if torch.is_grad_enabled() and (data.requires_grad or (gt is not None and gt.requires_grad)):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _LinearScan.apply(data.contiguous(), None if gt is None else gt.contiguous(), gs, lay, bool(reverse),
                                 tuple(hidden))
    return launch_linear_scan(lay, _plain(data), gs if gt is None else _plain(gt), bool(reverse), tuple(hidden))


# ------------------------------------------------------------------ per-sequence causal depthwise conv (an extension)
_CONV_SUPPORT = 'causal_conv supports'


def _conv_args(data: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], hidden: Tuple[int, ...],
               taps: Optional[int] = None) -> int:
    """K, after the checks that need no device — the filter is [K, *hidden] with 1 <= K <= CONV_MAX_TAPS, the bias
    [*hidden], both of the payload's dtype — and then the one that does: everything on one HIP device."""
    hidden = tuple(hidden)
    if weight is not None:
        if weight.dim() != 1 + len(hidden) or tuple(weight.shape[1:]) != hidden:
            raise L.RuaError(f'causal_conv: the weight has shape {tuple(weight.shape)}, the payload\'s hidden dimensions '
                             f'are {hidden}: it must be [K, *hidden] (tap-major)')
        taps = int(weight.shape[0])
    if taps is None or not 1 <= taps <= L.CONV_MAX_TAPS:
        raise L.RuaError(f'causal_conv: 1 <= K <= {L.CONV_MAX_TAPS} taps; got {taps}')
    if bias is not None and tuple(bias.shape) != hidden:
        raise L.RuaError(f'causal_conv: the bias has shape {tuple(bias.shape)}, the payload\'s hidden dimensions are {hidden}')
    for name, t in (('weight', weight), ('bias', bias)):
        if t is not None and t.dtype != data.dtype:
            raise L.RuaError(f'causal_conv: the {name} has dtype {t.dtype}, the payload {data.dtype}')
    L.require_device(data, weight, bias)
    return taps


def launch_causal_conv(lay: M.Lay, data: Tensor, weight: Tensor, bias: Optional[Tensor], reverse: bool,
                       hidden: Tuple[int, ...], out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_causal_conv: one launch, one read and one write of the payload; no workspace.  `out` may be `data`
    itself, never the weight or the bias."""
    taps = _conv_args(data, weight, bias, hidden)
    code = _require_dtype(data, L.DTYPES, _CONV_SUPPORT)
    dev, H = data.device, _prod(hidden)
    data, weight = data.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    out = _target(out, data.shape, data.dtype, dev, 'causal_conv' + _LIKE_PAYLOAD)      # padding rows: zeroed by the call
    _call('causal_conv_rev' if reverse else 'causal_conv', 'rua_segment_causal_conv', dev, lay.ref(), L.ptr(data),
          L.ptr(weight), L.ptr(bias), L.ptr(out), H, taps, code, int(bool(reverse)))
    return out


def launch_causal_conv_backward(lay: M.Lay, grad: Tensor, data: Optional[Tensor], weight: Optional[Tensor],
                                reverse: bool, hidden: Tuple[int, ...], taps: Optional[int] = None,
                                want_input: bool = True, want_weight: bool = True,
                                want_bias: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor]]:
    """rua_segment_causal_conv_backward: (grad_input, grad_weight, grad_bias) — None where not wanted — of the
    convolution whose direction was `reverse`: one walk, plus a small finish when a [K, H] / [H] sum is wanted.  With
    only grad_input wanted `data` is not read and no workspace is allocated."""
    want_input, want_weight, want_bias = bool(want_input), bool(want_weight), bool(want_bias)
    data = data if want_weight else None
    weight = weight if want_input or taps is None else None
    taps = _conv_args(grad, weight, None, hidden, taps)
    code = _require_dtype(grad, L.DTYPES, _CONV_SUPPORT)
    dev, H = grad.device, _prod(hidden)
    if want_weight:
        L.require_device(grad, data)
        if data is None or data.dtype != grad.dtype or data.shape != grad.shape:
            raise L.RuaError('causal_conv backward: the saved payload must have the dtype and shape of the cotangent')
        data = data.contiguous()
    if want_input and weight is None:
        raise L.RuaError('causal_conv backward: grad_input needs the weight')
    grad = grad.contiguous()
    weight = weight.contiguous() if want_input else None
    # the partial sums of grad_weight / grad_bias: at most 1 024 parts per column chunk, whatever the number of tokens
    ws = _workspace('rua_causal_conv_ws_bytes', lay, H, code, dev, want_weight or want_bias, taps)
    gx = torch.empty(grad.shape, dtype=grad.dtype, device=dev) if want_input else None
    # (nothing to walk: the entry point returns without a launch, and an empty sum is 0)
    small = torch.zeros if lay.B == 0 or lay.n_rows == 0 or H == 0 else torch.empty
    gw = small((taps,) + tuple(hidden), dtype=grad.dtype, device=dev) if want_weight else None
    gb = small(tuple(hidden), dtype=grad.dtype, device=dev) if want_bias else None
    _call('causal_conv_rev_bwd' if reverse else 'causal_conv_bwd', 'rua_segment_causal_conv_backward', dev, lay.ref(),
          L.ptr(grad), L.ptr(data), L.ptr(weight), L.ptr(gx), L.ptr(gw), L.ptr(gb), H, taps, code, int(bool(reverse)),
          L.ptr(ws))
    return gx, gw, gb


class _CausalConv(torch.autograd.Function):
    """y = the causal depthwise convolution of every sequence.  Saves the weight, and the payload only when the weight
    needs a gradient; the backward is one fused entry point.  While a graph of the backward is being recorded
    (create_graph=True) it is composed of two differentiable primitives that close over each other: the convolution
    itself (linear in each argument) and _ConvWeightGrad."""

    @staticmethod
    def forward(ctx, data: Tensor, weight: Tensor, bias: Optional[Tensor], lay: M.Lay, reverse: bool, hidden):
        ctx.lay, ctx.reverse, ctx.hidden, ctx.taps = lay, reverse, tuple(hidden), int(weight.shape[0])
        ctx.saved_data = ctx.needs_input_grad[1]
        if ctx.saved_data:
            ctx.save_for_backward(weight, data)
        else:
            ctx.save_for_backward(weight)
        return launch_causal_conv(lay, data, weight, bias, reverse, hidden)

    @staticmethod
    def backward(ctx, grad: Tensor):
        weight = ctx.saved_tensors[0]
        data = ctx.saved_tensors[1] if ctx.saved_data else None
        want_x, want_w, want_b = ctx.needs_input_grad[:3]
        if torch.is_grad_enabled():
            grad = grad.contiguous()
            gx = causal_conv(grad, weight, None, ctx.lay, not ctx.reverse, ctx.hidden) if want_x else None
            gw = gb = None
            if want_w or want_b:
                gw, gb = _ConvWeightGrad.apply(grad, data, ctx.lay, ctx.reverse, ctx.hidden, ctx.taps, want_w, want_b)
        else:
            gx, gw, gb = launch_causal_conv_backward(ctx.lay, grad, data, weight, ctx.reverse, ctx.hidden, ctx.taps,
                                                     want_x, want_w, want_b)
        return gx, gw, gb, None, None, None


class _ConvWeightGrad(torch.autograd.Function):
    """(g, x) -> (grad_weight [K, *hidden], grad_bias [*hidden]) of the convolution whose direction was `reverse`:
    gw[k] = sum_t g[t] * x[the token tap k read], gb = sum_t g[t].  Bilinear, so with cotangents (cw, cb) its adjoints
    are convolutions again:  d / dg = causal_conv(x, cw, bias=cb)  in the same direction,
    d / dx = causal_conv(g, cw, reverse = the other direction) — derivatives of any order from the library's kernels."""

    @staticmethod
    def forward(ctx, g: Tensor, x: Optional[Tensor], lay: M.Lay, reverse: bool, hidden, taps: int, want_w: bool,
                want_b: bool):
        ctx.lay, ctx.reverse, ctx.hidden, ctx.taps, ctx.has_x = lay, reverse, tuple(hidden), taps, x is not None
        ctx.save_for_backward(*((g, x) if x is not None else (g,)))
        _, gw, gb = launch_causal_conv_backward(lay, g, x, None, reverse, hidden, taps, False, want_w and x is not None,
                                                want_b)
        return gw, gb

    @staticmethod
    def backward(ctx, cw: Optional[Tensor], cb: Optional[Tensor]):
        g = ctx.saved_tensors[0]
        x = ctx.saved_tensors[1] if ctx.has_x else None
        dg = dx = None
        if ctx.needs_input_grad[0] and (cw is not None or cb is not None):
            if cw is not None and x is not None:
                dg = causal_conv(x, cw.contiguous(), cb, ctx.lay, ctx.reverse, ctx.hidden)
            else:
                # only the bias' cotangent: every live token receives cb (a one-tap filter of zeros, plus the bias)
                zero = torch.zeros((1,) + ctx.hidden, dtype=g.dtype, device=g.device)
                dg = causal_conv(torch.zeros_like(g), zero, cb, ctx.lay, ctx.reverse, ctx.hidden)
        if x is not None and ctx.needs_input_grad[1] and cw is not None:
            dx = causal_conv(g, cw.contiguous(), None, ctx.lay, not ctx.reverse, ctx.hidden)
        return dg, dx, None, None, None, None, None, None


def causal_conv(data: Tensor, weight: Tensor, bias: Optional[Tensor], lay: M.Lay, reverse: bool, hidden) -> Tensor:
    _conv_args(data, weight, bias, tuple(hidden))
    _require_dtype(data, L.DTYPES, _CONV_SUPPORT)
    if torch.is_grad_enabled() and (data.requires_grad or weight.requires_grad or
                                    (bias is not None and bias.requires_grad)):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _CausalConv.apply(data.contiguous(), weight.contiguous(), None if bias is None else bias.contiguous(), lay,
                                 bool(reverse), tuple(hidden))
    return launch_causal_conv(lay, _plain(data), _plain(weight), None if bias is None else _plain(bias), bool(reverse),
                              tuple(hidden))


# ------------------------------------------------------------------ per-sequence compress: keep tokens by mask (an extension)
def launch_compress_plan(lay: M.Lay, mask: Tensor, cut: bool = True) -> Tuple[Tensor, Tensor]:
    """rua_segment_compress_plan: (rank int32 [storage rows of `lay`], new_lens int64 [B]) from a bool mask with one
    value per storage row — one launch (two for cut sequences); the mask is read once.  rank is the position a kept
    token takes in its new sequence, -1 for a dropped token and for a padding row.  cut=False withholds the workspace
    (the same bits from one workgroup per sequence: a developer A/B)."""
    dev = L.require_device(mask)
    if mask.dtype != torch.bool or mask.numel() != lay.n_rows:
        raise L.RuaError(f'compress plan: the mask is a torch.bool tensor with one value per storage row ({lay.n_rows}); '
                         f'got {mask.dtype} with {mask.numel()} values')
    mask = _plain(mask).contiguous()
    rank = torch.empty(lay.n_rows, dtype=torch.int32, device=dev)
    new_lens = torch.empty(lay.B, dtype=torch.int64, device=dev)
    if lay.B == 0:
        return rank.fill_(-1), new_lens                 # (the entry point returns without a launch)
    ws = _workspace('rua_compress_ws_bytes', lay, None, None, dev, cut)
    _call('compress_plan', 'rua_segment_compress_plan', dev, lay.ref(), L.ptr(mask), L.ptr(rank), L.ptr(new_lens),
          L.ptr(ws))
    return rank, new_lens


def launch_compress_move(small: M.Lay, big: M.Lay, rank: Tensor, src: Tensor, hidden: Tuple[int, ...],
                         out_shape: Sequence[int], expand: bool, out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_compress_move: expand=False copies the rows of `src` (storage of `big`) whose rank is >= 0 to their
    rows of a new payload of `small`; expand=True is the adjoint — `src` has the storage of `small`, the result that of
    `big`, zeros at dropped tokens.  Rows move as bits; padding rows of a padded result are zeros; one launch."""
    dev = L.require_device(src, rank)
    if src.element_size() not in (1, 2, 4, 8):
        raise L.RuaError(f'compress moves elements of 1, 2, 4 or 8 bytes; got {src.dtype}')
    if rank.dtype != torch.int32 or rank.numel() != big.n_rows or not rank.is_contiguous():
        raise L.RuaError('compress move: the rank table is a contiguous int32 tensor with one entry per storage row')
    src = src.contiguous()
    out = _target(out, out_shape, src.dtype, dev, 'compress' + _LIKE_PAYLOAD)
    if out.numel() == 0:
        return out
    if src.numel() == 0:
        return out.zero_()                              # nothing was kept (or nothing came in): padding / zeros only
    rb = _prod(hidden) * src.element_size()
    args = (L.ptr(out), L.ptr(src)) if not expand else (L.ptr(src), L.ptr(out))
    _call('compress_expand' if expand else 'compress_move', 'rua_segment_compress_move', dev, small.ref(), big.ref(),
          L.ptr(rank), *args, rb, int(bool(expand)))
    return out


class _Compress(torch.autograd.Function):
    """payload of `big` -> payload of `small`: linear, its adjoint is _Expand with the same rank table.  Saves ONLY
    the int32 rank table (the mask is folded into it); no payload, no int64 index."""

    @staticmethod
    def forward(ctx, data: Tensor, rank: Tensor, small: M.Lay, big: M.Lay, hidden, small_shape, big_shape):
        ctx.args = (small, big, tuple(hidden), tuple(small_shape), tuple(big_shape))
        ctx.save_for_backward(rank)
        return launch_compress_move(small, big, rank, data, hidden, small_shape, False)

    @staticmethod
    def backward(ctx, grad: Tensor):
        rank, = ctx.saved_tensors
        return (expand(grad, rank, *ctx.args),) + (None,) * 6


class _Expand(torch.autograd.Function):
    """payload of `small` -> payload of `big` with zeros at dropped tokens and padding: the adjoint of _Compress, and
    _Compress is its adjoint — derivatives of every order from the one kernel."""

    @staticmethod
    def forward(ctx, data: Tensor, rank: Tensor, small: M.Lay, big: M.Lay, hidden, small_shape, big_shape):
        ctx.args = (small, big, tuple(hidden), tuple(small_shape), tuple(big_shape))
        ctx.save_for_backward(rank)
        return launch_compress_move(small, big, rank, data, hidden, big_shape, True)

    @staticmethod
    def backward(ctx, grad: Tensor):
        rank, = ctx.saved_tensors
        return (compress(grad, rank, *ctx.args),) + (None,) * 6


def compress(data: Tensor, rank: Tensor, small: M.Lay, big: M.Lay, hidden, small_shape, big_shape) -> Tensor:
    L.require_device(data)
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _Compress.apply(data.contiguous(), rank, small, big, tuple(hidden), tuple(small_shape), tuple(big_shape))
    return launch_compress_move(small, big, rank, _plain(data), tuple(hidden), tuple(small_shape), False)


def expand(data: Tensor, rank: Tensor, small: M.Lay, big: M.Lay, hidden, small_shape, big_shape) -> Tensor:
    L.require_device(data)
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        return _Expand.apply(data.contiguous(), rank, small, big, tuple(hidden), tuple(small_shape), tuple(big_shape))
    return launch_compress_move(small, big, rank, _plain(data), tuple(hidden), tuple(big_shape), True)


# ------------------------------------------------------------------ per-sequence unique_consecutive (an extension)
def launch_runs_heads(lay: M.Lay, data: Tensor, hidden: Tuple[int, ...]) -> Tensor:
    """rua_segment_runs_heads: a bool per storage row of `lay` — whether the token is the first of its sequence or
    differs from its predecessor in it (IEEE equality for the float dtypes, bits otherwise).  One launch, the only one
    that reads the payload; what launch_compress_plan scans.  Padding rows are not written."""
    dev = L.require_device(data)
    if data.is_complex() or data.element_size() not in (1, 2, 4, 8):
        raise L.RuaError(f'unique_consecutive compares elements of 1, 2, 4 or 8 bytes that are not complex; got {data.dtype}')
    data = _plain(data).contiguous()
    head = torch.empty(lay.n_rows, dtype=torch.bool, device=dev)
    if lay.B == 0 or lay.n_rows == 0:
        return head
    _call('runs_heads', 'rua_segment_runs_heads', dev, lay.ref(), L.ptr(data), _prod(hidden) * data.element_size(),
          L.DTYPES.get(data.dtype, L.RUNS_BITS), L.ptr(head))
    return head


def launch_runs_inverse(lay: M.Lay, head: Tensor, lead_shape: Sequence[int], cut: bool = True) -> Tensor:
    """rua_segment_runs_inverse: int64 of the storage's token dimensions — the index of every token's run inside its
    sequence, zeros in padding rows — from the head mask; one launch (two for cut sequences)."""
    dev = L.require_device(head)
    if head.dtype != torch.bool or head.numel() != lay.n_rows or not head.is_contiguous():
        raise L.RuaError('runs inverse: the head mask is a contiguous torch.bool tensor with one value per storage row')
    inverse = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)
    if inverse.numel() != lay.n_rows:
        raise L.RuaError(f'runs inverse: the token dimensions {tuple(lead_shape)} do not hold {lay.n_rows} storage rows')
    if lay.B == 0 or lay.n_rows == 0:
        return inverse
    ws = _workspace('rua_compress_ws_bytes', lay, None, None, dev, cut)
    lens = torch.empty(lay.B, dtype=torch.int64, device=dev)     # (the scan's sums: the plan's new lengths again)
    _call('runs_inverse', 'rua_segment_runs_inverse', dev, lay.ref(), L.ptr(head), L.ptr(inverse), L.ptr(lens), L.ptr(ws))
    return inverse


def launch_runs_counts(small: M.Lay, big: M.Lay, rank: Tensor, lead_shape: Sequence[int]) -> Tensor:
    """rua_segment_runs_counts: int64 of the token dimensions of the RESULT's storage — the length of every run, zeros
    in padding rows — from the plan's rank table; two small launches, no atomics."""
    dev = L.require_device(rank)
    if rank.dtype != torch.int32 or rank.numel() != big.n_rows or not rank.is_contiguous():
        raise L.RuaError('runs counts: the rank table is a contiguous int32 tensor with one entry per storage row')
    counts = torch.empty(tuple(lead_shape), dtype=torch.int64, device=dev)
    if counts.numel() != small.n_rows:
        raise L.RuaError(f'runs counts: the token dimensions {tuple(lead_shape)} do not hold {small.n_rows} storage rows')
    if big.B == 0 or small.n_rows == 0:
        return counts
    starts = torch.empty(small.n_rows, dtype=torch.int32, device=dev)
    _call('runs_counts', 'rua_segment_runs_counts', dev, small.ref(), big.ref(), L.ptr(rank), L.ptr(starts), L.ptr(counts))
    return counts


# ------------------------------------------------------------------ per-sequence repeat_interleave (an extension)
def launch_repeat_plan(lay: M.Lay, counts: Tensor, cut: bool = True) -> Tuple[Tensor, Tensor]:
    """rua_segment_repeat_plan: (first int64 [storage rows of `lay`], new_lens int64 [B + 1]) from int64 counts with one
    value per storage row — one launch (two for cut sequences); the counts are read once.  first is the position of a
    token's first copy in its new sequence, -1 for a padding row; new_lens[B] is the number of invalid counts (negative or
    above 2^31 - 1; taken as 0).  cut=False withholds the workspace (the same bits from one workgroup per sequence)."""
    dev = L.require_device(counts)
    if counts.dtype != torch.int64 or counts.numel() != lay.n_rows:
        raise L.RuaError(f'repeat plan: the counts are a torch.int64 tensor with one value per storage row ({lay.n_rows}); '
                         f'got {counts.dtype} with {counts.numel()} values')
    counts = _plain(counts).contiguous()
    first = torch.empty(lay.n_rows, dtype=torch.int64, device=dev)
    if lay.B == 0:
        return first.fill_(-1), torch.zeros(1, dtype=torch.int64, device=dev)     # (the entry point returns without a launch)
    new_lens = torch.empty(lay.B + 1, dtype=torch.int64, device=dev)
    ws = _workspace('rua_repeat_ws_bytes', lay, None, None, dev, cut)
    _call('repeat_plan', 'rua_segment_repeat_plan', dev, lay.ref(), L.ptr(counts), L.ptr(first), L.ptr(new_lens),
          L.ptr(ws))
    return first, new_lens


def _repeat_table(first: Optional[Tensor], counts: Optional[Tensor], src: M.Lay, what: str) -> None:
    for t, name in ((first, 'first'), (counts, 'counts')):
        if t is not None and (t.dtype != torch.int64 or t.numel() != src.n_rows or not t.is_contiguous()):
            raise L.RuaError(f'{what}: `{name}` is a contiguous int64 tensor with one entry per storage row of the source')


def launch_repeat_move(dst: M.Lay, src: M.Lay, first: Optional[Tensor], uniform: int, data: Tensor,
                       hidden: Tuple[int, ...], out_shape: Sequence[int], out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_repeat_move: the row of every token (b, u) of a new payload of `dst` receives the bits of the source
    token whose run holds u — found in `first`, or u // uniform when first is None.  Padding rows of a padded result are
    zeros; one launch."""
    dev = L.require_device(data, first)
    if data.element_size() not in (1, 2, 4, 8):
        raise L.RuaError(f'repeat_interleave moves elements of 1, 2, 4 or 8 bytes; got {data.dtype}')
    _repeat_table(first, None, src, 'repeat move')
    if data.numel() != src.n_rows * _prod(hidden):
        raise L.RuaError(f'repeat move: the payload has {data.numel()} elements, the source layout {src.n_rows} rows of '
                         f'{_prod(hidden)}')
    data = data.contiguous()
    out = _target(out, out_shape, data.dtype, dev, 'repeat_interleave' + _LIKE_PAYLOAD)
    if out.numel() != dst.n_rows * _prod(hidden):
        raise L.RuaError(f'repeat move: the result has {out.numel()} elements, its layout {dst.n_rows} rows of '
                         f'{_prod(hidden)}')
    if out.numel() == 0:
        return out
    if data.numel() == 0:
        return out.zero_()
    rb = _prod(hidden) * data.element_size()
    _call('repeat_move', 'rua_segment_repeat_move', dev, dst.ref(), src.ref(), L.ptr(first), int(uniform), L.ptr(out),
          L.ptr(data), rb)
    return out


def launch_repeat_sum(src: M.Lay, dst: M.Lay, first: Optional[Tensor], counts: Optional[Tensor], uniform: int,
                      grad: Tensor, hidden: Tuple[int, ...], src_shape: Sequence[int],
                      out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_repeat_sum, the adjoint of the move: every token of a new payload of `src` receives the sum of the
    rows of its run in `grad` (storage of `dst`), in ascending order, accumulated in fp32 (fp64) and rounded once; tokens
    with count 0 and padding rows are zeros.  One launch, no atomics."""
    dev = L.require_device(grad, first, counts)
    code = _require_dtype(grad, L.DTYPES, 'repeat_interleave sums')
    _repeat_table(first, counts, src, 'repeat sum')
    if (first is None) != (counts is None):
        raise L.RuaError('repeat sum: `first` and `counts` come together')
    if grad.numel() != dst.n_rows * _prod(hidden) or _prod(src_shape) != src.n_rows * _prod(hidden):
        raise L.RuaError(f'repeat sum: the gradient has {grad.numel()} elements, the layout it belongs to {dst.n_rows} '
                         f'rows of {_prod(hidden)}')
    grad = grad.contiguous()
    out = _target(out, src_shape, grad.dtype, dev, 'repeat_interleave' + _LIKE_PAYLOAD)
    if out.numel() == 0:
        return out
    if grad.numel() == 0:
        return out.zero_()                              # every count was 0
    _call('repeat_sum', 'rua_segment_repeat_sum', dev, src.ref(), dst.ref(), L.ptr(first), L.ptr(counts), int(uniform),
          L.ptr(out), L.ptr(grad), _prod(hidden), code)
    return out


class _Repeat(torch.autograd.Function):
    """payload of `src` -> payload of `dst`, every token `count` times: linear, its adjoint is _RunSum with the same
    table.  Saves ONLY `first` and the caller's counts (nothing at all for an int count): no payload, no index per
    output token."""

    @staticmethod
    def forward(ctx, data: Tensor, first: Optional[Tensor], counts: Optional[Tensor], uniform: int, dst: M.Lay,
                src: M.Lay, hidden, dst_shape, src_shape):
        ctx.args = (int(uniform), dst, src, tuple(hidden), tuple(dst_shape), tuple(src_shape))
        ctx.table = first is not None
        if ctx.table:
            ctx.save_for_backward(first, counts)
        return launch_repeat_move(dst, src, first, uniform, data, hidden, dst_shape)

    @staticmethod
    def backward(ctx, grad: Tensor):
        first, counts = ctx.saved_tensors if ctx.table else (None, None)
        return (run_sum(grad, first, counts, *ctx.args),) + (None,) * 8


class _RunSum(torch.autograd.Function):
    """payload of `dst` -> payload of `src`, every token the sum of its run: the adjoint of _Repeat, and _Repeat is its
    adjoint — derivatives of every order from the two kernels."""

    @staticmethod
    def forward(ctx, grad: Tensor, first: Optional[Tensor], counts: Optional[Tensor], uniform: int, dst: M.Lay,
                src: M.Lay, hidden, dst_shape, src_shape):
        ctx.args = (int(uniform), dst, src, tuple(hidden), tuple(dst_shape), tuple(src_shape))
        ctx.table = first is not None
        if ctx.table:
            ctx.save_for_backward(first, counts)
        return launch_repeat_sum(src, dst, first, counts, uniform, grad, hidden, src_shape)

    @staticmethod
    def backward(ctx, grad: Tensor):
        first, counts = ctx.saved_tensors if ctx.table else (None, None)
        return (repeat(grad, first, counts, *ctx.args),) + (None,) * 8


def repeat(data: Tensor, first: Optional[Tensor], counts: Optional[Tensor], uniform: int, dst: M.Lay, src: M.Lay, hidden,
           dst_shape, src_shape) -> Tensor:
    L.require_device(data)
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, before the Function (as in compress()): a copy made inside forward() would carry no history
        return _Repeat.apply(data.contiguous(), first, counts, int(uniform), dst, src, tuple(hidden), tuple(dst_shape),
                             tuple(src_shape))
    return launch_repeat_move(dst, src, first, int(uniform), _plain(data), tuple(hidden), tuple(dst_shape))


def run_sum(grad: Tensor, first: Optional[Tensor], counts: Optional[Tensor], uniform: int, dst: M.Lay, src: M.Lay, hidden,
            dst_shape, src_shape) -> Tensor:
    L.require_device(grad)
    if grad.is_floating_point() and grad.requires_grad and torch.is_grad_enabled():
        return _RunSum.apply(grad.contiguous(), first, counts, int(uniform), dst, src, tuple(hidden), tuple(dst_shape),
                             tuple(src_shape))
    return launch_repeat_sum(src, dst, first, counts, int(uniform), _plain(grad), tuple(hidden), tuple(src_shape))


# ------------------------------------------------------------------ per-sequence join / unjoin along time (an extension)
class JoinPlan:
    """Everything one rua_segment_join launch needs except the payloads: the layout and storage shape of the JOINED side
    and of every part (the layouts keep their length vectors alive).  This is all the autograd Functions hold."""
    __slots__ = ('joined', 'parts', 'hidden', 'joined_shape', 'part_shapes')

    def __init__(self, joined: M.Lay, parts: Sequence[M.Lay], hidden, joined_shape, part_shapes):
        self.joined, self.parts, self.hidden = joined, tuple(parts), tuple(hidden)
        self.joined_shape, self.part_shapes = tuple(joined_shape), tuple(tuple(s) for s in part_shapes)


def _lay_array(lays: Sequence[M.Lay]):
    """`lays` as the contiguous array of rua_layout the join entry points take (copies of the structs)."""
    return (L.RuaLayout * len(lays))(*[lay.c for lay in lays])


def launch_join_lens(lays: Sequence[M.Lay], dev, want_parts: bool = False) -> Tensor:
    """rua_segment_join_lens: row 0 of the result is the summed (clamped) length of every sequence over the parts; with
    want_parts the rows 1 .. n are the parts' own lengths — one buffer, so that a caller who has to read the sums back
    reads everything in one copy.  One small launch, no ATen kernel."""
    n, B = len(lays), lays[0].B
    out = torch.empty((n + 1 if want_parts else 1, B), dtype=torch.long, device=dev)
    if B:
        _call('join_lens', 'rua_segment_join_lens', dev, _lay_array(lays), n, L.ptr(out),
              out.data_ptr() + 8 * B if want_parts else None)
    return out


def launch_unjoin_lens(joined: M.Lay, sizes: Sequence, dev, want_own: bool = False) -> Tensor:
    """rua_segment_unjoin_lens: [n, B] — row k holds the length of part k of every sequence: what `sizes[k]` (a device
    [B] int64 tensor, or an int for every sequence) asks for, clamped to what the parts before left of the sequence.
    With want_own a row n follows: the container's own lengths — one buffer, one copy for a caller who reads back."""
    n, B = len(sizes), joined.B
    out = torch.empty((n + 1 if want_own else n, B), dtype=torch.long, device=dev)
    ptrs = (ctypes.c_void_p * n)(*[L.ptr(s) if isinstance(s, Tensor) else None for s in sizes])
    adds = (ctypes.c_int64 * n)(*[0 if isinstance(s, Tensor) else int(s) for s in sizes])
    if B:
        _call('unjoin_lens', 'rua_segment_unjoin_lens', dev, joined.ref(), ptrs, adds, n, L.ptr(out),
              out.data_ptr() + 8 * n * B if want_own else None)
    return out


def launch_join(plan: JoinPlan, src, unjoin: bool):
    """rua_segment_join.  unjoin=False: `src` is the parts' payloads, the result the joined payload; unjoin=True: `src`
    is the joined payload, the result a tuple with every part's.  Rows move as bits; padding rows of every result are
    zeros; ONE launch either way."""
    srcs = [src] if unjoin else list(src)
    dev = L.require_device(*srcs)
    dtype = srcs[0].dtype
    if srcs[0].element_size() not in (1, 2, 4, 8):
        raise L.RuaError(f'join moves elements of 1, 2, 4 or 8 bytes; got {dtype}')
    want = [plan.joined_shape] if unjoin else list(plan.part_shapes)
    if len(srcs) != len(want) or any(s.dtype != dtype or s.numel() != _prod(w) for s, w in zip(srcs, want)):
        raise L.RuaError('join: the payloads do not fit the plan (one per part, of one dtype, of the planned storage shapes)')
    srcs = [s.contiguous() for s in srcs]
    outs = [torch.empty(s, dtype=dtype, device=dev) for s in (plan.part_shapes if unjoin else [plan.joined_shape])]
    joined_data, part_data = (srcs[0], outs) if unjoin else (outs[0], srcs)
    n = len(plan.parts)
    ptrs = (ctypes.c_void_p * n)(*[L.ptr(t) if t.numel() else None for t in part_data])
    rb = _prod(plan.hidden) * srcs[0].element_size()
    _call('unjoin' if unjoin else 'join', 'rua_segment_join', dev, plan.joined.ref(), _lay_array(plan.parts), n,
          L.ptr(joined_data) if joined_data.numel() else None, ptrs, rb, int(bool(unjoin)))
    return tuple(outs) if unjoin else outs[0]


class _Join(torch.autograd.Function):
    """payloads of the parts -> payload of the joined side: a permutation of rows plus zeros, linear; its adjoint is
    _Unjoin with the same plan.  Holds ONLY the plan (length vectors and layout metadata): no payload, no index."""

    @staticmethod
    def forward(ctx, plan: JoinPlan, *datas: Tensor):
        ctx.plan = plan
        return launch_join(plan, datas, False)

    @staticmethod
    def backward(ctx, grad: Tensor):
        return (None,) + tuple(unjoin(grad, ctx.plan))


class _Unjoin(torch.autograd.Function):
    """payload of the joined side -> payloads of the parts: the adjoint of _Join, and _Join is its adjoint (dropped
    tokens and padding rows get exact zeros) — derivatives of every order from the one kernel."""

    @staticmethod
    def forward(ctx, plan: JoinPlan, data: Tensor):
        ctx.plan = plan
        return launch_join(plan, data, True)

    @staticmethod
    def backward(ctx, *grads: Tensor):
        return None, join(grads, ctx.plan)


def join(datas: Sequence[Tensor], plan: JoinPlan) -> Tensor:
    L.require_device(*datas)
    if torch.is_grad_enabled() and any(d.is_floating_point() and d.requires_grad for d in datas):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _Join.apply(plan, *[d.contiguous() for d in datas])
    return launch_join(plan, [_plain(d) for d in datas], False)


def unjoin(data: Tensor, plan: JoinPlan) -> Tuple[Tensor, ...]:
    L.require_device(data)
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        return _Unjoin.apply(plan, data.contiguous())
    return launch_join(plan, _plain(data), True)


# ------------------------------------------------------------------ per-sequence sliding-window pooling (an extension)
_WINDOW_SUPPORT = 'window_pool supports'
WINDOW_MODES = {'sum': L.SUM, 'mean': L.MEAN, 'max': L.MAX}
_WINDOW_NAMES = {L.SUM: 'sum', L.MEAN: 'mean', L.MAX: 'max', L.WINDOW_TAKE: 'take'}


class WindowPlan:
    """Everything a rua_segment_window_pool / _spread launch needs except the payloads: the layout and storage shape of
    the POOLED side and of the BIG side (the layouts keep their length vectors alive), the window and the step.  This
    is all the sum and mean Functions hold."""
    __slots__ = ('small', 'big', 'hidden', 'small_shape', 'big_shape', 'K', 'S')

    def __init__(self, small: M.Lay, big: M.Lay, hidden, small_shape, big_shape, K: int, S: int):
        self.small, self.big, self.hidden = small, big, tuple(hidden)
        self.small_shape, self.big_shape, self.K, self.S = tuple(small_shape), tuple(big_shape), int(K), int(S)


def launch_window_lens(lay: M.Lay, K: int, S: int, ceil_mode: bool, dev, want_own: bool = False) -> Tensor:
    """rua_window_lens: row 0 of the result is the number of windows of every sequence; with want_own a row 1 follows,
    the container's own lengths — one buffer, one copy for a caller who reads back.  One small launch, no ATen kernel."""
    B = lay.B
    out = torch.empty((2 if want_own else 1, B), dtype=torch.long, device=dev)
    if B:
        _call('window_lens', 'rua_window_lens', dev, lay.ref(), int(K), int(S), int(bool(ceil_mode)), L.ptr(out),
              out.data_ptr() + 8 * B if want_own else None)
    return out


def _window_payload(src: Tensor, shape, what: str) -> int:
    code = _require_dtype(src, L.SCAN_DTYPES, _WINDOW_SUPPORT)
    if src.numel() != _prod(shape):
        raise L.RuaError(f'window_pool: the {what} does not fit the plan (storage shape {tuple(shape)}; got '
                         f'{tuple(src.shape)})')
    return code


def _window_arg(arg: Optional[Tensor], plan: WindowPlan, dev) -> Tensor:
    if arg is None or arg.dtype != torch.uint8 or arg.numel() != _prod(plan.small_shape) or not arg.is_contiguous():
        raise L.RuaError('window_pool: the arg table is a contiguous uint8 tensor shaped like the pooled payload')
    L.require_device(arg)
    return arg


def launch_window_pool(plan: WindowPlan, data: Tensor, mode: int, arg: Optional[Tensor] = None,
                       want_arg: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """rua_segment_window_pool: payload of `plan.big` -> (payload of `plan.small`, arg).  mode MAX with want_arg also
    returns the uint8 table of the winners' offsets; mode WINDOW_TAKE reads `arg`.  ONE launch; padding rows of a
    padded result are zeros."""
    code = _window_payload(data, plan.big_shape, 'payload')
    dev = data.device
    data = data.contiguous()
    if mode == L.WINDOW_TAKE:
        arg = _window_arg(arg, plan, dev)
    else:
        arg = torch.empty(plan.small_shape, dtype=torch.uint8, device=dev) if want_arg and mode == L.MAX else None
    out = torch.empty(plan.small_shape, dtype=data.dtype, device=dev)
    if out.numel():
        _call('window_' + _WINDOW_NAMES[mode], 'rua_segment_window_pool', dev, plan.big.ref(), plan.small.ref(),
              L.ptr(data) if data.numel() else None, L.ptr(out), L.ptr(arg), _prod(plan.hidden), plan.K, plan.S, mode,
              code)
    return out, arg


def launch_window_spread(plan: WindowPlan, grad: Tensor, mode: int, arg: Optional[Tensor] = None) -> Tensor:
    """rua_segment_window_spread, the adjoint: payload of `plan.small` -> payload of `plan.big`; tokens in no window and
    padding rows get exact zeros.  ONE launch (also where nothing was pooled: the zeros are the kernel's)."""
    code = _window_payload(grad, plan.small_shape, 'pooled payload')
    dev = grad.device
    grad = grad.contiguous()
    by_arg = mode in (L.MAX, L.WINDOW_TAKE)
    if by_arg:
        arg = _window_arg(arg, plan, dev)
    out = torch.empty(plan.big_shape, dtype=grad.dtype, device=dev)
    if out.numel():
        _call('window_spread_' + _WINDOW_NAMES[mode], 'rua_segment_window_spread', dev, plan.small.ref(), plan.big.ref(),
              L.ptr(grad) if grad.numel() else None, L.ptr(arg) if by_arg and arg.numel() else None, L.ptr(out),
              _prod(plan.hidden), plan.K, plan.S, mode, code)
    return out


class _WindowPool(torch.autograd.Function):
    """payload of the big side -> payload of the pooled side.  sum and mean are linear and hold ONLY the plan (length
    vectors and layout metadata); max keeps the uint8 table of the winners' offsets — one byte per output element, no
    payload, no int64 index — and, given that table, is the linear map `take`.  The adjoint is _WindowSpread."""

    @staticmethod
    def forward(ctx, data: Tensor, arg: Optional[Tensor], plan: WindowPlan, mode: int):
        out, arg = launch_window_pool(plan, data, mode, arg, want_arg=True)
        ctx.plan, ctx.mode = plan, mode
        if arg is not None:
            ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, grad: Tensor):
        arg = ctx.saved_tensors[0] if ctx.saved_tensors else None
        return window_spread(grad, arg, ctx.plan, ctx.mode), None, None, None


class _WindowSpread(torch.autograd.Function):
    """payload of the pooled side -> payload of the big side: the adjoint of _WindowPool, and _WindowPool (max: as
    `take`) is its adjoint — derivatives of every order from the two kernels."""

    @staticmethod
    def forward(ctx, grad: Tensor, arg: Optional[Tensor], plan: WindowPlan, mode: int):
        ctx.plan, ctx.mode = plan, mode
        if arg is not None:
            ctx.save_for_backward(arg)
        return launch_window_spread(plan, grad, mode, arg)

    @staticmethod
    def backward(ctx, grad: Tensor):
        arg = ctx.saved_tensors[0] if ctx.saved_tensors else None
        mode = L.WINDOW_TAKE if ctx.mode in (L.MAX, L.WINDOW_TAKE) else ctx.mode
        return window_pool(grad, ctx.plan, mode, arg), None, None, None


def window_pool(data: Tensor, plan: WindowPlan, mode: int, arg: Optional[Tensor] = None) -> Tensor:
    L.require_device(data)
    if data.is_floating_point() and data.requires_grad and torch.is_grad_enabled():
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _WindowPool.apply(data.contiguous(), arg, plan, mode)
    return launch_window_pool(plan, _plain(data), mode, arg)[0]


def window_spread(grad: Tensor, arg: Optional[Tensor], plan: WindowPlan, mode: int) -> Tensor:
    L.require_device(grad)
    if grad.is_floating_point() and grad.requires_grad and torch.is_grad_enabled():
        return _WindowSpread.apply(grad.contiguous(), arg, plan, mode)
    return launch_window_spread(plan, _plain(grad), mode, arg)


# ------------------------------------------------------------------ per-sequence argmax / argmin (an extension)
_ARG_SUPPORT = 'argmax / argmin support'


def launch_argreduce(lay: M.Lay, data: Tensor, op: int, hidden: Tuple[int, ...], want_values: bool = True,
                     cut: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    """rua_segment_argreduce: (values or None, index), both [B, *hidden] and written completely by the call — one launch
    (two for cut sequences), one read of the payload.  cut=False withholds the workspace (the same bits from one
    workgroup per unit: a developer A/B)."""
    code = _require_dtype(data, L.SCAN_DTYPES, _ARG_SUPPORT)
    if op not in (L.MAX, L.MIN):
        raise L.RuaError('argreduce: the operator is MAX or MIN')
    dev, H = data.device, _prod(hidden)
    ws = _workspace('rua_argreduce_ws_bytes', lay, H, code, dev, cut)
    data = data.contiguous()
    shape = (lay.B,) + tuple(hidden)
    index = torch.empty(shape, dtype=torch.int64, device=dev)
    values = torch.empty(shape, dtype=data.dtype, device=dev) if want_values else None
    name = ('seq_max' if op == L.MAX else 'seq_min') if want_values else ('argmax' if op == L.MAX else 'argmin')
    _call(name, 'rua_segment_argreduce', dev, lay.ref(), L.ptr(data), L.ptr(values), L.ptr(index), H, code, op, L.ptr(ws))
    return values, index


def _index_arg(lay: M.Lay, index: Tensor, hidden: Tuple[int, ...], dev) -> Tensor:
    L.require_device(index)
    if index.dtype != torch.int64 or index.device != dev or tuple(index.shape) != (lay.B,) + tuple(hidden):
        raise L.RuaError('take / put: the index is a [B, *hidden] int64 tensor on the payload\'s device')
    return index.contiguous()


def launch_take(lay: M.Lay, data: Tensor, index: Tensor, hidden: Tuple[int, ...]) -> Tensor:
    """rua_segment_take: out[b, h] = data[row(b, index[b, h]), h], 0 where the position names no token of b."""
    code = _require_dtype(data, L.SCAN_DTYPES, _ARG_SUPPORT)
    dev = data.device
    index = _index_arg(lay, index, hidden, dev)
    data = data.contiguous()
    out = torch.empty((lay.B,) + tuple(hidden), dtype=data.dtype, device=dev)
    _call('take', 'rua_segment_take', dev, lay.ref(), L.ptr(data), L.ptr(index), L.ptr(out), _prod(hidden), code)
    return out


def launch_put(lay: M.Lay, src: Tensor, index: Tensor, hidden: Tuple[int, ...], shape: Sequence[int],
               out: Optional[Tensor] = None) -> Tensor:
    """rua_segment_put: a payload of storage shape `shape` that holds src[b, h] at token index[b, h] of sequence b and
    zeros everywhere else, padding rows included — written completely by the call (no pre-zeroing)."""
    code = _require_dtype(src, L.SCAN_DTYPES, _ARG_SUPPORT)
    dev = src.device
    index = _index_arg(lay, index, hidden, dev)
    if tuple(src.shape) != (lay.B,) + tuple(hidden):
        raise L.RuaError('put: the source is a [B, *hidden] tensor')
    src = src.contiguous()
    out = _target(out, shape, src.dtype, dev, 'put target must be contiguous, of the source dtype and of the payload shape')
    _call('put', 'rua_segment_put', dev, lay.ref(), L.ptr(src), L.ptr(index), L.ptr(out), _prod(hidden), code)
    return out


class _ArgReduce(torch.autograd.Function):
    """(values, index) of every sequence's largest / smallest token.  Saves ONLY the [B, *H] index; the gradient goes
    to the chosen token whole (torch.max(dim)'s rule, not torch.segment_reduce's split among ties): put(grad, index)."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, op: int, hidden):
        values, index = launch_argreduce(lay, data, op, hidden)
        ctx.lay, ctx.hidden, ctx.shape = lay, tuple(hidden), tuple(data.shape)
        ctx.save_for_backward(index)
        ctx.mark_non_differentiable(index)
        return values, index

    @staticmethod
    def backward(ctx, grad: Tensor, _grad_index):
        index, = ctx.saved_tensors
        return put(grad, index, ctx.lay, ctx.hidden, ctx.shape), None, None, None


class _Put(torch.autograd.Function):
    """src [B, *H] -> payload: linear in src, its adjoint is take at the same index."""

    @staticmethod
    def forward(ctx, src: Tensor, index: Tensor, lay: M.Lay, hidden, shape):
        ctx.lay, ctx.hidden = lay, tuple(hidden)
        ctx.save_for_backward(index)
        return launch_put(lay, src, index, hidden, shape)

    @staticmethod
    def backward(ctx, grad: Tensor):
        index, = ctx.saved_tensors
        return take(grad, index, ctx.lay, ctx.hidden), None, None, None, None


class _Take(torch.autograd.Function):
    """payload -> [B, *H]: linear in the payload, its adjoint is put at the same index."""

    @staticmethod
    def forward(ctx, data: Tensor, index: Tensor, lay: M.Lay, hidden):
        ctx.lay, ctx.hidden, ctx.shape = lay, tuple(hidden), tuple(data.shape)
        ctx.save_for_backward(index)
        return launch_take(lay, data, index, hidden)

    @staticmethod
    def backward(ctx, grad: Tensor):
        index, = ctx.saved_tensors
        return put(grad, index, ctx.lay, ctx.hidden, ctx.shape), None, None, None


def _wants_grad(t: Tensor) -> bool:
    return t.is_floating_point() and t.requires_grad and torch.is_grad_enabled()


def argreduce(data: Tensor, lay: M.Lay, op: int, hidden, want_values: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    _require_dtype(data, L.SCAN_DTYPES, _ARG_SUPPORT)
    if want_values and _wants_grad(data):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _ArgReduce.apply(data.contiguous(), lay, op, tuple(hidden))
    return launch_argreduce(lay, _plain(data), op, tuple(hidden), want_values)


def put(src: Tensor, index: Tensor, lay: M.Lay, hidden, shape) -> Tensor:
    _require_dtype(src, L.SCAN_DTYPES, _ARG_SUPPORT)
    if _wants_grad(src):
        return _Put.apply(src.contiguous(), index, lay, tuple(hidden), tuple(shape))
    return launch_put(lay, _plain(src), index, tuple(hidden), tuple(shape))


def take(data: Tensor, index: Tensor, lay: M.Lay, hidden) -> Tensor:
    _require_dtype(data, L.SCAN_DTYPES, _ARG_SUPPORT)
    if _wants_grad(data):
        return _Take.apply(data.contiguous(), index, lay, tuple(hidden))
    return launch_take(lay, _plain(data), index, tuple(hidden))


# ------------------------------------------------------------------ per-sequence stable sort / reorder (an extension)
_SORT_SUPPORT = 'sort / argsort support'


def launch_sort(lay: M.Lay, data: Tensor, descending: bool, hidden: Tuple[int, ...],
                want_values: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    """rua_segment_sort: (values or None, indices), both of the storage shape of `data` and written completely by the
    call — padding rows as zeros.  One launch for sequences up to a block (rua_sort_block_len), one plus the merge passes
    of the length bound for longer ones; nothing is read back."""
    code = _require_dtype(data, L.SCAN_DTYPES, _SORT_SUPPORT)
    dev, H = data.device, _prod(hidden)
    if data.numel() != lay.n_rows * H:
        raise L.RuaError(f'sort: the payload has {data.numel()} elements, its layout {lay.n_rows} rows of {H}')
    data = data.contiguous()
    indices = torch.empty(tuple(data.shape), dtype=torch.int64, device=dev)
    values = torch.empty_like(data) if want_values else None
    if data.numel() == 0:
        return values, indices
    ws = _workspace('rua_sort_ws_bytes', lay, H, code, dev)
    _call('sort' if want_values else 'argsort', 'rua_segment_sort', dev, lay.ref(), L.ptr(data), L.ptr(values),
          L.ptr(indices), H, code, int(bool(descending)), L.ptr(ws))
    return values, indices


def launch_reorder(lay: M.Lay, data: Tensor, index: Tensor, hidden: Tuple[int, ...], per_row: bool,
                   inverse: bool) -> Tensor:
    """rua_segment_reorder: a new payload of the storage shape of `data` — the gather out[b, t] = data[b, index[b, t]]
    or, with `inverse`, the scatter out[b, index[b, t]] = data[b, t]; per row (`index` holds one position per storage
    row) or per element (one per element).  Bits move; positions outside a sequence give zeros; padding rows are zeros."""
    dev = L.require_device(data, index)
    if data.element_size() not in (1, 2, 4, 8):
        raise L.RuaError(f'reorder moves elements of 1, 2, 4 or 8 bytes; got {data.dtype}')
    H = _prod(hidden)
    if data.numel() != lay.n_rows * H or index.dtype != torch.int64 or index.numel() != lay.n_rows * (1 if per_row else H):
        raise L.RuaError(f'reorder: the payload has {data.numel()} elements and the index {index.numel()} ({index.dtype}); '
                         f'the layout has {lay.n_rows} rows of {H}')
    data, index = data.contiguous(), _plain(index).contiguous()
    out = torch.empty_like(data)
    if out.numel() == 0:
        return out
    flat = data.view(torch.uint8) if data.dtype == torch.bool else data
    _call('reorder_inverse' if inverse else 'reorder', 'rua_segment_reorder', dev, lay.ref(), L.ptr(flat), L.ptr(index),
          L.ptr(out), H, data.element_size(), int(bool(per_row)), int(bool(inverse)))
    return out


class _Reorder(torch.autograd.Function):
    """payload -> payload permuted inside every sequence: linear, its adjoint is the same permutation the other way
    round (gather <-> scatter), so derivatives of every order exist.  Saves ONLY the index."""

    @staticmethod
    def forward(ctx, data: Tensor, index: Tensor, lay: M.Lay, hidden, per_row: bool, inverse: bool):
        ctx.args = (lay, tuple(hidden), bool(per_row), bool(inverse))
        ctx.save_for_backward(index)
        return launch_reorder(lay, data, index, hidden, per_row, inverse)

    @staticmethod
    def backward(ctx, grad: Tensor):
        index, = ctx.saved_tensors
        lay, hidden, per_row, inverse = ctx.args
        return reorder(grad, index, lay, hidden, per_row, not inverse), None, None, None, None, None


class _Sort(torch.autograd.Function):
    """(values, indices) of every sequence in order.  Saves ONLY the indices; the backward scatters the gradient back
    through them per element (reorder, inverse), whose own backward is the gather and so on."""

    @staticmethod
    def forward(ctx, data: Tensor, lay: M.Lay, descending: bool, hidden):
        values, indices = launch_sort(lay, data, descending, hidden)
        ctx.lay, ctx.hidden = lay, tuple(hidden)
        ctx.save_for_backward(indices)
        ctx.mark_non_differentiable(indices)
        return values, indices

    @staticmethod
    def backward(ctx, grad: Tensor, _grad_indices):
        indices, = ctx.saved_tensors
        return reorder(grad, indices, ctx.lay, ctx.hidden, False, True), None, None, None


def sort(data: Tensor, lay: M.Lay, descending: bool, hidden, want_values: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    _require_dtype(data, L.SCAN_DTYPES, _SORT_SUPPORT)
    if want_values and _wants_grad(data):
        # contiguous HERE, before the Function (as in reduce()): a copy made inside forward() would carry no history
        return _Sort.apply(data.contiguous(), lay, bool(descending), tuple(hidden))
    return launch_sort(lay, _plain(data), bool(descending), tuple(hidden), want_values)


def reorder(data: Tensor, index: Tensor, lay: M.Lay, hidden, per_row: bool, inverse: bool) -> Tensor:
    L.require_device(data, index)
    if _wants_grad(data):
        return _Reorder.apply(data.contiguous(), index, lay, tuple(hidden), bool(per_row), bool(inverse))
    return launch_reorder(lay, _plain(data), index, tuple(hidden), bool(per_row), bool(inverse))


# ------------------------------------------------------------------ scatter-sum of rows (adjoint of a row gather)
def index_buckets(index: Tensor, S: int) -> Tuple[Tensor, Tensor]:
    """(counts[S], perm[M]): the entries of `index` bucketed by destination, every bucket in ascending entry order
    (rua_index_buckets: a stable LSD radix sort, deterministic for any fan-in)."""
    dev = L.require_device(index)
    lib = L.load()
    index = M._as_lens(index)
    m = index.numel()
    counts = torch.empty(S, dtype=torch.long, device=dev)
    off = torch.empty(S, dtype=torch.long, device=dev)
    perm = torch.empty(m, dtype=torch.long, device=dev)
    ws = torch.empty(lib.rua_bucket_ws_elems(m, S), dtype=torch.long, device=dev)
    L.check(lib.rua_index_buckets(L.ptr(index), m, S, L.ptr(counts), L.ptr(off), L.ptr(perm), L.ptr(ws),
                                  L.stream_ptr(dev)), 'rua_index_buckets')
    M._memo_put(counts, 'off', off)
    return counts, perm


class _ScatterSumRows(torch.autograd.Function):
    """out[s] = sum of rows[i] over index[i] == s; adjoint: the gather rows[index]."""

    @staticmethod
    def forward(ctx, rows: Tensor, index: Tensor, n_out: int):
        ctx.save_for_backward(index)        # (saved, not a plain attribute: autograd then checks its version)
        return scatter_sum_rows(rows.detach(), index, n_out)

    @staticmethod
    def backward(ctx, g: Tensor):
        index, = ctx.saved_tensors
        return gather_rows(g.contiguous(), index), None, None


class _GatherRows(torch.autograd.Function):
    """out[i] = rows[index[i]] (zeros where index[i] is out of range); adjoint: the scatter-sum."""

    @staticmethod
    def forward(ctx, rows: Tensor, index: Tensor):
        ctx.save_for_backward(index)
        ctx.n = int(rows.size(0))
        plan = MovePlan(M.lay_list(None, index), M.lay_flat(ctx.n), (index.numel(),) + tuple(rows.shape[1:]), fill=0,
                        name='gather_rows')
        return launch_move(plan, rows.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        index, = ctx.saved_tensors
        return scatter_sum(g.contiguous(), index, ctx.n), None


def gather_rows(rows: Tensor, index: Tensor) -> Tensor:
    """rows[index] through the mover; recorded by autograd when `rows` carries a graph (second-order gradients)."""
    if rows.requires_grad and torch.is_grad_enabled():
        return _GatherRows.apply(rows, index)
    return _GatherRows.forward(_NoCtx(), rows, index)


def scatter_sum(rows: Tensor, index: Tensor, n_out: int) -> Tensor:
    """scatter_sum_rows, recorded by autograd when `rows` carries a graph (second-order gradients)."""
    if rows.requires_grad and torch.is_grad_enabled():
        return _ScatterSumRows.apply(rows, index, n_out)
    return scatter_sum_rows(rows, index, n_out)


class _NoCtx:
    """Stands in for an autograd context when a Function's forward is run for its value only."""

    def save_for_backward(self, *tensors) -> None:
        pass


def scatter_sum_rows(rows: Tensor, index: Tensor, n_out: int) -> Tensor:
    """out[s] = sum of rows[i] over the entries i with index[i] == s, s < n_out (rows nobody names are 0)."""
    hidden = tuple(rows.shape[1:])
    counts, perm = index_buckets(index, n_out)
    lay = M.lay_cat(counts, n_out, int(rows.size(0)))
    lay.heavy_tail = True
    if rows.dtype in L.INT_DTYPES:        # (integer payloads carry no gradient: the integer reducer, for completeness)
        out = torch.empty((n_out,) + hidden, dtype=rows.dtype, device=rows.device)
        H = _prod(hidden)
        split, ws = int_split_workspace(int(rows.size(0)), H, rows.dtype, rows.device)
        L.check(L.load().rua_segment_reduce(lay.ref(), L.ptr(perm), L.ptr(rows.contiguous()), L.ptr(out), H,
                                            L.INT_DTYPES[rows.dtype], L.SUM, 0, 0, None, split, L.ptr(ws), None,
                                            L.stream_ptr(rows.device)), 'rua_segment_reduce')
        return out
    return launch_reduce(lay, rows, L.SUM, perm=perm, hidden=hidden, reference_initial=False, name='scatter')


# ------------------------------------------------------------------ a row scatter autograd sees (core/set.py)
def setitem_backward(plan: MovePlan, grad: Tensor, hidden: Tuple[int, ...], want_value: bool, want_raw: bool):
    """rua_setitem_backward for the scatter `plan` describes: (grad_value [M, *hidden] or None, grad_raw or None)."""
    dev = L.require_device(grad)
    grad = grad.contiguous()
    m, n_rows = plan.dst.n_rows, plan.src.n_rows
    rb = _prod(hidden) * grad.element_size() if n_rows else 0
    g_value = torch.empty((m,) + hidden, dtype=grad.dtype, device=dev) if want_value else None
    g_raw = torch.empty_like(grad) if want_raw else None
    if rb == 0 or (m == 0 and not want_raw):
        return (g_value.zero_() if want_value and g_value.numel() else g_value), g_raw
    _call(plan.name + '_bwd', 'rua_setitem_backward', dev, plan.dst.ref(), plan.src.ref(), L.ptr(grad), L.ptr(g_value),
          L.ptr(g_raw), rb, 0)
    return g_value, g_raw


def _sum_rows(g: Tensor, n_seq: int, per_seq: int, hidden: Tuple[int, ...]) -> Tensor:
    """[n_seq * per_seq, *hidden] -> [n_seq, *hidden]: the sum over each run of per_seq rows, by the segmented reducer
    (its split path keeps a long sum deterministic).  Differentiable (the adjoint is the reducer's broadcast)."""
    lay = M.lay_cat(None, n_seq, n_seq * per_seq, len_add=per_seq)
    return reduce(g.reshape((n_seq * per_seq,) + hidden), lay, L.SUM, hidden, None)


def _sum_to_value(g: Tensor, lead: Tuple[int, ...], hidden: Tuple[int, ...], vshape: Tuple[int, ...]) -> Tensor:
    """The adjoint of broadcasting `value` [vshape] to [*lead, *hidden], applied to g [M, *hidden].  A broadcast along
    the ROWS is summed by the library's reducer; what remains is a broadcast inside a row (sum_to_size)."""
    full = tuple(lead) + tuple(hidden)
    if tuple(vshape) == full:
        return g.reshape(vshape)
    k = len(lead)
    v = (1,) * (len(full) - len(vshape)) + tuple(vshape)
    summed = [i for i in range(k) if v[i] == 1 and lead[i] != 1]
    live = [i for i in range(k) if lead[i] != 1]
    g = g.reshape(full)
    if summed and g.numel():
        cut = len(summed)
        if summed == live[:cut]:              # a leading run of row dims ([H], [1, H], 0-d ...): ONE sequence per kept row
            keep = tuple(lead[i] for i in live[cut:])
            rest = keep + tuple(hidden)
            g = _sum_rows(g, 1, _prod(lead) // _prod(keep), rest)
            g = g.reshape(tuple(1 if i in summed else lead[i] for i in range(k)) + tuple(hidden))
        elif summed == live[len(live) - cut:]:  # a trailing run of row dims: one sequence per leading row
            n_seq = _prod(lead[i] for i in live[:len(live) - cut])
            g = _sum_rows(g, n_seq, _prod(lead) // n_seq, tuple(hidden))
            g = g.reshape(tuple(1 if i in summed else lead[i] for i in range(k)) + tuple(hidden))
        # (row dims broadcast in the middle of others: left to sum_to_size below)
    return g.sum_to_size(vshape) if tuple(g.shape) != tuple(vshape) else g


class _ScatterRows(torch.autograd.Function):
    """rows_of(raw)[key] = value, in place, recorded by autograd (core/set.py:21-92).  Forward: the row mover in scatter
    mode into `raw` itself (mark_dirty).  Backward: rua_setitem_backward — one index resolution serves the gather of
    d/d value and the zeroing of d/d raw.  `value` arrives in its own shape and is broadcast HERE, so that the sum over
    broadcast rows is the library's reducer, not the backward of an ATen expand.
    What the backward computes follows `ctx.needs_input_grad`, i.e. which inputs REQUIRE grad, not which gradients the
    caller asked for: with a storage that requires grad, `torch.autograd.grad(out, [value])` still pays the copy and the
    zeroing of d/d raw, and the engine drops the result.  Only a storage that does not require grad skips them.
    `flat_fn` is kept on the node of the written storage, so it must not reference that storage (or a container that
    holds it): that would be a reference cycle only Python's cyclic collector frees."""

    @staticmethod
    def forward(ctx, raw: Tensor, value: Tensor, plan: MovePlan, lead: Tuple[int, ...], flat_fn, row_dims: int = 1):
        hidden = tuple(raw.shape[row_dims:])       # (the first row_dims dims of raw enumerate its storage rows)
        ctx.row_dims = row_dims
        ctx.plan, ctx.lead, ctx.hidden, ctx.flat_fn = plan, tuple(lead), hidden, flat_fn
        ctx.vshape = tuple(value.shape)
        ctx.save_for_backward(*[t for t in plan.dst.keep if t is not None])    # (saved: autograd checks the keys' versions)
        m = plan.dst.n_rows
        if m and plan.src.n_rows:
            rows = value.detach().expand(tuple(lead) + hidden).reshape((m,) + hidden)
            launch_move(plan, rows, out=raw.detach())
        ctx.mark_dirty(raw)
        return raw

    @staticmethod
    def backward(ctx, grad: Tensor):
        _ = ctx.saved_tensors                   # raises if a key tensor was modified in place since the forward
        plan = ctx.plan
        want_raw, want_value = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if torch.is_grad_enabled() and grad.requires_grad:
            # a graph of this backward is being recorded (create_graph=True): torch's setitem differentiates any number of
            # times, so here the two gradients are spelled with differentiable pieces of the library — the row gather
            # (whose adjoint is the scatter-sum) and this very Function with the value 0 — and the recursion gives every order
            g_value = g_raw = None
            if want_value:
                n_rows = plan.src.n_rows
                rows = gather_rows(grad.reshape((n_rows,) + ctx.hidden), ctx.flat_fn().reshape(-1))
                g_value = _sum_to_value(rows, ctx.lead, ctx.hidden, ctx.vshape)
            if want_raw:
                zero = torch.zeros((), dtype=grad.dtype, device=grad.device)
                g_raw = _ScatterRows.apply(grad.clone(), zero, plan, ctx.lead, ctx.flat_fn, ctx.row_dims)
            return g_raw, g_value, None, None, None, None
        g_value, g_raw = setitem_backward(plan, grad.detach(), ctx.hidden, want_value, want_raw)
        if want_value:
            with torch.no_grad():
                g_value = _sum_to_value(g_value, ctx.lead, ctx.hidden, ctx.vshape)
        return g_raw, g_value, None, None, None, None


def scatter_rows(raw: Tensor, value: Tensor, plan: MovePlan, lead: Sequence[int], flat_fn, row_dims: int = 1) -> None:
    """The write of `_ScatterRows`; `flat_fn()` -> the non-negative flat storage rows of the keys (rows >= n_rows for a
    key that names no token), only asked for when a second derivative is taken."""
    _ScatterRows.apply(raw, value, plan, tuple(lead), flat_fn, row_dims)
