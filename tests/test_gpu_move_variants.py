"""The row mover's VARIANTS on the GPU (csrc/rua_move.hip, planned by csrc/rua_move_plan.h), one small exact case each.
tests/test_gpu_move_plan.py runs every kernel family once, all with SCATTER=0, NT=0, plain blockIdx order, the time maps
T_SHIFT / T_ROLL and host-known lengths; this module runs what that leaves out.  Every case goes through the public
surface under the dispatch trace with the spy of test_gpu_move_plan on rua_move_rows, and asserts three things: the
trace record equals the dry record (rua_debug_move_plan with the same arguments), the record carries the case's words,
and the whole result — for a scatter the whole storage — equals, bit for bit, a plain torch indexing construction on
the CPU from the lengths.  Payloads are seeded random bits over the full range of the element's integer type.

Covered:
* XCD span (RUA_MOVE_XCD_SPAN_ON ORed into the one mover call the case is about, at tile counts >= 9 that are no
  multiple of 8, so that the rounded grid has surplus workgroups): pack_tile_lds_kernel both ways, pack_tile_vec_kernel
  both ways (the full grid P -> L included), pack_roll_steps_kernel, pack_roll_tile_kernel, move_rows_narrow_kernel,
  move_rows_span_kernel, move_rows_kernel (TROWS=16, TAIL8=1, SCATTER=1) — and one crossing of MOVE_SPAN_MIN_TILES with
  no flag at all (`natural_*`: C.left() at 1 KiB rows just above and just below 2 048 tiles).
* NT=1 (RUA_MOVE_NT_ON) on the forms that keep their routing under the flag: seq_copy_kernel, move_rows_narrow_kernel
  (VEC 8 and 2), move_rows_span_kernel, move_rows_kernel (VEC=16 TROWS=16, VEC=2, TAIL8=1, RPT=4, SCATTER=1).
* SCATTER=1 through `z[(bp, tp)] = v` on a C, an L and a P at five widths (the one-vector rows, 1 KiB rows, 26-byte
  rows, the 1 000-byte tail form one row into its storage) and through `z[key] = v` with a container and a tensor key.
* R = 2 / 4 / 8 of pack_tile_lds_kernel (P.cat() at 64 / 32 / 16-byte rows).
* T_REV_S (rev, last), T_REV_D (the gradient of rev), T_ROLL with pad_row = 0 (L.roll / R.roll), T_SHIFT with an
  argument and len_add (trunc, head) through the narrow, span, rows and roll-tile kernels, over every container for
  which the operation launches the mover (L.trunc / R.trunc / L.head / P.head are views and have no case).
* Lengths that live on the device only (`ta.C(data, lens_on_device)`).

Not covered, and why:
* seq_copy_kernel and the RPT=4 variant of move_rows_kernel never span (rua_move_plan.h: NEVER_SPAN): no span case.
* The tile kernels have no NT variant; pack_roll_steps_kernel NT=1 needs 512 MiB of PackedSequence, because
  RUA_MOVE_NT_ON reroutes the call: left out.
* A non-zero `phase` of the shifted windows.  R > 1 is taken only where the batch-major side is the destination
  (P.cat()); no cast takes `out=`, the destination is always a fresh allocation, and those start on a 128-byte line.  In
  the other direction (pack() of a C over a view at a storage offset) the offset payload is the plan's `major`, but the
  plan gives a pack R = 1.  So the three cases assert R and `phase=0`: a non-zero phase is unreachable from Python."""
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, host_sort
from test_gpu_move_plan import FILL, _expect, _lens, _rows, _traced
from test_move_plan import KERNELS
from torchrua_amd import _lib as K

gpu = pytest.mark.gpu
SPAN, NT = K.MOVE_XCD_SPAN_ON, K.MOVE_NT_ON
SPANNING = ('move_rows_kernel', 'move_rows_narrow_kernel', 'move_rows_span_kernel', 'pack_tile_lds_kernel',
            'pack_tile_vec_kernel', 'pack_roll_tile_kernel', 'pack_roll_steps_kernel')      # the seven that print per_xcd
I64, I16, F32, BF16, F64 = torch.int64, torch.int16, torch.float32, torch.bfloat16, torch.float64
INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Case(NamedTuple):
    B: int
    lo: int
    hi: int
    hidden: Tuple[int, ...]
    dtype: torch.dtype
    src: str                     # the container the operation is called on: C / L / R / P
    op: str
    arg: object = 0
    flags: int = 0               # developer flags ORed into the one mover call the case is about
    want: Optional[str] = None   # the kernel and the KEY=value words its record must carry; None: whatever the plan says
    span: bool = False           # per_xcd != 0, over a tile count that is no multiple of 8
    offset: bool = False         # the payload one row into its storage
    empty: bool = False
    phase: Optional[int] = None


ROWS16 = 'move_rows_kernel VEC=16 SCATTER=0 RPT=1 TROWS=16 TAIL8=0'
CASES = {
    # ---- XCD span, flag forced: the shape of the test_gpu_move_plan case of the same form, B changed where its tile
    # count was a multiple of 8
    'span_lds_pack': Case(6000, 1, 40, (16,), F32, 'C', 'pack', 0, SPAN, 'pack_tile_lds_kernel VEC=16 TO_PACK=1 TTL=4 TRL=4', True),
    'span_lds_cat': Case(6000, 1, 40, (4,), F32, 'P', 'cat', 0, SPAN, 'pack_tile_lds_kernel VEC=16 TO_PACK=0 TTL=6 TRL=4', True),
    'span_vec_pack': Case(6000, 1, 40, (), I64, 'C', 'pack', 0, SPAN, 'pack_tile_vec_kernel RB=8 TO_PACK=1 TTL=6 TRL=5', True),
    'span_vec_full_grid_left': Case(6000, 1, 40, (), I64, 'P', 'left', 0, SPAN, 'pack_tile_vec_kernel RB=8 TO_PACK=0 TTL=6 TRL=5', True),
    'span_roll_steps': Case(5800, 1, 40, (), I64, 'P', 'roll', 2, SPAN, 'pack_roll_steps_kernel NT=0', True),
    'span_roll_tiles': Case(6000, 1, 40, (4,), F32, 'P', 'roll', 9, SPAN, 'pack_roll_tile_kernel VEC=16 TTL=6', True),
    'span_narrow_left': Case(500, 1, 40, (), I64, 'C', 'left', 0, SPAN, 'move_rows_narrow_kernel VEC=8 SCATTER=0 NT=0 CH=8', True, empty=True),
    'span_span_1000': Case(120, 1, 90, (500,), BF16, 'C', 'pack', 0, SPAN, 'move_rows_span_kernel NT=0', True),
    'span_rows_1024': Case(120, 1, 90, (256,), F32, 'C', 'pack', 0, SPAN, ROWS16 + ' NT=0', True),
    'span_rows_tail8': Case(120, 1, 90, (500,), BF16, 'C', 'pack', 0, SPAN, 'move_rows_kernel VEC=16 SCATTER=0 NT=0 RPT=1 TROWS=16 TAIL8=1', True, offset=True),
    # ---- the natural crossing of MOVE_SPAN_MIN_TILES (2 048 tiles of 16 rows in the padded destination): no flag
    'natural_span_left': Case(700, 1, 90, (256,), F32, 'C', 'left', 0, 0, ROWS16 + ' NT=0', True),
    'natural_plain_left': Case(300, 1, 90, (256,), F32, 'C', 'left', 0, 0, ROWS16 + ' NT=0 per_xcd=0'),
    # ---- NT=1, flag forced
    'nt_seq_copy': Case(6000, 1, 40, (), I64, 'C', 'left', 0, NT, 'seq_copy_kernel NT=1'),
    'nt_narrow_8': Case(300, 1, 40, (), I64, 'C', 'left', 0, NT, 'move_rows_narrow_kernel VEC=8 SCATTER=0 NT=1', empty=True),
    'nt_narrow_2': Case(300, 1, 40, (), I16, 'C', 'right', 0, NT, 'move_rows_narrow_kernel VEC=2 SCATTER=0 NT=1'),
    'nt_span_1000': Case(120, 1, 90, (500,), BF16, 'C', 'pack', 0, NT, 'move_rows_span_kernel NT=1'),
    'nt_rows_1024': Case(120, 1, 90, (256,), F32, 'C', 'pack', 0, NT, ROWS16 + ' NT=1'),
    'nt_rows_26': Case(150, 1, 60, (13,), BF16, 'C', 'left', 0, NT, 'move_rows_kernel VEC=2 SCATTER=0 NT=1 RPT=1 TROWS=256 TAIL8=0'),
    'nt_rows_tail8': Case(120, 1, 90, (500,), BF16, 'C', 'pack', 0, NT, 'move_rows_kernel VEC=16 SCATTER=0 NT=1 RPT=1 TROWS=16 TAIL8=1', offset=True),
    'nt_rows_same_pack_rpt': Case(300, 1, 2, (8,), F32, 'P', 'roll', 1, NT, 'move_rows_kernel VEC=16 SCATTER=0 NT=1 RPT=4 TROWS=256 TAIL8=0'),
    # ---- the shifted windows of P.cat(): R rows of a 128-byte line
    'shift_R2': Case(6000, 1, 40, (16,), F32, 'P', 'cat', 0, 0, 'pack_tile_lds_kernel VEC=16 TO_PACK=0 R=2', phase=0),
    'shift_R4': Case(6000, 1, 40, (8,), F32, 'P', 'cat', 0, 0, 'pack_tile_lds_kernel VEC=16 TO_PACK=0 R=4', phase=0),
    'shift_R8': Case(6000, 1, 40, (4,), F32, 'P', 'cat', 0, 0, 'pack_tile_lds_kernel VEC=16 TO_PACK=0 R=8', phase=0),
    # ---- rev inside one PackedSequence on the (rank x time) tiles: T_REV_S
    'rev_P_tiles_16': Case(150, 0, 60, (4,), F32, 'P', 'rev', 0, 0, 'pack_roll_tile_kernel VEC=16', empty=True),
}

# ---- SCATTER=1: z[(bp, tp)] = value on a C, an L and a P, ~1 000 distinct pairs inside the lengths
SCATTER_WIDTHS = {
    'i64': ((), I64, False, 'move_rows_narrow_kernel VEC=8 SCATTER=1'),
    'i16': ((), I16, False, 'move_rows_narrow_kernel VEC=2 SCATTER=1'),
    '1024': ((256,), F32, False, 'move_rows_kernel VEC=16 SCATTER=1 TAIL8=0'),
    '26': ((13,), BF16, False, 'move_rows_kernel VEC=2 SCATTER=1'),
    'tail8': ((500,), BF16, True, 'move_rows_kernel VEC=16 SCATTER=1 TAIL8=1'),
}
for _k in 'CLP':
    for _w, (_h, _d, _o, _want) in SCATTER_WIDTHS.items():
        CASES[f'scatter_{_k}_{_w}'] = Case(150, 1, 60, _h, _d, _k, 'setitem_ptr', 0, 0, _want + ' NT=0', offset=_o)
CASES.update({
    'scatter_key_container_8': Case(150, 1, 60, (), I64, 'L', 'setitem_container', 0, 0, 'move_rows_narrow_kernel VEC=8 SCATTER=1'),
    'scatter_key_container_1024': Case(150, 1, 60, (256,), F32, 'L', 'setitem_container', 0, 0, 'move_rows_kernel VEC=16 SCATTER=1'),
    'scatter_key_tensor_8': Case(150, 1, 60, (), I64, 'C', 'setitem_tensor', 0, 0, 'move_rows_narrow_kernel VEC=8 SCATTER=1'),
    'scatter_key_tensor_1024': Case(150, 1, 60, (256,), F32, 'C', 'setitem_tensor', 0, 0, 'move_rows_kernel VEC=16 SCATTER=1'),
    'scatter_nt_1024': Case(150, 1, 60, (256,), F32, 'C', 'setitem_ptr', 0, NT, 'move_rows_kernel VEC=16 SCATTER=1 NT=1'),
    'scatter_span_1024': Case(150, 1, 60, (256,), F32, 'C', 'setitem_ptr', 0, SPAN, 'move_rows_kernel VEC=16 SCATTER=1 NT=0', True),
})

# ---- the time maps, pad_row and len_add at three widths: rows of one vector, the span form, 1 KiB rows.  About 150
# sequences of 0 .. 60 tokens, empty ones and one of exactly T among them; `last` needs a last token (the reference reads
# token -1 of an empty sequence) and trunc((1, 2)) / head(2) three tokens, so those start at 1 and 3.
TMAP_WIDTHS = {'i64': ((), I64, 'move_rows_narrow_kernel VEC=8 SCATTER=0'), '1000': ((500,), BF16, 'move_rows_span_kernel'),
               '1024': ((256,), F32, ROWS16)}
TMAP_OPS = [('rev', 0, 'CLRP', 0), ('roll', 3, 'LR', 0), ('roll', -2, 'LR', 0), ('last', 0, 'CLRP', 1),
            ('trunc', (1, 2), 'CP', 3), ('head', 2, 'CR', 3)]
for _op, _arg, _kinds, _lo in TMAP_OPS:
    for _k in _kinds:
        for _w, (_h, _d, _want) in TMAP_WIDTHS.items():
            _name = f'{_op}_{_k}_{_w}' if _op != 'roll' else f'roll{_arg:+d}_{_k}_{_w}'
            CASES[_name] = Case(150, _lo, 60, _h, _d, _k, _op, _arg, 0, _want + ' NT=0', empty=_lo == 0)
# T_REV_D: the gradient of rev (float64 stands in for int64 at 8-byte rows: an integer payload has no gradient)
for _w, (_h, _d, _want) in {**TMAP_WIDTHS, 'i64': ((), F64, TMAP_WIDTHS['i64'][2])}.items():
    for _k in 'CL':
        CASES[f'grad_rev_{_k}_{_w if _w != "i64" else "f64"}'] = Case(150, 0, 60, _h, _d, _k, 'grad_rev', 0, 0, _want + ' NT=0', empty=True)
# ---- lengths on the device only: whatever form the plan takes for that layout
for _op in ('left', 'right', 'pack', 'rev'):
    for _w, (_h, _d) in {'i64': ((), I64), '1024': ((256,), F32)}.items():
        CASES[f'devlens_{_op}_{_w}'] = Case(300, 0, 40, _h, _d, 'C', _op, 0, 0, None, empty=True)


def test_the_table_declares_every_variant():
    """What the cases DECLARE (their record words), on any machine: a variant dropped from the table fails here."""
    words = {name: set((c.want or '').split()) | ({'span'} if c.span else set()) for name, c in CASES.items()}
    kernel = {name: (c.want or ' ').split(' ')[0] for name, c in CASES.items()}

    def some(k, *need):
        return any(kernel[n] == k and set(need) <= w for n, w in words.items())

    assert set(kernel.values()) - {''} == set(KERNELS)
    assert some('move_rows_kernel', 'SCATTER=1') and some('move_rows_narrow_kernel', 'SCATTER=1')
    for k in ('seq_copy_kernel', 'move_rows_narrow_kernel', 'move_rows_span_kernel', 'move_rows_kernel'):
        assert some(k, 'NT=1'), k
    for k in SPANNING:
        assert some(k, 'span'), k
    assert len(SPANNING) == 7 and set(SPANNING) < set(KERNELS)
    for r in ('R=2', 'R=4', 'R=8'):
        assert some('pack_tile_lds_kernel', r), r
    assert some('move_rows_kernel', 'TAIL8=1', 'SCATTER=1') and some('move_rows_kernel', 'RPT=4', 'NT=1')
    assert some('move_rows_kernel', 'SCATTER=1', 'NT=1') and some('move_rows_kernel', 'SCATTER=1', 'span')
    ops = {c.op for c in CASES.values()}
    assert {'rev', 'roll', 'last', 'trunc', 'head', 'grad_rev', 'setitem_ptr', 'setitem_container', 'setitem_tensor'} <= ops
    for op in ('rev', 'roll', 'last', 'trunc', 'grad_rev'):
        assert {kernel[n] for n, c in CASES.items() if c.op == op} >= {'move_rows_narrow_kernel', 'move_rows_span_kernel',
                                                                      'move_rows_kernel'}, op
    assert any(c.op == 'rev' and kernel[n] == 'pack_roll_tile_kernel' for n, c in CASES.items())
    assert sum(c.want is None for c in CASES.values()) == 8 and all(n.startswith('devlens_') for n, c in CASES.items() if c.want is None)


# ------------------------------------------------------------------ payloads and the CPU constructions
def _bits(shape, dtype, seed):
    """Seeded random bits over the full range of the element's integer type, viewed as `dtype`.  Rows of ONE 2-byte
    element are drawn without replacement, so that no two rows agree by accident (wider rows: 2^-32 or less)."""
    g = torch.Generator().manual_seed(seed)
    it = INT_OF[dtype.itemsize]
    if dtype.itemsize == 2 and len(shape) == 1:
        assert shape[0] <= 65536
        raw = (torch.randperm(65536, generator=g)[:shape[0]] - 32768).to(it)
    else:
        info = torch.iinfo(it)
        raw = torch.randint(info.min, info.max, tuple(shape), dtype=it, generator=g)
    return raw.view(dtype)


def _same_bits(a, b):
    it = INT_OF[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _pack_rows(lens, srt=None):
    """Per storage row of the PackedSequence: the CattedSequence row of its token (the order `srt`: the host sort)."""
    srt = torch.as_tensor(host_sort(lens)) if srt is None else srt
    off = torch.cumsum(lens, 0) - lens
    steps = [off[srt[lens[srt] > t]] + t for t in range(int(lens.max()) if lens.numel() else 0)]
    return torch.cat(steps) if steps else torch.zeros(0, dtype=torch.long)


def _place(kind, data, lens, pad=0, srt=None):
    """`data` (a CattedSequence's payload with the lengths `lens`) as the storage of `kind`; padding rows hold `pad`."""
    if kind == 'C':
        return data
    if kind == 'P':
        return data[_pack_rows(lens, srt)]
    B, T = lens.numel(), int(lens.max())
    out = torch.empty((B, T) + tuple(data.shape[1:]), dtype=data.dtype)
    out[:] = pad
    for b, r in enumerate(_rows(lens)):
        if kind == 'L':
            out[b, :r.numel()] = data[r]
        else:
            out[b, T - r.numel():] = data[r]
    return out


def _per_seq(data, lens, fn):
    return torch.cat([fn(data[r]) for r in _rows(lens)]) if lens.numel() else data


def _container(kind, c):
    return {'C': lambda: c, 'L': lambda: c.left(FILL), 'R': lambda: c.right(FILL), 'P': c.pack}[kind]()


def _one_row_in(z):
    """(the same container over a view one row into a fresh storage, that storage): rows of 8 (mod 16) bytes then start
    on 8-byte boundaries only."""
    flat = z.data if isinstance(z, (ta.C, ta.P)) else z.data.flatten(0, 1)
    store = torch.cat([flat[:1], flat])
    return z._replace(data=store[1:].view(z.data.shape)), store


def _storage_rows(kind, lens, b, t):
    """The storage rows of the tokens (b, t) of a container of `kind` (layout/*.py: idx())."""
    off = torch.cumsum(lens, 0) - lens
    if kind == 'C':
        return off[b] + t
    T = int(lens.max())
    if kind == 'L':
        return b * T + t
    if kind == 'R':
        return b * T + (T - lens[b]) + t
    where = torch.empty(int(lens.sum()), dtype=torch.long)
    where[_pack_rows(lens)] = torch.arange(where.numel())           # CattedSequence row -> PackedSequence row
    return where[off[b] + t]


def _run(case, name, monkeypatch):
    """(result, expected, real records, dry records, plain dry records of the flagged call)"""
    lens = _lens(case.B, case.lo, case.hi, empty=case.empty)
    if name == 'nt_rows_same_pack_rpt':
        lens[0] = 700                              # (as in test_gpu_move_plan: the tile table would be mostly dead cells)
    if case.hi == 60:
        lens[1] = 60                               # one sequence of exactly T
    data = _bits((int(lens.sum()),) + case.hidden, case.dtype, seed=11)
    rb = case.dtype.itemsize
    for d in case.hidden:
        rb *= d
    scatter = case.op.startswith('setitem')
    pick = lambda row_bytes, flags: row_bytes == rb and bool(flags & K.MOVE_SCATTER) == scatter
    plain = []
    traced = lambda fn: _traced(monkeypatch, fn, case.flags, pick, plain)

    if case.op == 'grad_rev':
        src = _place(case.src, data, lens, pad=FILL)
        x = src.clone().to(DEV).requires_grad_(True)
        sizes = ta.with_host_sizes(x.detach(), lens).token_sizes
        z = {'C': ta.C, 'L': ta.L}[case.src](x, sizes)
        cot = _bits(tuple(src.shape), case.dtype, seed=13)
        cot_dev = cot.to(DEV)
        torch.cuda.synchronize()
        _, real, dry = traced(lambda: z.rev().data.backward(cot_dev))
        # the adjoint of a reversal is the reversal of the cotangent; padding rows get no gradient
        want = _place(case.src, _per_seq(_gather_tokens(case.src, cot, lens), lens, lambda s: s.flip(0)), lens, pad=0)
        return x.grad.cpu(), want, real, dry, plain

    c = ta.with_host_sizes(data.to(DEV), lens) if not name.startswith('devlens_') else ta.C(data.to(DEV), lens.to(DEV))
    z = _container(case.src, c)
    store = None
    if case.offset:
        z, store = _one_row_in(z)
    torch.cuda.synchronize()

    if scatter:
        store = z.data if store is None else store
        before = store.cpu()
        g = torch.Generator().manual_seed(17)
        if case.op == 'setitem_ptr':
            bp = torch.repeat_interleave(torch.arange(lens.numel()), lens)
            tp = torch.cat([torch.arange(int(n)) for n in lens])
            keep = torch.randperm(bp.numel(), generator=g)[:1000]          # distinct (b, t) pairs, every one a token
            bp, tp = bp[keep], tp[keep]
            rows = _storage_rows(case.src, lens, bp, tp)
            key = (bp.to(DEV), tp.to(DEV))
        else:
            rows = torch.randperm(int(z.raw().size(0)), generator=g)[:1000]      # distinct storage rows, padding rows too
            key = rows.to(DEV)
            if case.op == 'setitem_container':
                key = ta.C(key, torch.tensor([400, 0, 600]).to(DEV))
        value = _bits((1000,) + case.hidden, case.dtype, seed=19)
        value_dev = value.to(DEV)
        torch.cuda.synchronize()

        def run():
            with torch.no_grad():
                z[key] = value_dev
        _, real, dry = traced(run)
        want = before.clone()
        flat = want.view((-1,) + case.hidden)
        flat.index_put_((rows + (1 if case.offset else 0),), value)
        return store.cpu(), want, real, dry, plain

    op, arg = case.op, case.arg
    run = {'pack': lambda: z.pack(), 'cat': lambda: z.cat(), 'left': lambda: z.left(FILL), 'right': lambda: z.right(FILL),
           'roll': lambda: z.roll(arg), 'rev': lambda: z.rev(), 'last': lambda: z.last(), 'trunc': lambda: z.trunc(arg),
           'head': lambda: z.head(arg)}[op]
    out, real, dry = traced(run)
    got = (out if isinstance(out, torch.Tensor) else out.data).cpu()
    if op in ('pack', 'cat', 'left', 'right'):
        want = _expect({'pack': 'P', 'cat': 'C', 'left': 'L', 'right': 'R'}[op], data, lens)
    elif op == 'rev':
        # select.py, _rev: "padding rows = 0 for L/R: the reference goes through .left()/.right() with the default fill"
        want = _place(case.src, _per_seq(data, lens, lambda s: s.flip(0)), lens, pad=0)
    elif op == 'roll':
        # select.py, _padded_roll: "The reference pads its index tensor with 0, so its padding rows are copies of
        # storage row 0": row 0 of the SOURCE's storage (for an R that is a padding row itself unless sequence 0 is a
        # longest one)
        pad = _expect(case.src, data, lens)[0, 0] if case.src in 'LR' else 0
        want = _place(case.src, _per_seq(data, lens, lambda s: s.roll(arg, 0)), lens, pad=pad)
    elif op == 'last':
        want = torch.stack([data[r[-1]] for r in _rows(lens)])
    elif op == 'trunc':
        a, b = arg
        cut = _per_seq(data, lens, lambda s: s[a:s.size(0) - b])
        want = _place(case.src, cut, lens - a - b, srt=torch.as_tensor(host_sort(lens)))     # (P: batch_sizes[a + b:], the same order)
    elif op == 'head':
        first = _per_seq(data, lens, lambda s: s[:arg])
        want = first if case.src == 'C' else first.view((lens.numel(), arg) + case.hidden)
    return got, want, real, dry, plain


def _gather_tokens(kind, stor, lens):
    """The CattedSequence payload of the tokens of a storage of `kind`."""
    if kind == 'C':
        return stor
    return torch.cat([stor[b, :int(n)] for b, n in enumerate(lens)])


def _field(record, key):
    return int(dict(w.split('=') for w in record.split()[1:])[key])


@gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_variant_record_and_result(name, monkeypatch):
    case = CASES[name]
    got, want, real, dry, plain = _run(case, name, monkeypatch)
    print(name, 'real:', real, 'plain:', plain)
    assert real == dry and len(real) >= 1, (real, dry)
    if case.want is None:
        assert all(r.split()[0] in KERNELS for r in real) and len(real) == 1, real
        hits = real
    else:
        kernel, *pairs = case.want.split()
        hits = [r for r in real if r.split()[0] == kernel and set(pairs) <= set(r.split()[1:])]
        assert hits, (case.want, real)
    if case.flags:
        assert len(plain) == 1, plain                              # the flags went into ONE mover call
    if case.span:
        rec = hits[-1]
        per_xcd, grid = _field(rec, 'per_xcd'), _field(rec, 'grid')
        assert per_xcd > 0 and grid == 8 * per_xcd, rec
        if case.flags:
            tiles = _field(plain[0], 'grid')                       # plain blockIdx order: one workgroup per tile
            assert tiles >= 9 and tiles % 8 != 0 and per_xcd == (tiles + 7) // 8 and grid != tiles, (plain, rec)
    if case.phase is not None:
        assert _field(hits[-1], 'phase') == case.phase, hits
    assert _same_bits(got, want), name
