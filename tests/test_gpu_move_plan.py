"""One small case per form of the row mover's plan (csrc/rua_move_plan.h), through the public surface.  For every
rua_move_rows call a case makes: the record the call leaves in the dispatch trace equals the record rua_debug_move_plan
gives for the same arguments (taken at the call, by a spy on the binding), the form the case is there for did take it, and
the result equals, bit for bit, a plain torch indexing construction from the lengths."""
import ctypes

import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace, host_sort
from test_move_plan import KERNELS
from torchrua_amd import _lib as K

pytestmark = pytest.mark.gpu
FILL = 7


def _lens(B, lo, hi, seed=5, empty=False):
    lens = torch.randint(lo, hi + 1, (B,), generator=torch.Generator().manual_seed(seed))
    if empty:
        lens[::41] = 0
    return lens


def _data(lens, hidden, dtype):
    shape = (int(lens.sum()),) + hidden
    return (torch.arange(torch.Size(shape).numel()) % 251 + 1).reshape(shape).to(dtype)      # (exact in every dtype used here)


def _rows(lens):
    """Per sequence: the storage rows of its tokens in the CattedSequence."""
    off = torch.cumsum(lens, 0) - lens
    return [torch.arange(int(o), int(o + l)) for o, l in zip(off, lens)]


def _pack_index(lens):
    srt = torch.as_tensor(host_sort(lens))
    off = torch.cumsum(lens, 0) - lens
    T = int(lens.max())
    return torch.cat([off[srt[lens[srt] > t]] + t for t in range(T)])


def _expect(kind, data, lens, roll=0):
    """`data` (a CattedSequence's payload) as the payload of `kind`, every sequence rolled by `roll` first."""
    rows = _rows(lens)
    if roll:
        data = data[torch.cat([torch.roll(r, roll) for r in rows])]
    if kind == 'C':
        return data
    if kind == 'P':
        return data[_pack_index(lens)]
    B, T = lens.numel(), int(lens.max())
    out = torch.full((B, T) + tuple(data.shape[1:]), FILL, dtype=data.dtype)
    for b, r in enumerate(rows):
        if kind == 'L':
            out[b, :r.numel()] = data[r]
        else:
            out[b, T - r.numel():] = data[r]
    return out


def _traced(monkeypatch, fn, extra_flags=0, pick=None, plain=None):
    """fn() with the trace on and a spy on rua_move_rows: (result, the mover's trace records, the dry records).
    extra_flags: developer flags (include/rua.h) ORed into the calls `pick(row_bytes, flags)` accepts, before the dry
    call and the real one alike; every other mover call passes through unchanged.  `plain` (a list) receives, per call
    that was picked, the dry record of the call as the library made it."""
    lib = K.load()
    real, dry = lib.rua_move_rows, []

    def plan(dst, src, tmap, arg, out_ptr, src_ptr, rb, pad_row, flags):
        buf = ctypes.create_string_buffer(512)
        n = lib.rua_debug_move_plan(dst, src, tmap, arg, out_ptr or 0, src_ptr or 0, rb, pad_row, flags, buf, 512)
        assert n >= 0, n
        return buf.raw[:n].decode()

    def spy(dst, src, tmap, arg, out_ptr, src_ptr, rb, fill, pad_row, flags, stream):
        if extra_flags and pick(rb, flags):
            if plain is not None:
                plain.append(plan(dst, src, tmap, arg, out_ptr, src_ptr, rb, pad_row, flags))
            flags |= extra_flags
        rec = plan(dst, src, tmap, arg, out_ptr, src_ptr, rb, pad_row, flags)
        if rec:
            dry.append(rec)
        return real(dst, src, tmap, arg, out_ptr, src_ptr, rb, fill, pad_row, flags, stream)

    monkeypatch.setattr(lib, 'rua_move_rows', spy)
    with dispatch_trace() as tr:
        out = fn()
    monkeypatch.undo()
    return out, [r for r in tr.records if r.split(' ', 1)[0] in KERNELS], dry


# id: (B, lo, hi, hidden, dtype, source kind, operation, result kind, roll, a word sequence the form's record must carry)
CASES = {
    'tiles_lds_pack': (6000, 1, 40, (16,), torch.float32, 'C', 'pack', 'P', 0, 'pack_tile_lds_kernel VEC=16 TO_PACK=1 TTL=4 TRL=4'),
    'tiles_lds_cat_line_aligned': (6000, 1, 40, (4,), torch.float32, 'P', 'cat', 'C', 0, 'pack_tile_lds_kernel VEC=16 TO_PACK=0 TTL=6 TRL=4'),
    'tiles_vec_pack_16': (6000, 1, 40, (4,), torch.float32, 'C', 'pack', 'P', 0, 'pack_tile_vec_kernel RB=16 TO_PACK=1 TTL=6 TRL=4'),
    'tiles_vec_pack_8': (6000, 1, 40, (), torch.int64, 'C', 'pack', 'P', 0, 'pack_tile_vec_kernel RB=8 TO_PACK=1 TTL=6 TRL=5'),
    'tiles_lds_pack_1': (6000, 1, 120, (), torch.uint8, 'C', 'pack', 'P', 0, 'pack_tile_lds_kernel VEC=1 TO_PACK=1 TTL=7 TRL=7'),
    'tiles_full_grid_left': (6000, 1, 40, (), torch.int64, 'P', 'left', 'L', 0, 'pack_tile_vec_kernel RB=8 TO_PACK=0 TTL=6 TRL=5'),
    'roll_steps': (6000, 1, 40, (), torch.int64, 'P', 'roll', 'P', 2, 'pack_roll_steps_kernel NT=0'),
    'roll_tiles': (6000, 1, 40, (4,), torch.float32, 'P', 'roll', 'P', 9, 'pack_roll_tile_kernel VEC=16 TTL=6'),
    'seq_copy_left': (6000, 1, 40, (), torch.int64, 'C', 'left', 'L', 0, 'seq_copy_kernel NT=0'),
    'narrow_left_with_empty': (300, 1, 40, (), torch.int64, 'C', 'left', 'L', 0, 'move_rows_narrow_kernel VEC=8 SCATTER=0 NT=0 CH=8'),
    'narrow_right_2': (300, 1, 40, (), torch.int16, 'C', 'right', 'R', 0, 'move_rows_narrow_kernel VEC=2 SCATTER=0 NT=0 CH=8'),
    'span_1000': (120, 1, 90, (500,), torch.bfloat16, 'C', 'pack', 'P', 0, 'move_rows_span_kernel NT=0'),
    'span_2000': (60, 1, 70, (1000,), torch.bfloat16, 'C', 'left', 'L', 0, 'move_rows_span_kernel NT=0'),
    'rows_tail8': (120, 1, 90, (500,), torch.bfloat16, 'C', 'pack_offset', 'P', 0, 'move_rows_kernel VEC=16 SCATTER=0 NT=0 RPT=1 TROWS=16 TAIL8=1'),
    'rows_1024': (120, 1, 90, (256,), torch.float32, 'C', 'pack', 'P', 0, 'move_rows_kernel VEC=16 SCATTER=0 NT=0 RPT=1 TROWS=16 TAIL8=0'),
    'rows_26': (150, 1, 60, (13,), torch.bfloat16, 'C', 'left', 'L', 0, 'move_rows_kernel VEC=2 SCATTER=0 NT=0 RPT=1 TROWS=256 TAIL8=0'),
    'rows_same_pack_rpt': (300, 1, 2, (8,), torch.float32, 'P', 'roll', 'P', 1, 'move_rows_kernel VEC=16 SCATTER=0 NT=0 RPT=4 TROWS=256 TAIL8=0'),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_form_record_and_result(case, monkeypatch):
    B, lo, hi, hidden, dtype, src_kind, op, dst_kind, roll, want = CASES[case]
    lens = _lens(B, lo, hi, empty='empty' in case)
    if case == 'rows_same_pack_rpt':
        lens[0] = 700                              # one long sequence among short ones: the tile table would be mostly dead cells
    data = _data(lens, hidden, dtype)
    if op == 'pack_offset':                        # the payload one row into its storage: 1 000-byte rows on an 8-byte boundary
        store = torch.cat([data[:1], data]).to(DEV)
        c = ta.with_host_sizes(store[1:], lens)
    else:
        c = ta.with_host_sizes(data.to(DEV), lens)
    z = {'C': lambda: c, 'P': c.pack}[src_kind]()
    torch.cuda.synchronize()
    run = {'pack': lambda: z.pack(), 'pack_offset': lambda: z.pack(), 'cat': lambda: z.cat(), 'left': lambda: z.left(FILL),
           'right': lambda: z.right(FILL), 'roll': lambda: z.roll(roll)}[op]
    out, real, dry = _traced(monkeypatch, run)
    assert real == dry and len(real) >= 1, (real, dry)
    name, *pairs = want.split()
    assert any(r.split()[0] == name and r.split()[1:1 + len(pairs)] == pairs for r in real), (want, real)
    assert torch.equal(out.data.cpu(), _expect(dst_kind, data, lens, roll)), case
