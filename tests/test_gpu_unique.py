"""Per-sequence unique_consecutive on the GPU, bit for bit: every container against the yardstick of tests/runs_util.py
(stock torch.unique_consecutive per sequence on the CPU), the two commutation identities for values, counts and
inverse (PackedSequence metadata included), wave, block and cut borders, runs that straddle them, sequence borders,
padding, every row width class, the equality rule, the read-back, autograd and the dispatch trace of every kernel
form.  No tolerance anywhere: integers, and floats through an integer view."""
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from runs_util import runs_cat, runs_padded, same_bits, split
from test_gpu_compress import LT, SHORT_LENS, WAVE_LENS, WIDTHS, build, rewrap, same_fields
from torchrua_amd import _meta
from torchrua_amd import _ops as O
from torchrua_amd.layout import lay_hidden

pytestmark = pytest.mark.gpu

BLOCK = 2048                                   # SEG_BLOCK_TOK of csrc/rua_seg_plan.h
LONG_LENS = [2047, 2048, 2049, 0, 1]           # the long form and a block border
CUT_LENS = [8192 + 5, 3]                       # fewer than 1 024 sequences with a bound of at least 8 192: the cut form
BF16, F16, F32, F64, I64, I32, U8, BOOL = (torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64,
                                           torch.int32, torch.uint8, torch.bool)
PATTERNS = ('same', 'distinct', 'random', 'border')


# ------------------------------------------------------------------ helpers
def table(dtype, hidden):
    """Three rows to draw tokens from, pairwise different.  A row wider than one element: row 1 differs from row 0 in its
    FIRST element only, row 2 in its LAST element only (the last 4 bytes of a 132-byte float32 row)."""
    g = torch.Generator().manual_seed(5)
    n = 1
    for d in hidden:
        n *= d
    if dtype == BOOL:
        base = torch.rand(n, generator=g) < 0.5
        rows = torch.stack([base, base, base]).clone()
        rows[1, 0], rows[2, -1] = ~base[0], ~base[-1]
        if n == 1:
            rows[2] = rows[0]                                       # (one bool: an alphabet of two)
    elif dtype.is_floating_point:
        base = (torch.rand(n, generator=g) + 1).to(dtype)
        rows = torch.stack([base, base, base]).clone()
        rows[1, 0], rows[2, -1] = 3, 4
        if n == 1:
            rows[2, 0] = 4
    else:
        base = torch.randint(1, 100, (n,), generator=g).to(dtype)
        rows = torch.stack([base, base, base]).clone()
        rows[1, 0], rows[2, -1] = 101, 102
    return rows.reshape((3,) + tuple(hidden))


def draw_ids(pattern, lens, seed, straddle=()):
    """Token ids in [0, 3) (or [0, 2)) per pattern; `straddle`: (sequence, from, to) ranges forced to one id."""
    g = torch.Generator().manual_seed(seed)
    n = int(lens.sum())
    if pattern == 'same':
        ids = torch.zeros(n, dtype=torch.long)
    elif pattern == 'distinct':
        ids = torch.cat([torch.arange(int(k)) for k in lens] + [torch.zeros(0, dtype=torch.long)]) % 3
    else:
        ids = torch.randint(0, 3, (n,), generator=g)
    offs = torch.cumsum(lens, 0) - lens
    for b, lo, hi in (straddle if pattern in ('random', 'border') else ()):
        ids[int(offs[b]) + lo:int(offs[b]) + hi] = 1
    if pattern == 'border':                                         # the last token of a sequence == the first of the next
        last = None
        for b, k in enumerate(lens.tolist()):
            if k and last is not None:
                ids[int(offs[b])] = last
            if k:
                last = int(ids[int(offs[b]) + k - 1])
    return ids


def payload(ids, dtype, hidden):
    tab = table(dtype, hidden)
    if dtype == BOOL and not tab[0].numel() > 1:
        ids = ids % 2
        tab[1] = ~tab[0]
    return tab[ids]


def cast(ref, kind):
    return {'C': lambda: ref, 'L': ref.left, 'R': ref.right, 'P': ref.pack}[kind]()


def check(kind, x, lens, what, device_lens=False, fill=0):
    """z.unique_consecutive(True, True) against the yardstick and both commutation identities; returns the result."""
    z = build(kind, x, lens, fill=fill, device_lens=device_lens)
    before = z.data.clone()
    out = z.unique_consecutive(return_inverse=True, return_counts=True)
    what = f'{what} {kind}'
    assert isinstance(out, ta.SeqRuns) and all(type(f) is type(z) for f in out), what
    assert out.values.data.dtype == x.dtype and out.inverse.data.dtype == out.counts.data.dtype == I64, what
    assert same_bits(z.data, before), f'{what}: the input changed'
    assert out.values.data.numel() == 0 or \
        out.values.data.untyped_storage().data_ptr() != z.data.untyped_storage().data_ptr(), what
    # metadata objects: counts shares the values', inverse reuses z's
    if kind == 'P':
        assert out.counts.batch_sizes is out.values.batch_sizes and out.counts.sorted_indices is out.values.sorted_indices
        assert out.inverse.batch_sizes is z.batch_sizes and out.inverse.unsorted_indices is z.unsorted_indices
    else:
        assert out.counts.token_sizes is out.values.token_sizes and out.inverse.token_sizes is z.token_sizes, what
    # the yardstick, in cat form and in the container's own storage
    values, new_lens, inverse, counts, _ = runs_cat(x, lens)
    got = out.values.cat()
    assert same_bits(got.data, values), f'{what}: values'
    assert got.token_sizes.dtype == I64 and got.token_sizes.cpu().tolist() == new_lens.tolist(), f'{what}: lengths'
    assert torch.equal(out.counts.cat().data.cpu(), counts), f'{what}: counts'
    assert torch.equal(out.inverse.cat().data.cpu(), inverse), f'{what}: inverse'
    if kind in 'LR':
        pv, pi, pc = runs_padded(x, lens, right=kind == 'R')
        assert same_bits(out.values.data, pv) and torch.equal(out.counts.data.cpu(), pc), f'{what}: padded storage'
        assert torch.equal(out.inverse.data.cpu(), pi), f'{what}: padded inverse'
    else:
        assert out.counts.data.shape == (int(new_lens.sum()),) and out.inverse.data.shape == (int(lens.sum()),), what
    # z.f(...) == z.cat().f(...).X() and z.f(...).cat() == z.cat().f(...), field by field
    ref = z.cat().unique_consecutive(return_inverse=True, return_counts=True)
    for name in ta.SeqRuns._fields:
        same_fields(getattr(out, name), cast(getattr(ref, name), kind), f'{what}: X({name}(cat))')
        same_fields(getattr(out, name).cat(), getattr(ref, name), f'{what}: cat({name})')
    return out


def rows_of(dtype, hidden):
    return ('seg_runs_heads_lanes_kernel' if table(dtype, hidden)[0].numel() * table(dtype, hidden).element_size() <= 16
            else 'seg_runs_heads_rows_kernel')


# ------------------------------------------------------------------ every width, pattern and layout at the wave borders
@pytest.mark.parametrize('dtype,hidden,row_bytes', WIDTHS, ids=[f'{rb}B' for _, _, rb in WIDTHS])
def test_widths_patterns_layouts(dtype, hidden, row_bytes):
    lens = LT(WAVE_LENS)
    for i, pattern in enumerate(PATTERNS):
        x = payload(draw_ids(pattern, lens, 10 + i, straddle=((6, 60, 70),)), dtype, hidden)
        assert x[0].numel() * x.element_size() == row_bytes
        for kind in 'CLPR':
            with dispatch_trace() as tr:
                out = check(kind, x, lens, f'{row_bytes}B {pattern}')
            assert tr.matching(f'{rows_of(dtype, hidden)} row_bytes={row_bytes}'), tr.records
            if pattern == 'same':
                assert out.values.cat().token_sizes.cpu().tolist() == [min(k, 1) for k in WAVE_LENS]
            if pattern == 'distinct' and row_bytes > 1:
                assert out.values.cat().token_sizes.cpu().tolist() == WAVE_LENS
                same_fields(out.values, build(kind, x, lens), 'all distinct: the identity')


def test_sequence_borders_do_not_merge():
    """The last token of every sequence equals the first of the next: a global unique_consecutive merges them."""
    lens = LT([3, 2, 0, 4, 1, 1])
    ids = LT([7, 7, 5, 5, 5, 5, 5, 9, 9, 9, 9])
    assert torch.unique_consecutive(ids).tolist() == [7, 5, 9]
    for kind in 'CLPR':
        out = check(kind, ids, lens, 'borders')
        c = out.values.cat()
        assert c.data.cpu().tolist() == [7, 5, 5, 5, 9, 9, 9] and c.token_sizes.cpu().tolist() == [2, 1, 0, 2, 1, 1]
        assert out.counts.cat().data.cpu().tolist() == [2, 1, 2, 2, 2, 1, 1]
        assert out.inverse.cat().data.cpu().tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0]


def test_padding_is_ignored_and_comes_back_as_zeros():
    """Padding of an L / R filled with the neighbouring tokens' value: never read, zeros in every output."""
    lens = LT([3, 0, 9, 5])
    for dtype, hidden, fill in ((I64, (), 4), (F32, (5,), 2.5), (BF16, (), 2.5)):
        x = torch.full((int(lens.sum()),) + hidden, fill, dtype=dtype)
        for kind in 'LR':
            out = check(kind, x, lens, 'padding', fill=fill)
            assert out.values.data.shape[:2] == (4, 1) and out.counts.data.cpu().reshape(-1).tolist() == [3, 0, 9, 5]
            assert not bool(out.inverse.data.any()) and not bool(out.values.data[1].any())
    # T_phys above the longest sequence, NaN padding
    data = torch.full((4, 12, 2), float('nan'))
    x = payload(draw_ids('random', lens, 3), F32, (2,))
    for right in (False, True):
        for b, s in enumerate(split(x, lens)):
            n = s.shape[0]
            data[b, (9 - n if right else 0):(9 if right else n)] = s
        z = (ta.R if right else ta.L)(data.to(DEV), lens.to(DEV))
        out = z.unique_consecutive(True, True)
        pv, pi, pc = runs_padded(x, lens, right=right)
        assert same_bits(out.values.data, pv) and torch.equal(out.counts.data.cpu(), pc)
        assert out.inverse.data.shape == (4, 12) and not bool(out.inverse.data[:, 9:].any())
        assert torch.equal(out.inverse.data[:, :9].cpu(), pi)


# ------------------------------------------------------------------ the forms: lanes, rows, long, cut
def test_short_sequences_take_the_lanes_forms():
    lens = LT(SHORT_LENS)
    for dtype, hidden in ((I64, ()), (F32, (5,))):
        x = payload(draw_ids('random', lens, 7), dtype, hidden)
        for kind in 'CLPR':
            for device_lens in (False, True):
                with dispatch_trace() as tr:
                    check(kind, x, lens, 'short', device_lens=device_lens)
                if device_lens and kind == 'C':
                    continue                                     # (the bound is the row count: another form)
                assert tr.matching('seg_compress_plan_kernel form=lanes G=32'), tr.records
                assert tr.matching('seg_runs_inverse_kernel form=lanes G=32'), tr.records
                assert tr.matching('seg_runs_counts_kernel form=lanes phase=starts'), tr.records
                assert tr.matching('seg_runs_counts_kernel form=lanes phase=diff'), tr.records
                if hidden:
                    assert tr.matching('seg_runs_heads_rows_kernel form=long G=256 W=4 row_bytes=20'), tr.records
                else:
                    assert tr.matching('seg_runs_heads_lanes_kernel form=lanes G=32 W=8 row_bytes=8'), tr.records


def test_wave_lengths_take_the_rows_forms():
    lens = LT(WAVE_LENS)
    x = payload(draw_ids('random', lens, 8, straddle=((6, 60, 70),)), I64, ())
    for kind in 'CLPR':
        for device_lens in (False, True):
            with dispatch_trace() as tr:
                check(kind, x, lens, 'rows', device_lens=device_lens)
            for name in ('seg_runs_heads_lanes_kernel', 'seg_compress_plan_kernel', 'seg_runs_inverse_kernel'):
                assert tr.matching(f'{name} form=rows G=64'), tr.records
            assert tr.matching('seg_runs_counts_kernel form=rows phase=starts'), tr.records


def test_sequences_across_blocks_take_the_long_forms():
    lens = LT(LONG_LENS)
    straddle = ((0, 60, 70), (1, 2040, 2048), (2, 2040, 2049), (2, 60, 70))
    for dtype, hidden in ((I64, ()), (BF16, (20,))):
        for pattern in ('random', 'same', 'border'):
            x = payload(draw_ids(pattern, lens, 9, straddle=straddle), dtype, hidden)
            for kind in 'CLPR':
                for device_lens in ((False, True) if pattern == 'random' else (False,)):
                    with dispatch_trace() as tr:
                        check(kind, x, lens, f'long {pattern}', device_lens=device_lens)
                    assert tr.matching('seg_compress_plan_kernel form=long G=256 cut=0'), tr.records
                    assert tr.matching('seg_runs_inverse_kernel form=long G=256 cut=0'), tr.records
                    assert tr.matching(f'{rows_of(dtype, hidden)} form=long cut=0'), tr.records
                    assert tr.matching('seg_runs_counts_kernel phase=starts form=long'), tr.records
                    assert not tr.matching('seg_compress_plan_kernel form=cut')


def test_cut_equals_uncut():
    """B = 2 with a bound of 8 197 is cut across workgroups (two launches per scan); without the workspace the same
    tables come from one workgroup per sequence, bit for bit.  Runs straddle the cut-block borders."""
    lens = LT(CUT_LENS)
    straddle = ((0, 2040, 2056), (0, 4095, 4097), (0, 6100, 8197))
    for dtype, hidden in ((I64, ()), (F32, (33,))):
        x = payload(draw_ids('random', lens, 14, straddle=straddle), dtype, hidden)
        for kind in 'CLPR':
            for device_lens in (False, True):
                if device_lens and kind == 'C':
                    continue                                     # (T_log unknown: the same rule over the row count)
                with dispatch_trace() as tr:
                    check(kind, x, lens, 'cut', device_lens=device_lens)
                blocks = 5
                for name in ('seg_compress_plan_kernel', 'seg_runs_inverse_kernel'):
                    assert tr.matching(f'{name} form=cut phase=count blocks={blocks}'), tr.records
                    assert tr.matching(f'{name} form=cut phase=finish blocks={blocks}'), tr.records
                assert tr.matching(f'{rows_of(dtype, hidden)} form=cut cut=1 blocks={blocks}'), tr.records
                assert tr.matching(f'seg_runs_counts_kernel form=cut phase=starts blocks={blocks}'), tr.records
            # the same tables without the workspace
            z = build(kind, x, lens)
            big, hid = lay_hidden(z)
            head = O.launch_runs_heads(big, z.data, hid)
            lead = tuple(z.data.shape[:1 if kind in 'CP' else 2])
            with dispatch_trace() as tr:
                rank_u, lens_u = O.launch_compress_plan(big, head, cut=False)
                inv_u = O.launch_runs_inverse(big, head, lead, cut=False)
            assert tr.matching('seg_runs_inverse_kernel form=long cut=0') and not tr.matching('seg_runs_inverse_kernel form=cut')
            rank_c, lens_c = O.launch_compress_plan(big, head)
            assert torch.equal(rank_u, rank_c) and torch.equal(lens_u, lens_c)
            assert torch.equal(inv_u, O.launch_runs_inverse(big, head, lead))
            assert torch.equal(inv_u, z.unique_consecutive(return_inverse=True).inverse.data)


# ------------------------------------------------------------------ the equality rule
def test_float_equality_is_ieee_and_other_dtypes_compare_bits():
    lens = LT([5, 0, 6, 2])
    nan, inf = float('nan'), float('inf')
    for dtype in (F32, F64, BF16, F16):
        # NaN rows never merge; -0.0 / +0.0 merge and the value keeps the first one's bits
        x = torch.tensor([nan, nan, 1, 1, 1, -0.0, 0.0, 0.0, -0.0, inf, inf, 0.0, -0.0], dtype=dtype)
        for hidden in ((), (3,), (9,)):
            xs = x if not hidden else torch.stack([torch.ones_like(x)] * (hidden[0] - 1) + [x], dim=1).contiguous()
            for kind in 'CLPR':
                out = check(kind, xs, lens, f'ieee {dtype} {hidden}')
                assert out.values.cat().token_sizes.cpu().tolist() == [3, 0, 2, 1], (dtype, hidden)
                assert out.counts.cat().data.cpu().tolist() == [1, 1, 3, 4, 2, 2]
                v = out.values.cat().data.reshape(6, -1)[:, -1]
                assert bool(torch.signbit(v[3])) and not bool(torch.signbit(v[5])) and bool(torch.isnan(v[:2]).all())
        # the same float value, another NaN payload: apart (a NaN equals nothing), and the payload bits survive
        iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
        q = torch.tensor([nan, nan, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2], dtype=dtype)
        q.view(iv)[1] += 1
        out = check('C', q, lens, f'nan payload {dtype}')
        assert out.values.token_sizes.cpu().tolist() == [3, 0, 1, 1] and same_bits(out.values.data[:2], q[:2])
    # int64 values that differ only in bit 63 stay apart; int32, uint8 and bool compare bits
    x = LT([5, 5, 5 - 2 ** 63, 5 - 2 ** 63, 5, 0, 0, -2 ** 63, -2 ** 63, 0, 1, 1, 1])
    for kind in 'CLPR':
        out = check(kind, x, lens, 'bit 63')
        assert out.counts.cat().data.cpu().tolist() == [2, 2, 1, 2, 2, 1, 1, 2]
    for dtype in (I32, U8, BOOL):
        g = torch.Generator().manual_seed(3)
        for hidden in ((), (3,), (20,)):
            x = torch.randint(0, 2, (13,) + hidden, generator=g).to(dtype)
            x[3:5] = x[2]
            for kind in 'CLPR':
                check(kind, x, lens, f'bits {dtype} {hidden}')


# ------------------------------------------------------------------ strides, base addresses, flags, the segment form
def test_sliced_and_non_contiguous_payloads():
    lens = LT(WAVE_LENS)
    n = int(lens.sum())
    for dtype, hidden in ((I64, ()), (F32, (5,)), (BF16, (66,)), (U8, ())):
        x = payload(draw_ids('random', lens, 19), dtype, hidden)
        want = runs_cat(x, lens)
        shifted = torch.cat([x[:1], x]).to(DEV)[1:]               # the base address offset by one row
        flat = torch.cat([x.reshape(-1)[:1], x.reshape(-1)]).to(DEV)[1:].reshape(x.shape)     # ... by one element
        assert flat.data_ptr() % 16 != 0
        for data in (shifted, flat):
            out = ta.C(data, lens.to(DEV)).unique_consecutive(True, True)
            assert same_bits(out.values.data, want[0]) and torch.equal(out.counts.data.cpu(), want[3])
            assert torch.equal(out.inverse.data.cpu(), want[2])
    wide = payload(draw_ids('random', lens, 20), F32, (10,)).to(DEV)
    wide[:, 1::2] = 7
    x = wide[:, ::2]
    assert not x.is_contiguous()
    out = ta.C(x, lens.to(DEV)).unique_consecutive(True, True)
    want = runs_cat(x.cpu(), lens)
    assert same_bits(out.values.data, want[0]) and torch.equal(out.counts.data.cpu(), want[3])
    left = ta.C(x, lens.to(DEV)).left()
    out = ta.L(left.data.transpose(0, 1).contiguous().transpose(0, 1), left.token_sizes).unique_consecutive()
    assert same_bits(out.values.cat().data, want[0])


def test_flags_off_return_none_and_skip_their_launches():
    lens = LT(WAVE_LENS)
    x = payload(draw_ids('random', lens, 21), I64, ())
    want = runs_cat(x, lens)
    for kind in 'CLPR':
        z = build(kind, x, lens)
        with dispatch_trace() as tr:
            out = z.unique_consecutive()
        assert out.inverse is None and out.counts is None and same_bits(out.values.cat().data, want[0])
        assert not tr.matching('seg_runs_inverse_kernel') and not tr.matching('seg_runs_counts_kernel'), tr.records
        assert len(tr.matching('seg_runs_heads_lanes_kernel')) == 1 and len(tr.matching('seg_compress_plan_kernel')) == 1
        with dispatch_trace() as tr:
            out = z.unique_consecutive(return_inverse=True)
        assert out.counts is None and torch.equal(out.inverse.cat().data.cpu(), want[2])
        assert tr.matching('seg_runs_inverse_kernel') and not tr.matching('seg_runs_counts_kernel'), tr.records
        with dispatch_trace() as tr:
            out = ta.unique_consecutive(z, return_counts=True)
        assert out.inverse is None and torch.equal(out.counts.cat().data.cpu(), want[3])
        assert not tr.matching('seg_runs_inverse_kernel') and len(tr.matching('seg_runs_counts_kernel')) == 2, tr.records


def test_segment_form_and_degenerate_batches():
    lens = LT(WAVE_LENS)
    x = payload(draw_ids('random', lens, 22), F32, (5,))
    want = runs_cat(x, lens)
    values, sizes, inverse, counts = ta.segment_unique_consecutive(x.to(DEV), lens.to(DEV), True, True)
    assert same_bits(values, want[0]) and sizes.dtype == I64 and sizes.cpu().tolist() == want[1].tolist()
    assert torch.equal(inverse.cpu(), want[2]) and torch.equal(counts.cpu(), want[3])
    values, sizes, inverse, counts = ta.segment_unique_consecutive(x.to(DEV), lens.to(DEV))
    assert inverse is None and counts is None and same_bits(values, want[0])
    # all sequences empty, and no sequence at all
    for lens in (LT([0, 0, 0]), LT([])):
        for dtype, hidden in ((I64, ()), (F32, (5,))):
            x = torch.zeros((0,) + hidden, dtype=dtype)
            for kind in 'CLPR':
                out = check(kind, x, lens, f'empty B={lens.numel()}')
                assert out.values.data.numel() == 0 and out.counts.data.numel() == 0 and out.inverse.data.numel() == 0


# ------------------------------------------------------------------ identities
def test_identities_with_repeat_interleave_and_seg():
    lens = LT(WAVE_LENS)
    for dtype, hidden in ((I64, ()), (F32, (5,)), (BF16, (66,))):
        x = payload(draw_ids('random', lens, 23), dtype, hidden)
        for kind in 'CLPR':
            z = build(kind, x, lens)
            out = z.unique_consecutive(True, True)
            # values.repeat_interleave(counts) == z, bit for bit (no NaN, no mixed-sign zeros here)
            same_fields(out.values.repeat_interleave(out.counts), z, f'{kind} {dtype}: the round trip')
            # counts sum to the old lengths per sequence
            per_seq = [int(c.sum()) for c in split(out.counts.cat().data.cpu(), out.counts.cat().token_sizes.cpu())]
            assert per_seq == WAVE_LENS
            # values[b, inverse[b, t]] == z[b, t]
            v, i = out.values.cat(), out.inverse.cat().data.cpu()
            for seq, vb, ib in zip(split(x, lens), split(v.data.cpu(), v.token_sizes.cpu()), split(i, lens)):
                assert bool((vb[ib] == seq).all())


def count_read_backs(monkeypatch):
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    return calls


def test_one_read_back(monkeypatch):
    lens = LT(WAVE_LENS)
    x = payload(draw_ids('random', lens, 24), F32, (5,))
    zs = {kind: build(kind, x, lens) for kind in 'CLPR'}
    torch.cuda.synchronize()
    calls = count_read_backs(monkeypatch)
    for kind in 'CLPR':
        del calls[:]
        out = zs[kind].unique_consecutive(True, True)
        assert calls == [(len(WAVE_LENS),)], (kind, calls)
        c = out.values.cat()
        c.pack(), c.left(), c.right(), out.counts.cat().left()
        summed = zs[kind].seg(out.counts, ta.segment_sum)
        assert calls == [(len(WAVE_LENS),)], (kind, calls)
        # (repeat_interleave with tensor counts reads its OWN plan back — new lengths and the invalid-count word, B + 1
        # — and nothing for the lengths of `values` / `counts`)
        out.values.repeat_interleave(out.counts)
        assert calls == [(len(WAVE_LENS),), (len(WAVE_LENS) + 1,)], (kind, calls)
        assert summed.cat().data.shape == (out.values.cat().data.shape[0], 5)
    host = _meta._memo_get(zs['C'].unique_consecutive().values.token_sizes, 'host')
    assert host is not None and not host.is_cuda and host.tolist() == runs_cat(x, lens)[1].tolist()


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_gradient_goes_to_the_run_heads_only(dtype):
    """d (values.data * w).sum() / d z.data: w at the first token of every run, exact zeros at every other token — whole
    runs of inf are planted (a NaN token is always a head) — and at padding rows, which hold NaN."""
    lens = LT(WAVE_LENS)
    for hidden in ((), (9,)):
        form = 'lanes' if not hidden else 'rows'
        ids = draw_ids('random', lens, 25)
        x = payload(ids, dtype, hidden)
        x[ids == 2] = float('inf')                                 # runs of inf: equal, so only their heads get a gradient
        head = torch.cat([torch.cat([torch.ones(1, dtype=BOOL), s[1:] != s[:-1]]) for s in split(ids, lens) if s.numel()])
        for kind in 'CLPR':
            z = build(kind, x, lens, fill=float('nan'))
            leaf = z.data.clone().requires_grad_(True)
            with dispatch_trace() as tr:
                out = rewrap(z, leaf).unique_consecutive(True, True)
                assert out.values.data.requires_grad and not out.inverse.data.requires_grad
                assert not out.counts.data.requires_grad and out.counts.data.grad_fn is None
                w = torch.randn(out.values.data.shape, generator=torch.Generator().manual_seed(26)).to(dtype).to(DEV)
                (out.values.data * w).sum().backward()
            assert tr.matching(f'seg_compress_move_{form}_kernel expand=0'), tr.records
            assert tr.matching(f'seg_compress_move_{form}_kernel expand=1'), tr.records
            assert len(tr.matching('seg_compress_plan_kernel')) == 1, 'the backward plans nothing again'
            assert len(tr.matching('seg_runs_heads_' + form + '_kernel')) == 1, 'the backward compares nothing again'
            want = torch.zeros_like(x)
            want[head] = rewrap(out.values, w).cat().data.cpu()
            assert leaf.grad.dtype == dtype and same_bits(leaf.grad, build(kind, want, lens).data), (kind, hidden)


def test_gradcheck_and_double_backward():
    lens = LT([3, 0, 5])
    ids = LT([0, 0, 1, 2, 2, 2, 0, 0])
    x = payload(ids, F64, (2,))
    for kind in 'CLPR':
        z = build(kind, x, lens)
        leaf = z.data.clone().requires_grad_(True)
        # (finite differences stay inside the runs' pattern only where the perturbed token ends up a head either way: the
        # analytic gradient is that of the compress by the heads of the UNPERTURBED payload, so compare with that)
        out = rewrap(z, leaf).unique_consecutive().values
        cot = torch.randn(out.data.shape, dtype=F64, device=DEV).requires_grad_(True)
        g, = torch.autograd.grad(out.data, leaf, cot, create_graph=True)
        assert g.requires_grad and g.shape == leaf.shape
        head = LT([1, 0, 1, 1, 0, 0, 1, 0]).bool()
        want = torch.zeros(8, 2, dtype=F64)
        want[head] = rewrap(out, cot.detach()).cat().data.cpu()
        assert same_bits(g.detach(), build(kind, want, lens).data), kind
        v = torch.randn(leaf.shape, dtype=F64, device=DEV)
        gg, = torch.autograd.grad(g, cot, v)
        mask = build(kind, head, lens).data
        assert same_bits(gg, rewrap(z, v).compress(mask).data), kind
        # the Function pair itself: linear in the payload, so gradcheck / gradgradcheck apply to it with the rank fixed
        assert torch.autograd.gradcheck(lambda d: rewrap(z, d).compress(mask).data, (leaf,), nondet_tol=0.0)
        assert torch.autograd.gradgradcheck(lambda d: rewrap(z, d).compress(mask).data, (leaf,), nondet_tol=0.0)


def test_integer_and_bool_payloads_carry_no_graph():
    lens = LT(WAVE_LENS)
    for dtype in (I64, BOOL):
        x = payload(draw_ids('random', lens, 27), dtype, ())
        with torch.enable_grad():
            out = build('P', x, lens).unique_consecutive(True, True)
        assert not out.values.data.requires_grad and out.values.data.grad_fn is None and out.values.data.dtype == dtype
        assert same_bits(out.values.cat().data, runs_cat(x, lens)[0])


# ------------------------------------------------------------------ the CTC collapse, worked by hand
def test_ctc_greedy_collapse():
    """argmax ids -> collapse repeats -> drop blanks (0): 'hh_e_ll_llo' -> 'hello'."""
    blank, h, e, l, o = 0, 1, 2, 3, 4
    seqs = [[h, h, blank, e, blank, l, l, blank, l, l, o], [blank, blank, blank], [o, o, blank, o, h, h, h]]
    ids, lens = LT(sum(seqs, [])), LT([len(s) for s in seqs])
    for kind in 'CP':
        z = build(kind, ids, lens)
        collapsed = z.unique_consecutive().values
        assert collapsed.cat().data.cpu().tolist() == [h, blank, e, blank, l, blank, l, o, blank, o, blank, o, h]
        decoded = collapsed.compress(collapsed.data != blank)
        assert type(decoded) is type(z)
        assert decoded.cat().data.cpu().tolist() == [h, e, l, l, o, o, o, h]
        assert decoded.cat().token_sizes.cpu().tolist() == [5, 0, 3]
