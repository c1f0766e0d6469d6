"""Per-sequence join / unjoin on the GPU, bit for bit: every container against the yardstick of tests/join_util.py (plain
torch on the CPU), the two commutation identities field by field (PackedSequence metadata included), wave, block and cut
boundaries with the dispatch trace of every kernel form, every row width class, tensor parts, empty parts, padding,
device-only lengths, strided inputs, the read-backs of every path, and autograd of every order.  No tolerance anywhere:
rows move as bits and floats are compared through an integer view."""
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from join_util import as_seqs, cat, join_seqs, padded, same_bits, split, unjoin_seqs
from torchrua_amd import _meta

pytestmark = pytest.mark.gpu

WAVE_LENS = [0, 1, 7, 63, 64, 65, 129]         # around the wave boundaries; the second part takes the list reversed
SHORT_A = [30, 0, 1, 7, 31, 33, 32, 2, 0, 5]   # + SHORT_B: ten sequences (more than a workgroup's 8) with a bound of 64
SHORT_B = [34, 0, 63, 1, 33, 31, 0, 2, 1, 0]
BF16, F32, F64, I64, BOOL = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.bool
# (dtype, hidden, row bytes): the widths of test_gpu_compress.py
WIDTHS = [(BOOL, (), 1), (BF16, (1,), 2), (I64, (), 8), (F32, (4,), 16), (F32, (5,), 20), (F32, (2, 3), 24),
          (F32, (32,), 128), (F32, (33,), 132), (BF16, (512,), 1024)]


# ------------------------------------------------------------------ helpers
def LT(values):
    return torch.tensor(list(values), dtype=torch.long)


def draw(shape, dtype, seed):
    """Random payload on the CPU; floats carry a few NaNs and infinities (rows are bits: they must survive)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == BOOL:
        return torch.rand(shape, generator=g) < 0.5
    if dtype == I64:
        return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g)
    x = torch.randn(shape, generator=g).to(dtype)
    flat = x.view(-1)
    if flat.numel() >= 8:
        flat[1], flat[flat.numel() // 2], flat[-2] = float('nan'), float('inf'), float('-inf')
    return x


def build(kind, x, lens, device_lens=False):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.C(x.to(DEV), lens.to(DEV)) if device_lens else ta.with_host_sizes(x.to(DEV), lens)
    return {'C': lambda: c, 'L': c.left, 'R': c.right, 'P': c.pack}[kind]()


def fresh(z):
    """The same container over new metadata objects: nothing memoised, the lengths exist on the device only."""
    if isinstance(z, ta.P):
        return ta.P(z.data, z.batch_sizes.clone(), z.sorted_indices.clone(), z.unsorted_indices.clone())
    return z._replace(token_sizes=z.token_sizes.clone())


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def cast(c, kind):
    return {'C': lambda: c, 'L': c.left, 'R': c.right, 'P': c.pack}[kind]()


def same_fields(a, b, what):
    assert type(a) is type(b), what
    assert same_bits(a.data, b.data), f'{what}: data {tuple(a.data.shape)} vs {tuple(b.data.shape)}'
    if isinstance(a, ta.P):
        assert a.batch_sizes.dtype == b.batch_sizes.dtype and torch.equal(a.batch_sizes.cpu(), b.batch_sizes.cpu()), what
        assert torch.equal(a.sorted_indices, b.sorted_indices) and torch.equal(a.unsorted_indices, b.unsorted_indices), what
    else:
        assert a.token_sizes.dtype == b.token_sizes.dtype == I64 and torch.equal(a.token_sizes, b.token_sizes), what


def storage_ptr(t):
    return t.untyped_storage().data_ptr()


def check_join(kind, specs, what, device_lens=False):
    """join of the parts `specs` — (x, lens) in cat form on the CPU, or (x, None): a tensor part — as containers of
    `kind`: against the yardstick, in the container's own storage, and through both commutation identities.  Returns
    (result, the parts as given to join)."""
    parts = [x.to(DEV) if lens is None else build(kind, x, lens, device_lens) for x, lens in specs]
    datas = [p if isinstance(p, torch.Tensor) else p.data for p in parts]
    before = [d.clone() for d in datas]
    out = ta.join(parts)
    what = f'{what} {kind}'
    like = specs[0][0]
    assert type(out) is type(next(p for p in parts if not isinstance(p, torch.Tensor))) and out.data.dtype == like.dtype, what
    for d, d0 in zip(datas, before):
        assert same_bits(d, d0), f'{what}: an input changed'
        assert out.data.numel() == 0 or storage_ptr(out.data) != storage_ptr(d), f'{what}: the output aliases an input'
    seqs = join_seqs([as_seqs(x, lens) for x, lens in specs])
    want, want_lens = cat(seqs, like)
    got = out.cat()
    assert same_bits(got.data, want), f'{what}: payload'
    assert got.token_sizes.dtype == I64 and got.token_sizes.cpu().tolist() == want_lens.tolist(), f'{what}: lengths'
    if kind in 'LR':
        assert same_bits(out.data, padded(seqs, like, right=kind == 'R')), f'{what}: padded storage'
    # join([z_i]) == join([z_i.cat()]).X(), and join([z_i]).cat() == join([z_i.cat()])
    ref = ta.join([p if isinstance(p, torch.Tensor) else p.cat() for p in parts])
    same_fields(out, cast(ref, kind), f'{what}: X(join(cat))')
    same_fields(got, ref, f'{what}: cat(join)')
    return out, parts


def check_unjoin(kind, x, lens, sizes, what, device_lens=False):
    """unjoin of C(x, lens) cast to `kind` at `sizes` (ints, or CPU lists per sequence): every part against the
    yardstick, in its own storage, and through both commutation identities."""
    z = build(kind, x, lens, device_lens)
    before = z.data.clone()
    dev_sizes = [s if isinstance(s, int) else LT(s).to(DEV) for s in sizes]
    outs = ta.unjoin(z, dev_sizes)
    refs = ta.unjoin(z.cat(), dev_sizes)
    want = unjoin_seqs(split(x, lens), sizes)
    assert len(outs) == len(refs) == len(sizes) and same_bits(z.data, before), what
    for j, (out, ref, seqs) in enumerate(zip(outs, refs, want)):
        tag = f'{what} {kind} part {j}'
        assert type(out) is type(z) and (out.data.numel() == 0 or storage_ptr(out.data) != storage_ptr(z.data)), tag
        data, part_lens = cat(seqs, x)
        got = out.cat()
        assert same_bits(got.data, data), f'{tag}: payload'
        assert got.token_sizes.dtype == I64 and got.token_sizes.cpu().tolist() == part_lens.tolist(), f'{tag}: lengths'
        if kind in 'LR':
            assert same_bits(out.data, padded(seqs, x, right=kind == 'R')), f'{tag}: padded storage'
        same_fields(out, cast(ref, kind), f'{tag}: X(unjoin(cat))')
        same_fields(got, ref, f'{tag}: cat(unjoin)')
    return outs


def join_records(trace, **pairs):
    want = 'seg_join_kernel ' + ' '.join(f'{k}={v}' for k, v in pairs.items())
    return trace.matching(want)


# ------------------------------------------------------------------ every width class x every layout, at the wave boundaries
@pytest.mark.parametrize('dtype,hidden,row_bytes', WIDTHS, ids=[f'{rb}B' for _, _, rb in WIDTHS])
def test_widths_layouts(dtype, hidden, row_bytes):
    la, lb = LT(WAVE_LENS), LT(reversed(WAVE_LENS))
    a = draw((int(la.sum()),) + hidden, dtype, seed=row_bytes)
    b = draw((int(lb.sum()),) + hidden, dtype, seed=row_bytes + 1)
    assert a[0].numel() * a.element_size() == row_bytes
    for kind in 'CLPR':
        with dispatch_trace() as t:
            out, parts = check_join(kind, [(a, la), (b, lb)], f'{row_bytes}B')
        form = 'lanes' if row_bytes <= 16 else ('wave' if 129 * row_bytes <= 16384 else 'rows')   # 129: the longest joined sequence
        recs = join_records(t, form=form, row_bytes=row_bytes, unjoin=0, cut=0)
        assert len(recs) == 2 and len(join_records(t)) == 2, t.records          # the call and its cat-form twin
        # the inverse, field by field: unjoin at the parts' lengths gives the parts back
        back = ta.unjoin(out, [la.to(DEV), lb.to(DEV)])
        for got, part in zip(back, parts):
            same_fields(got, part, f'{row_bytes}B {kind}: unjoin(join)')


def test_lanes_form_beyond_one_workgroup():
    la, lb = LT(SHORT_A), LT(SHORT_B)
    assert len(SHORT_A) > 8 and int((la + lb).max()) == 64
    na, nb = int(la.sum()), int(lb.sum())
    a, b = draw((na + nb,), I64, 1), draw((na + nb, 2), F32, 2)
    for kind in 'CLPR':
        with dispatch_trace() as t:
            check_join(kind, [(a[:na], la), (a[na:], lb)], 'lanes int64')
            check_join(kind, [(b[:na], la), (b[na:], lb)], 'lanes 2 x f32')
        assert len(join_records(t, form='lanes', G=1, cut=0)) == len(join_records(t)) == 4, t.records


# ------------------------------------------------------------------ 1, 2, 3 and 8 parts; tensor parts; empty parts
def test_part_counts_tensor_parts_and_empty_parts():
    B, hidden = 6, (5,)
    lens = [LT([3, 0, 1, 4, 0, 2]), LT([0, 0, 2, 1, 0, 5]), LT([0] * B), LT([1, 0, 0, 0, 0, 7])]
    xs = [draw((int(n.sum()),) + hidden, F32, 20 + i) for i, n in enumerate(lens)]
    tok = draw((B,) + hidden, F32, 30)                            # one token per sequence
    P_ = [(x, n) for x, n in zip(xs, lens)]
    cases = {
        'one part (a copy)': [P_[0]],
        'one empty part': [P_[2]],
        'two parts': [P_[0], P_[1]],
        'everything empty': [P_[2], P_[2]],
        'three, one empty in all sequences': [P_[0], P_[2], P_[3]],
        'tensor first': [(tok, None), P_[0]],
        'tensor in the middle': [P_[1], (tok, None), P_[3]],
        'tensor last': [P_[0], P_[1], (tok, None)],
        'tensor around an empty part': [(tok, None), P_[2], (tok * 2, None)],
        'eight parts': [P_[0], P_[1], (tok, None), P_[2], P_[3], P_[0], (tok * 2, None), P_[1]],
    }
    for what, specs in cases.items():
        for kind in 'CLPR':
            out, parts = check_join(kind, specs, what)
            if what == 'one part (a copy)':
                same_fields(out, parts[0], f'{what} {kind}')
            if what == 'everything empty':
                assert out.data.numel() == 0 and out.cat().token_sizes.cpu().tolist() == [0] * B
                if kind == 'P':
                    assert out.batch_sizes.numel() == 0 and out.sorted_indices.numel() == B
    # a result with empty sequences packs exactly as C.pack() does (sequences 1 and 4 are empty in parts 0 and 1)
    out, _ = check_join('P', [P_[0], P_[1]], 'empty sequences')
    want = ta.with_host_sizes(out.cat().data, lens[0] + lens[1]).pack()
    same_fields(out, want, 'empty sequences in a P')
    # 1-D payloads with a tensor part [B]
    ids, bos = draw((int(lens[0].sum()),), I64, 40), draw((B,), I64, 41)
    for kind in 'CLPR':
        check_join(kind, [(bos, None), (ids, lens[0]), (bos + 1, None)], 'BOS + ids + EOS')


def test_packed_parts_whose_sort_orders_differ():
    la, lb = LT([1, 2, 2, 5, 9, 9, 12]), LT([12, 9, 9, 5, 2, 2, 2])          # ascending, descending, with ties
    a, b = draw((int(la.sum()), 3), F32, 50), draw((int(lb.sum()), 3), F32, 51)
    out, parts = check_join('P', [(a, la), (b, lb)], 'sort orders')
    assert not torch.equal(parts[0].sorted_indices, parts[1].sorted_indices)
    want = ta.with_host_sizes(out.cat().data, la + lb).pack()                 # C.pack() of the summed lengths
    same_fields(out, want, 'the order of the summed lengths')
    assert torch.equal(out.sorted_indices.cpu(), torch.sort(la + lb, descending=True)[1])
    for got, part in zip(out.unjoin(la.to(DEV), lb.to(DEV)), parts):
        same_fields(got, part, 'unjoin gives each part its own order back')


# ------------------------------------------------------------------ block and cut boundaries
@pytest.mark.parametrize('total', [2047, 2048, 2049])
def test_one_sequence_across_the_block_boundary(total):
    la, lb = LT([2040]), LT([total - 2040])                       # the second part straddles token 2048
    a, b = draw((2040, 8), F32, total), draw((total - 2040, 8), F32, total + 1)
    for kind in 'CLPR':
        with dispatch_trace() as t:
            check_join(kind, [(a, la), (b, lb)], f'{total} tokens')
        assert len(join_records(t, form='rows', cut=0, G=2)) == len(join_records(t)) == 2, t.records
        check_unjoin(kind, torch.cat([a, b]), la + lb, [2040, [total]], f'{total} tokens')


@pytest.mark.parametrize('dtype,hidden,row_bytes', [(I64, (), 8), (F32, (8,), 32)], ids=['8B', '32B'])
def test_cut_form_equals_uncut(dtype, hidden, row_bytes):
    """Three long sequences: the cut rule applies (a workgroup per block of 2 048 tokens, narrow rows too).  The same
    data as the head of 1 030 sequences: no cut (lanes form at 8 bytes, rows form at 32).  The common prefix agrees."""
    la, lb = [9000, 10000, 9500], [10000, 9000, 9999]
    a, b = draw((sum(la),) + hidden, dtype, 60), draw((sum(lb),) + hidden, dtype, 61)
    many = 1027
    a2, b2 = torch.cat([a, a[:many]]), torch.cat([b, b[:many]])
    for kind in 'CLPR':
        with dispatch_trace() as t:
            out, _ = check_join(kind, [(a, LT(la)), (b, LT(lb))], f'cut {row_bytes}B')
        blocks = -(-max(x + y for x, y in zip(la, lb)) // 2048)
        recs = join_records(t, form='rows', cut=1, blocks=blocks, row_bytes=row_bytes)
        assert len(recs) == len(join_records(t)) == 2, t.records
        if kind in 'LR':
            continue                                              # (1 030 x 19 999 padded rows: the cat forms cover it)
        with dispatch_trace() as t:
            big = ta.join([build(kind, a2, LT(la + [1] * many)), build(kind, b2, LT(lb + [1] * many))])
        assert len(join_records(t, form='lanes' if row_bytes <= 16 else 'rows', cut=0)) == len(join_records(t)) == 1, t.records
        n = sum(la) + sum(lb)
        assert same_bits(big.cat().data[:n], out.cat().data), f'cut == uncut {kind}'


def test_cut_unjoin():
    lens = [9000, 20000, 8193]
    x = draw((sum(lens), 8), F32, 62)
    for kind in 'CP':
        with dispatch_trace() as t:
            check_unjoin(kind, x, LT(lens), [[100, 10000, 0], 7000, [5000, 9000, 5000]], 'cut unjoin')
        assert len(join_records(t, form='rows', cut=1, unjoin=1)) == len(join_records(t)) == 2, t.records


# ------------------------------------------------------------------ padding that must not leak
def test_padded_parts_with_spare_rows_and_nan_padding():
    la, lb = LT([3, 0, 5, 1]), LT([2, 4, 0, 1])
    a, b = torch.randn(9, 3), torch.randn(7, 3)
    seqs = join_seqs([as_seqs(a, la), as_seqs(b, lb)])
    for kind, cls in (('L', ta.L), ('R', ta.R)):
        parts = []
        for x, lens in ((a, la), (b, lb)):
            t_log, t_phys = int(lens.max()), int(lens.max()) + 3
            data = torch.full((4, t_phys, 3), float('nan'))
            data[:, :t_log] = padded(split(x, lens), x, right=kind == 'R')
            for i, n in enumerate(lens.tolist()):                 # NaN in every padding row, inside T_log too
                if kind == 'L':
                    data[i, n:] = float('nan')
                else:
                    data[i, :t_log - n] = float('nan')
            parts.append(cls(data.to(DEV), lens.to(DEV)))
        out = ta.join(parts)
        assert same_bits(out.data, padded(seqs, a, right=kind == 'R')), kind
        back = ta.unjoin(out, [la.to(DEV), lb.to(DEV)])
        for got, (x, lens) in zip(back, ((a, la), (b, lb))):
            assert same_bits(got.data, padded(split(x, lens), x, right=kind == 'R')), kind
        # an unjoin of a container with spare rows and NaN padding: nothing leaks either
        first, second = ta.unjoin(parts[0], [2, la.to(DEV)])
        want = unjoin_seqs(split(a, la), [2, la.tolist()])
        assert same_bits(first.data, padded(want[0], a, right=kind == 'R'))
        assert same_bits(second.data, padded(want[1], a, right=kind == 'R'))


def test_non_contiguous_inputs():
    la, lb = LT(SHORT_A), LT(SHORT_B)
    wide_a, wide_b = draw((int(la.sum()), 8), F32, 70), draw((int(lb.sum()), 8), F32, 71)
    tok = draw((len(SHORT_A), 8), F32, 72)
    a, b = wide_a[:, 1:6], wide_b[:, 1:6]
    seqs = join_seqs([as_seqs(a, la), as_seqs(tok[:, 1:6]), as_seqs(b, lb)])
    for kind in 'CLPR':
        za, zb = build(kind, wide_a, la), build(kind, wide_b, lb)
        za, zb = rewrap(za, za.data[..., 1:6]), rewrap(zb, zb.data[..., 1:6])         # column slices
        assert not za.data.is_contiguous()
        out = ta.join([za, tok.to(DEV)[:, 1:6], zb])
        assert same_bits(out.cat().data, cat(seqs, a)[0]), kind
        cut = ta.unjoin(za, [3, 100])
        want = unjoin_seqs(split(a, la), [3, 100])
        for got, w in zip(cut, want):
            assert same_bits(got.cat().data, cat(w, a)[0]), kind


def test_lengths_that_exist_on_the_device_only():
    la, lb = LT(WAVE_LENS), LT(reversed(WAVE_LENS))
    a, b = draw((int(la.sum()), 5), F32, 80), draw((int(lb.sum()), 5), F32, 81)
    tok = draw((len(WAVE_LENS), 5), F32, 82)
    for kind in 'CLPR':
        check_join(kind, [(a, la), (tok, None), (b, lb)], 'device lengths', device_lens=True)
        check_unjoin(kind, a, la, [[1] * 7, 60, la.tolist()], 'device lengths', device_lens=True)


# ------------------------------------------------------------------ unjoin
def test_unjoin_sizes():
    lens = LT(WAVE_LENS)
    x = draw((int(lens.sum()), 5), F32, 90)
    ids = draw((int(lens.sum()),), I64, 91)
    cases = {
        'python ints': [1, 63, 2],
        'the tail dropped': [[0, 1, 3, 10, 10, 10, 10], [0, 0, 2, 20, 20, 20, 100]],
        'past the end (clamped)': [[0, 0, 5, 70, 64, 1000, 100], 40, [7] * 7],
        'a zero size': [0, [5] * 7],
        'mixed': [[1] * 7, 5, [0, 0, 0, 60, 0, 60, 0]],
    }
    for what, sizes in cases.items():
        for kind in 'CLPR':
            outs = check_unjoin(kind, x, lens, sizes, what)
            check_unjoin(kind, ids, lens, sizes, what + ' int64')
            if what == 'past the end (clamped)':
                assert outs[0].cat().token_sizes.cpu().tolist() == [0, 0, 5, 63, 64, 65, 100]
                assert outs[1].cat().token_sizes.cpu().tolist() == [0, 1, 2, 0, 0, 0, 29]
                assert outs[2].cat().token_sizes.cpu().tolist() == [0] * 7
    z = build('C', x, lens)
    assert all(same_bits(m.data, f.data) for m, f in zip(z.unjoin(1, 63, 2), ta.unjoin(z, [1, 63, 2])))


# ------------------------------------------------------------------ synchronisation
def count_read_backs(monkeypatch):
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    return calls


def test_read_backs(monkeypatch):
    la, lb = LT(WAVE_LENS), LT(reversed(WAVE_LENS))
    a, b = draw((int(la.sum()), 5), F32, 100), draw((int(lb.sum()), 5), F32, 101)
    tok = draw((7, 5), F32, 102).to(DEV)
    built = {kind: (build(kind, a, la), build(kind, b, lb)) for kind in 'CLPR'}
    torch.cuda.synchronize()
    calls = count_read_backs(monkeypatch)
    for kind in 'CLPR':
        # every part carries host lengths: nothing is read back, by the call or by the casts that follow
        za, zb = built[kind]
        out = ta.join([za, tok, zb])
        out.cat(), out.pack(), out.left(), out.right(), out.size()
        for part in ta.unjoin(out, [3, za.cat().token_sizes, 2]):
            part.cat(), part.pack(), part.left(), part.right()
        assert calls == [], (kind, calls)
    # a C result never synchronises, with lengths that exist on the device only
    ca, cb = fresh(built['C'][0]), fresh(built['C'][1])
    out = ta.join([ca, tok, cb])
    assert calls == [] and out.data.shape[0] == a.shape[0] + b.shape[0] + 7
    assert same_bits(out.data, cat(join_seqs([as_seqs(a, la), as_seqs(tok.cpu()), as_seqs(b, lb)]), a)[0])
    # ... but an unjoin sizes its parts' storages from lengths the host has never seen: ONE read-back
    parts = ta.unjoin(fresh(built['C'][0]), [2, 5])
    assert calls == [(3, 7)], calls                               # the two parts' lengths and its own, in one copy
    parts[0].left(), parts[1].pack()
    assert calls == [(3, 7)], calls
    # a part whose storage holds more rows than its lengths add up to: the spare rows of the result are zeros
    spare = ta.C(torch.cat([built['C'][0].data, tok]), built['C'][0].token_sizes.clone())
    out = ta.join([spare, fresh(built['C'][1])])
    assert calls == [(3, 7)] and out.data.shape[0] == a.shape[0] + 7 + b.shape[0]
    want = torch.cat([cat(join_seqs([as_seqs(a, la), as_seqs(b, lb)]), a)[0], torch.zeros(7, 5)])
    assert same_bits(out.data, want)
    # an L / R / P result from device-only lengths: exactly ONE read-back, and none for the casts that follow
    for kind in 'LRP':
        del calls[:]
        za, zb = fresh(built[kind][0]), fresh(built[kind][1])
        out = ta.join([za, tok, zb])
        assert calls == [(4, 7)], (kind, calls)                    # the sums and the three parts' own, in one copy
        out.cat(), out.pack(), out.left(), out.right(), out.size(), za.cat(), zb.cat()
        assert calls == [(4, 7)], (kind, calls)
        want = cat(join_seqs([as_seqs(a, la), as_seqs(tok.cpu()), as_seqs(b, lb)]), a)[0]
        assert same_bits(out.cat().data, want), kind
        del calls[:]
        parts = ta.unjoin(fresh(out), [1, la.to(DEV), 100])
        assert calls == [(4, 7)], (kind, calls)                    # the three parts' lengths and its own, in one copy
        n = len(calls)
        for part in parts:
            part.cat(), part.pack(), part.left(), part.right()
        assert len(calls) == n, (kind, calls)


# ------------------------------------------------------------------ autograd
def nan_padding(z):
    """The same L / R with NaN in every padding row (a leaf that requires grad)."""
    data = z.data.clone()
    if isinstance(z, (ta.L, ta.R)):
        T = data.shape[1]
        pos = torch.arange(T, device=DEV)[None, :]
        n = z.token_sizes[:, None]
        pad = pos >= n if isinstance(z, ta.L) else pos < T - n
        data[pad] = float('nan')
    return data.requires_grad_(True)


def cat_rows(z, data):
    """`data`, a tensor of the storage shape of `z`, as cat-form rows on the CPU."""
    return data.detach().cpu() if isinstance(z, torch.Tensor) else rewrap(z, data.detach()).cat().data.cpu()


def padding_is_zero(z, grad):
    if not isinstance(z, (ta.L, ta.R)):
        return True
    T = grad.shape[1]
    pos = torch.arange(T, device=DEV)[None, :]
    n = z.token_sizes[:, None]
    pad = pos >= n if isinstance(z, ta.L) else pos < T - n
    return not bool(grad[pad].view(torch.int32).any())            # exact zeros: not a bit set


def test_autograd_of_join():
    la, lb = LT(WAVE_LENS), LT(reversed(WAVE_LENS))
    B, hidden = len(WAVE_LENS), (3,)
    a, b = torch.randn(int(la.sum()), 3), torch.randn(int(lb.sum()), 3)
    for kind in 'CLPR':
        za, zb = build(kind, a, la), build(kind, b, lb)
        da, db = nan_padding(za), nan_padding(zb)
        tok = torch.randn((B,) + hidden, device=DEV, requires_grad=True)
        parts = [rewrap(za, da), tok, rewrap(zb, db)]
        out = ta.join(parts)
        assert out.data.grad_fn is not None
        w = torch.randn(out.data.shape, device=DEV)
        grads = torch.autograd.grad((out.data * w).sum(), [da, tok, db])
        # the yardstick: the cotangent, cut where the parts were glued — a permutation of rows plus zeros
        w_seqs = split(cat_rows(out, w), la + 1 + lb)
        want = unjoin_seqs(w_seqs, [la.tolist(), 1, lb.tolist()])
        for z, g, seqs in zip(parts, grads, want):
            assert same_bits(cat_rows(z, g), cat(seqs, a)[0]), kind
            assert padding_is_zero(z, g), f'{kind}: the gradient of a padding row is not an exact zero'
        # twice: the gradient w.r.t. the cotangent of the gradients is the join again
        wg = w.clone().requires_grad_(True)
        g1 = torch.autograd.grad(out.data, [da, tok, db], grad_outputs=wg, create_graph=True)
        assert all(g.grad_fn is not None for g in g1)
        vs = [torch.randn_like(g) for g in g1]
        g2, = torch.autograd.grad(sum((g * v).sum() for g, v in zip(g1, vs)), wg)
        same = ta.join([v if isinstance(z, torch.Tensor) else rewrap(z, v) for z, v in zip(parts, vs)])
        assert same_bits(g2, same.data), kind
        # only some parts ask for a gradient
        out = ta.join([za, tok, zb])
        g, = torch.autograd.grad((out.data * w).sum(), [tok])
        assert same_bits(g, grads[1]), kind


def test_autograd_of_unjoin():
    lens = LT(WAVE_LENS)
    x = torch.randn(int(lens.sum()), 3)
    sizes = [[0, 1, 3, 10, 10, 10, 10], 2, [0, 0, 2, 20, 20, 20, 100]]          # a dropped tail in the longer sequences
    for kind in 'CLPR':
        z = build(kind, x, lens)
        d = nan_padding(z)
        zz = rewrap(z, d)
        outs = ta.unjoin(zz, [s if isinstance(s, int) else LT(s).to(DEV) for s in sizes])
        assert all(o.data.grad_fn is not None for o in outs)
        ws = [torch.randn(o.data.shape, device=DEV) for o in outs]
        g, = torch.autograd.grad(sum((o.data * w).sum() for o, w in zip(outs, ws)), d)
        # the yardstick: the join of the cotangents, zeros for the dropped tokens
        w_seqs = [split(cat_rows(o, w), o.cat().token_sizes.cpu()) for o, w in zip(outs, ws)]
        want = []
        for i, n in enumerate(lens.tolist()):
            rows = torch.cat([p[i] for p in w_seqs])
            want.append(torch.cat([rows, torch.zeros(n - rows.shape[0], 3)]))
        assert same_bits(cat_rows(zz, g), torch.cat(want)), kind
        assert padding_is_zero(zz, g), kind


def test_integer_and_bool_payloads_carry_no_graph():
    lens = LT([2, 0, 3])
    for x in (draw((5,), I64, 110), draw((5, 2), BOOL, 111)):
        for kind in 'CLPR':
            z = build(kind, x, lens)
            out = ta.join([z, z])
            assert out.data.grad_fn is None and not out.data.requires_grad
            assert all(p.data.grad_fn is None for p in ta.unjoin(out, [lens.to(DEV), 1]))


# ------------------------------------------------------------------ the segment_* forms
def test_segment_forms_are_the_container_forms():
    la, lb = LT(WAVE_LENS), LT(reversed(WAVE_LENS))
    a, b = draw((int(la.sum()), 5), F32, 120), draw((int(lb.sum()), 5), F32, 121)
    data, sizes = ta.segment_join([a.to(DEV), b.to(DEV)], [la.to(DEV), lb.to(DEV)])
    want = ta.join([ta.C(a.to(DEV), la.to(DEV)), ta.C(b.to(DEV), lb.to(DEV))])
    assert same_bits(data, want.data) and sizes.dtype == I64 and torch.equal(sizes, want.token_sizes)
    assert same_bits(data, cat(join_seqs([as_seqs(a, la), as_seqs(b, lb)]), a)[0])
    pieces = ta.segment_unjoin(data, sizes, [la.to(DEV), 3, lb.to(DEV)])
    twins = ta.unjoin(ta.C(data, sizes), [la.to(DEV), 3, lb.to(DEV)])
    assert len(pieces) == 3
    for (d, s), twin in zip(pieces, twins):
        assert same_bits(d, twin.data) and torch.equal(s, twin.token_sizes)
    assert same_bits(pieces[0][0], a) and pieces[0][1].cpu().tolist() == WAVE_LENS
