"""Per-sequence repeat_interleave on the GPU: every container against the yardstick of tests/repeat_util.py (stock
torch.repeat_interleave per sequence on the CPU), bit for bit; the commutation identities field by field (PackedSequence
metadata included); every form boundary of the plan, the cut geometry, every row width class; int counts; the compress
and seg identities; synchronisation; invalid counts; the backward (exact where sums are exact, a derived bound against
fp64 elsewhere, gradcheck of both orders, reproducibility) and the dispatch trace for every kernel form."""
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from repeat_util import padded, repeat, repeat_cat, repeat_grad_cat, same_bits, split
from torchrua_amd import _meta

pytestmark = pytest.mark.gpu

BLOCK = 2048                                   # SEG_BLOCK_TOK of csrc/rua_seg_plan.h
BF16, F16, F32, F64, I64, I8, BOOL = (torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64,
                                      torch.int8, torch.bool)
# the plan's forms go by the longest sequence: <= 64 lanes, < 2 048 rows, longer long; few and >= 8 192 cut
BATCHES = {
    'lanes': [64, 0, 1, 7, 63, 33, 32, 2, 64],
    'rows': [0, 1, 63, 64, 65, 2047],
    'long': [3, 2048, 0, 2049, 65, 2047],
    'one': [130],                                                        # B = 1
    'cut': [9000, 8999, 9001],
}
WAVE_LENS = [0, 1, 7, 63, 64, 65, 129]
# (dtype, hidden, row bytes)
WIDTHS = [(I64, (), 8), (BOOL, (), 1), (BF16, (), 2), (I8, (3,), 3), (BF16, (5,), 10), (F32, (4,), 16), (F32, (32,), 128),
          (BF16, (500,), 1000)]


# ------------------------------------------------------------------ helpers
def LT(values):
    return torch.tensor(list(values), dtype=torch.long)


def draw(shape, dtype, seed):
    """Random payload on the CPU; floats are random BITS, so NaN patterns of every kind and infinities are among them."""
    g = torch.Generator().manual_seed(seed)
    if dtype == BOOL:
        return torch.rand(shape, generator=g) < 0.5
    if dtype == I64:
        return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g)
    if dtype == I8:
        return torch.randint(-128, 128, shape, generator=g).to(I8)
    if dtype in (BF16, F16):
        return torch.randint(-2 ** 15, 2 ** 15, shape, generator=g).to(torch.int16).view(dtype)
    if dtype == F32:
        return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g).to(torch.int32).view(dtype)
    return torch.randn(shape, generator=g, dtype=dtype)


def draw_counts(lens, seed, big=(70, 300, 5000), top=3):
    """Counts from {0 .. top} with the `big` ones planted in the longest sequence; the first sequence that has two tokens
    gets a leading and a trailing zero, the last non-empty one is all zeros."""
    g = torch.Generator().manual_seed(seed)
    n = int(lens.sum())
    counts = torch.randint(0, top + 1, (n,), generator=g)
    off = [0] + torch.cumsum(lens, 0).tolist()
    longest = int(torch.argmax(lens))
    for i, v in enumerate(big):
        if lens[longest] > 2 * i + 1:
            counts[off[longest] + (int(lens[longest]) * (i + 1)) // (len(big) + 1)] = v
    for b, length in enumerate(lens.tolist()):
        if length >= 2 and b != longest:
            counts[off[b]] = 0
            counts[off[b] + length - 1] = 0
            break
    for b in reversed(range(len(lens))):
        if lens[b] > 0 and b != longest:
            counts[off[b]:off[b + 1]] = 0
            break
    return counts


def build(kind, x, lens, fill=0, device_lens=False):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.C(x.to(DEV), lens.to(DEV)) if device_lens else ta.with_host_sizes(x.to(DEV), lens)
    return {'C': lambda: c, 'L': lambda: c.left(fill), 'R': lambda: c.right(fill), 'P': c.pack}[kind]()


def counts_like(kind, counts, lens, device_lens=False):
    """The counts cast the same way as the data; padding rows of an L / R hold NEGATIVE counts (never read)."""
    return build(kind, counts, lens, fill=-5, device_lens=device_lens).data


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def same_fields(a, b, what):
    assert type(a) is type(b), what
    assert same_bits(a.data, b.data), f'{what}: data {tuple(a.data.shape)} vs {tuple(b.data.shape)}'
    if isinstance(a, ta.P):
        assert a.batch_sizes.dtype == b.batch_sizes.dtype and torch.equal(a.batch_sizes.cpu(), b.batch_sizes.cpu()), what
        assert torch.equal(a.sorted_indices, b.sorted_indices) and torch.equal(a.unsorted_indices, b.unsorted_indices), what
    else:
        assert a.token_sizes.dtype == b.token_sizes.dtype == I64 and torch.equal(a.token_sizes, b.token_sizes), what


def cast(kind, c):
    return {'C': lambda: c, 'L': c.left, 'R': c.right, 'P': c.pack}[kind]()


def check(kind, x, counts, lens, what, want=None):
    """z.repeat_interleave(r) against the yardstick and both commutation identities; returns the result."""
    z, r = build(kind, x, lens), counts_like(kind, counts, lens)
    x_before, r_before = z.data.clone(), r.clone()
    out = z.repeat_interleave(r)
    what = f'{what} {kind}'
    assert type(out) is type(z) and out.data.dtype == x.dtype, what
    assert same_bits(z.data, x_before) and torch.equal(r, r_before), f'{what}: an input changed'
    want, want_lens = repeat_cat(x, counts, lens) if want is None else want
    got = out.cat()
    assert got.token_sizes.dtype == I64 and got.token_sizes.cpu().tolist() == want_lens.tolist(), f'{what}: lengths'
    assert same_bits(got.data, want), f'{what}: payload'
    if kind in 'LR':       # T' = the longest new sequence, padding rows exact zeros
        assert same_bits(out.data, padded(split(want, want_lens), x, right=kind == 'R')), f'{what}: padded storage'
    # z.repeat_interleave(r) == z.cat().repeat_interleave(r_as_cat).X(), and .cat() of it == the inner result
    rc = counts.to(DEV) if kind == 'C' else rewrap(z, r).cat().data
    ref = z.cat().repeat_interleave(rc)
    same_fields(out, cast(kind, ref), f'{what}: X(repeat(cat))')
    same_fields(got, ref, f'{what}: cat(repeat)')
    return out


# ------------------------------------------------------------------ the plan's forms, every layout
@pytest.mark.parametrize('name', list(BATCHES))
def test_form_boundaries(name):
    lens = LT(BATCHES[name])
    plan = {'one': 'rows'}.get(name, name)
    for dtype, hidden in ((F32, (4,)), (I64, ())):
        x = draw((int(lens.sum()),) + hidden, dtype, 1)
        counts = draw_counts(lens, 2)
        want = repeat_cat(x, counts, lens)
        for kind in 'CLPR':
            with dispatch_trace() as tr:
                check(kind, x, counts, lens, name, want)
            assert tr.matching(f'seg_repeat_plan_kernel form={plan}'), tr.records
            assert tr.matching('seg_repeat_move_kernel form=lanes table=1'), tr.records
            if name == 'cut':
                assert tr.matching('seg_repeat_plan_kernel form=cut phase=sum blocks=5'), tr.records
                assert tr.matching('seg_repeat_plan_kernel form=cut phase=finish blocks=5'), tr.records
                assert tr.matching('seg_repeat_move_kernel cut=1'), tr.records
            else:
                assert not tr.matching('seg_repeat_plan_kernel form=cut'), tr.records


def test_cut_move_of_wide_rows_and_all_zero_batch():
    lens = LT(BATCHES['cut'])
    x = draw((int(lens.sum()), 5), F32, 3)
    counts = draw_counts(lens, 4)
    with dispatch_trace() as tr:
        check('C', x, counts, lens, 'cut rows')
        check('P', x, counts, lens, 'cut rows')
    assert tr.matching('seg_repeat_move_kernel form=rows cut=1'), tr.records
    n = sum(WAVE_LENS)
    for kind in 'CLPR':
        out = check(kind, x[:n], torch.zeros(n, dtype=I64), LT(WAVE_LENS), 'all-zero batch')
        assert out.data.numel() == 0 and out.cat().token_sizes.cpu().tolist() == [0] * len(WAVE_LENS)


def test_device_only_lengths_take_the_long_plan():
    """C(data, token_sizes_on_device): the host never saw the lengths, the bound is the row count."""
    lens = LT(WAVE_LENS + [BLOCK + 5])
    x, counts = draw((int(lens.sum()), 5), F32, 5), draw_counts(lens, 6)
    with dispatch_trace() as tr:
        out = ta.C(x.to(DEV), lens.to(DEV)).repeat_interleave(counts.to(DEV))
    assert tr.matching('seg_repeat_plan_kernel form=long'), tr.records
    want, want_lens = repeat_cat(x, counts, lens)
    assert same_bits(out.data, want) and out.token_sizes.cpu().tolist() == want_lens.tolist()


# ------------------------------------------------------------------ every row width class
@pytest.mark.parametrize('dtype,hidden,row_bytes', WIDTHS, ids=[f'{rb}B' for _, _, rb in WIDTHS])
def test_widths(dtype, hidden, row_bytes):
    lens = LT(WAVE_LENS)
    x = draw((int(lens.sum()),) + hidden, dtype, seed=row_bytes)
    assert x[0].numel() * x.element_size() == row_bytes
    counts = draw_counts(lens, 7, big=(70, 300))
    want = repeat_cat(x, counts, lens)
    for kind in 'CLPR':
        with dispatch_trace() as tr:
            check(kind, x, counts, lens, f'{row_bytes}B', want)
        assert tr.matching(f'seg_repeat_move_kernel form={"rows" if row_bytes > 16 else "lanes"}'), tr.records
    # a payload view whose base sits 8 bytes into its allocation: accesses of at most 8 bytes
    if row_bytes % 8 == 0:
        raw = torch.empty(x.numel() * x.element_size() + 8, dtype=torch.uint8, device=DEV)
        view = raw[8:].view(dtype).view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == 8
        with dispatch_trace() as tr:
            out = ta.with_host_sizes(view, lens).repeat_interleave(counts.to(DEV))
        assert tr.matching('seg_repeat_move_kernel W=8'), tr.records
        assert same_bits(out.data, want[0])


def test_nan_bits_survive():
    lens = LT(WAVE_LENS)
    for dtype in (F32, BF16):
        x = draw((int(lens.sum()), 3), dtype, 8)
        assert bool(x.isnan().any())
        counts = draw_counts(lens, 9, big=())
        out = build('P', x, lens).repeat_interleave(counts_like('P', counts, lens))
        assert same_bits(out.cat().data, repeat_cat(x, counts, lens)[0])


# ------------------------------------------------------------------ int counts, identities
def test_int_counts_equal_filled_tensors():
    lens = LT(WAVE_LENS)
    for dtype, hidden in ((F32, (5,)), (I64, ())):
        x = draw((int(lens.sum()),) + hidden, dtype, 10)
        for r in (0, 1, 2, 7):
            filled = torch.full((int(lens.sum()),), r, dtype=I64)
            for kind in 'CLPR':
                z = build(kind, x, lens)
                with dispatch_trace() as tr:
                    got = z.repeat_interleave(r)
                assert not tr.matching('seg_repeat_plan_kernel'), 'an int count plans nothing'
                assert r == 0 or tr.matching('seg_repeat_move_kernel table=0'), tr.records
                same_fields(got, z.repeat_interleave(counts_like(kind, filled, lens)), f'r={r} {kind}')
                if r == 1:
                    same_fields(got, z, f'identity {kind}')
                if r == 0:
                    assert got.cat().token_sizes.cpu().tolist() == [0] * len(WAVE_LENS)


def test_compress_and_seg_identities():
    lens = LT(WAVE_LENS)
    x = torch.randn(int(lens.sum()), 5, generator=torch.Generator().manual_seed(11))
    mask = torch.rand(int(lens.sum()), generator=torch.Generator().manual_seed(12)) < 0.5
    d = torch.randint(1, 4, (int(lens.sum()),), generator=torch.Generator().manual_seed(13))
    for kind in 'CLPR':
        z = build(kind, x, lens)
        m = build(kind, mask, lens, fill=True).data
        same_fields(z.repeat_interleave(m.long()), z.compress(m), f'compress {kind}')
        same_fields(z.repeat_interleave(torch.ones_like(m, dtype=I64)), z, f'ones {kind}')
        # un-pooling: the max over d >= 1 copies of a token is the token, exactly
        back = z.repeat_interleave(counts_like(kind, d, lens)).seg(ta.with_host_sizes(d.to(DEV), lens), ta.segment_max)
        same_fields(back.cat(), z.cat(), f'seg {kind}')


def test_segment_repeat_interleave_is_the_cat_form():
    lens = LT(WAVE_LENS)
    x, counts = draw((int(lens.sum()), 5), F32, 14), draw_counts(lens, 15)
    data, sizes = ta.segment_repeat_interleave(x.to(DEV), counts.to(DEV), lens.to(DEV))
    want, want_lens = repeat_cat(x, counts, lens)
    assert same_bits(data, want) and sizes.dtype == I64 and sizes.cpu().tolist() == want_lens.tolist()
    c = ta.with_host_sizes(x.to(DEV), lens).repeat_interleave(counts.to(DEV))
    assert same_bits(data, c.data) and torch.equal(sizes, c.token_sizes)
    data, sizes = ta.segment_repeat_interleave(x.to(DEV), 2, lens.to(DEV))
    assert same_bits(data, torch.repeat_interleave(x, 2, dim=0)) and sizes.cpu().tolist() == (2 * lens).tolist()


# ------------------------------------------------------------------ synchronisation
def count_read_backs(monkeypatch):
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    return calls


def test_read_backs(monkeypatch):
    lens = LT(WAVE_LENS)
    x, counts = draw((int(lens.sum()), 5), F32, 16), draw_counts(lens, 17)
    zs = {kind: build(kind, x, lens) for kind in 'CLPR'}
    rs = {kind: counts_like(kind, counts, lens) for kind in 'CLPR'}
    dev_only = ta.C(x.to(DEV), lens.to(DEV))
    torch.cuda.synchronize()
    calls = count_read_backs(monkeypatch)
    # an int count and lengths the host knows: nothing is read back, whatever the layout
    for kind in 'CLPR':
        zs[kind].repeat_interleave(3)
        assert calls == [], (kind, calls)
    # a C result never synchronises, with lengths that exist on the device only
    out = dev_only.repeat_interleave(3)
    assert calls == [] and _meta._memo_get(out.token_sizes, 'host') is None
    # tensor counts: exactly one copy, of the new lengths and the invalid-count word; the casts that follow add none
    for kind in 'CLPR':
        del calls[:]
        out = zs[kind].repeat_interleave(rs[kind])
        assert calls == [(len(WAVE_LENS) + 1,)], (kind, calls)
        c = out.cat()
        c.pack(), c.left(), c.right()
        assert calls == [(len(WAVE_LENS) + 1,)], (kind, calls)
    host = _meta._memo_get(zs['C'].repeat_interleave(rs['C']).token_sizes, 'host')
    assert host is not None and not host.is_cuda and host.tolist() == repeat_cat(x, counts, lens)[1].tolist()


# ------------------------------------------------------------------ invalid counts
def test_invalid_counts_raise():
    lens = LT([3, 0, 5])
    x = torch.randn(8, 2)
    for bad, n in (([1, -1, 2, 0, 1, 1, 1, 1], 1), ([1, 2 ** 31, 2, 0, 1, -7, 1, 1], 2), ([2 ** 31] + [1] * 7, 1)):
        for kind in 'CLPR':
            z, r = build(kind, x, lens), counts_like(kind, LT(bad), lens)
            with pytest.raises(ta.RuaError, match=f'{n} invalid count'):
                z.repeat_interleave(r)
    # 2^31 - 1 is a valid count (not run: it would allocate); negative counts in the padding rows of an L do not raise
    l = build('L', x, lens)
    out = l.repeat_interleave(counts_like('L', LT([1] * 8), lens))
    assert bool((counts_like('L', LT([1] * 8), lens) < 0).any())
    same_fields(out, l, 'negative counts in padding')


# ------------------------------------------------------------------ backward
def backward(kind, x, counts, lens, w_cat, pad=0.0):
    """(gradient in cat form on the CPU, the result) of (z.repeat_interleave(r).data * w).sum(), the cotangent given in
    cat form; padding rows of an L / R cotangent hold `pad`."""
    z, r = build(kind, x, lens), counts_like(kind, counts, lens)
    leaf = z.data.clone().requires_grad_(True)
    out = rewrap(z, leaf).repeat_interleave(r)
    w = build(kind, w_cat, repeat_cat(x, counts, lens)[1], fill=pad).data
    assert w.shape == out.data.shape
    out.data.backward(w)
    return leaf.grad, rewrap(z, leaf.grad).cat().data.cpu()


@pytest.mark.parametrize('dtype', [BF16, F16, F32, F64], ids=['bf16', 'f16', 'f32', 'f64'])
def test_gradient_is_the_yardsticks_bit_for_bit(dtype):
    """Integer cotangents in [-8, 8]: a run of c copies sums to at most 8 c in magnitude, an integer, exact in a dtype
    with p significand bits while 8 c <= 2^p — checked here — so the fp32 fold and the CPU's fp64 one agree bit for bit."""
    p = {BF16: 8, F16: 11, F32: 24, F64: 53}[dtype]
    longest = 32 if dtype == BF16 else 128
    assert longest <= 2 ** 7 and 8 * longest <= 2 ** p
    lens = LT(WAVE_LENS)
    for hidden in ((), (9,), (8,)):
        x = torch.randn((int(lens.sum()),) + hidden, generator=torch.Generator().manual_seed(18)).to(dtype)
        counts = draw_counts(lens, 19, big=(longest, longest - 1))
        n_out = int(counts.sum())
        w = torch.randint(-8, 9, (n_out,) + hidden, generator=torch.Generator().manual_seed(20)).to(dtype)
        want = repeat_grad_cat(counts, w, lens, x).to(dtype)
        for kind in 'CLPR':
            with dispatch_trace() as tr:
                grad, got = backward(kind, x, counts, lens, w)
            form = 'rows' if x[0].numel() * x.element_size() > 16 else 'lanes'
            assert tr.matching(f'seg_repeat_sum_kernel form={form} table=1'), tr.records
            assert len(tr.matching('seg_repeat_plan_kernel')) == 1, 'the backward plans nothing again'
            assert grad.dtype == dtype and same_bits(got, want), (kind, hidden)
        # an int count: the same sums from the closed form
        z = build('P', x, lens)
        leaf = z.data.clone().requires_grad_(True)
        out = rewrap(z, leaf).repeat_interleave(3)
        w3 = torch.randint(-8, 9, out.data.shape, generator=torch.Generator().manual_seed(21)).to(dtype).to(DEV)
        with dispatch_trace() as tr:
            out.data.backward(w3)
        assert tr.matching('seg_repeat_sum_kernel table=0'), tr.records
        w3_cat = rewrap(out, w3).cat().data.cpu()
        want3 = repeat_grad_cat(torch.full((int(lens.sum()),), 3), w3_cat, lens, x).to(dtype)
        assert same_bits(rewrap(z, leaf.grad).cat().data, want3), hidden


def test_zero_count_tokens_and_padding_get_exact_zeros():
    lens = LT(WAVE_LENS)
    x = torch.randn(int(lens.sum()), 5, generator=torch.Generator().manual_seed(22))
    counts = draw_counts(lens, 23, big=(70,))
    w = torch.randn(int(counts.sum()), 5, generator=torch.Generator().manual_seed(24))
    w[::3, 0], w[1::3, 1] = float('nan'), float('inf')
    zero = counts == 0
    for kind in 'CLPR':
        grad, got = backward(kind, x, counts, lens, w, pad=float('nan'))
        assert bool(got.isnan().any()), 'the neighbourhood does hold NaN'
        assert same_bits(got[zero], torch.zeros_like(x[zero])), f'{kind}: tokens with count 0'
        if kind in 'LR':
            live = build(kind, torch.ones(int(lens.sum()), dtype=BOOL), lens, fill=False).data
            assert same_bits(grad[~live], torch.zeros_like(grad[~live])), f'{kind}: padding rows'


def test_backward_of_the_cut_geometry():
    lens = LT(BATCHES['cut'])
    x = torch.randn(int(lens.sum()), 5, generator=torch.Generator().manual_seed(25))
    counts = draw_counts(lens, 26, big=(128,))
    w = torch.randint(-8, 9, (int(counts.sum()), 5), generator=torch.Generator().manual_seed(27)).float()
    want = repeat_grad_cat(counts, w, lens, x).float()
    for kind in 'CP':
        with dispatch_trace() as tr:
            _, got = backward(kind, x, counts, lens, w)
        assert tr.matching('seg_repeat_sum_kernel form=rows cut=1 blocks=5'), tr.records
        assert same_bits(got, want), kind


def half_ulp(t):
    """Half the distance from |t| (fp32) to the next fp32 number, in fp64."""
    a = t.abs()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))).to(F64) - a.to(F64)) / 2


def test_random_cotangents_within_the_fold_bound(capsys):
    """fp32 cotangents against an fp64 evaluation.  The kernel adds the c rows of a run one after the other in fp32:
    c - 1 roundings, each at most 2^-24 relative to a partial sum that is at most sum |g|, the last of them at most half
    an ulp of the fp32 result.  The bound per (token, column) is (c - 1) * 2^-24 * sum |g| plus half an ulp of the
    result: derived from the fold, not tuned.  For a C the stock spelling of the backward, segment_sum(g, counts), is
    compared DIRECTLY within the same bound (its fold order may differ)."""
    u = 2.0 ** -24
    lens = LT(WAVE_LENS)
    x = torch.randn(int(lens.sum()), 7, generator=torch.Generator().manual_seed(28))
    counts = draw_counts(lens, 29, big=(128, 70))
    w = torch.randn(int(counts.sum()), 7, generator=torch.Generator().manual_seed(30))
    ref = repeat_grad_cat(counts, w, lens, x)
    mass = repeat_grad_cat(counts, w.abs(), lens, x)
    fold = (counts - 1).clamp_min(0).to(F64)[:, None] * u * mass
    with capsys.disabled():
        for kind in 'CLPR':
            _, got = backward(kind, x, counts, lens, w)
            assert got.dtype == F32
            bound = fold + half_ulp(got)
            err = (got.to(F64) - ref).abs()
            worst = float((err / bound).max())
            print(f'repeat report: {kind} f32 H=7 runs<=128 max err {float(err.max()):.3e} max err/bound {worst:.4f}')
            assert bool((err <= bound).all()), (kind, worst)
        stock = ta.segment_sum(w.to(DEV), counts.to(DEV)).cpu()
        _, got = backward('C', x, counts, lens, w)
        bound = fold + half_ulp(got)
        own = (stock.to(F64) - ref).abs()
        print(f'repeat report: segment_sum(g, counts) against fp64 max err {float(own.max()):.3e} max err/bound '
              f'{float((own / bound).max()):.4f}')
        err = (got.to(F64) - stock.to(F64)).abs()
        worst = float((err / bound).max())
        print(f'repeat report: C grad against segment_sum(g, counts) max diff {float(err.max()):.3e} max diff/bound {worst:.4f}')
        assert bool((err <= bound).all()), worst


def test_a_new_sequence_beyond_int32_is_refused_before_any_allocation():
    """Two counts of 2^31 - 1 in one sequence are valid each and add up to a sequence nobody can hold: refused after the
    read-back, nothing allocated (the result would be 2^32 rows).  An int count with lengths the host never saw: an
    L / R / P result reads them back as its cast would and refuses then; a C result never synchronises and cannot tell —
    the documented exception."""
    top = 2 ** 31 - 1
    lens = LT([3, 0, 2])
    x = torch.randn(5, 2)
    counts = LT([1, 0, 2, top, top])
    before = torch.cuda.memory_allocated()
    for kind in 'CLPR':
        z, r = build(kind, x, lens), counts_like(kind, counts, lens)
        with pytest.raises(ta.RuaError, match='the most is 2\\^31 - 1'):
            z.repeat_interleave(r)
        with pytest.raises(ta.RuaError, match='the most is 2\\^31 - 1'):
            z.repeat_interleave(2 ** 30)                                      # host lengths: 3 * 2^30
    for kind in 'LPR':
        z = cast(kind, ta.C(x.to(DEV), lens.to(DEV)))                       # device-only lengths
        if kind == 'P':                                                       # (drop the host copy the cast left)
            z = ta.P(z.data, z.batch_sizes.clone(), z.sorted_indices, z.unsorted_indices)
        else:
            z = type(z)(z.data, z.token_sizes.clone())
        with pytest.raises(ta.RuaError, match='the most is 2\\^31 - 1'):
            z.repeat_interleave(2 ** 30)
    del z, r
    assert torch.cuda.memory_allocated() - before < 1 << 20


def test_gradcheck_and_double_backward():
    lens = LT([3, 0, 5])
    counts = LT([2, 0, 3, 1, 0, 0, 2, 1])
    x = torch.randn(8, 2, dtype=F64, generator=torch.Generator().manual_seed(31))
    for kind in 'CLPR':
        z, r = build(kind, x, lens), counts_like(kind, counts, lens)
        leaf = z.data.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda d: rewrap(z, d).repeat_interleave(r).data, (leaf,), nondet_tol=0.0)
        assert torch.autograd.gradgradcheck(lambda d: rewrap(z, d).repeat_interleave(r).data, (leaf,), nondet_tol=0.0)
        assert torch.autograd.gradcheck(lambda d: rewrap(z, d).repeat_interleave(2).data, (leaf,), nondet_tol=0.0)
        # create_graph: the gradient is the run sum of the cotangent, and ITS backward repeats again
        out = rewrap(z, leaf).repeat_interleave(r)
        cot = torch.randn(out.data.shape, dtype=F64, device=DEV).requires_grad_(True)
        g, = torch.autograd.grad(out.data, leaf, cot, create_graph=True)
        assert g.requires_grad and g.shape == leaf.shape
        v = torch.randn(leaf.shape, dtype=F64, device=DEV)
        gg, = torch.autograd.grad(g, cot, v)
        assert same_bits(gg, rewrap(z, v).repeat_interleave(r).data), kind


def test_backward_is_reproducible_and_saves_no_payload():
    lens = LT(WAVE_LENS)
    x = torch.randn(int(lens.sum()), 33, generator=torch.Generator().manual_seed(32)).to(BF16)
    counts = draw_counts(lens, 33, big=(70, 300))
    w = torch.randn(int(counts.sum()), 33, generator=torch.Generator().manual_seed(34)).to(BF16)
    for kind in 'CP':
        a, _ = backward(kind, x, counts, lens, w)
        b, _ = backward(kind, x, counts, lens, w)
        assert same_bits(a, b), kind
    z = build('C', x, lens)
    leaf = z.data.clone().requires_grad_(True)
    out = rewrap(z, leaf).repeat_interleave(counts.to(DEV))
    saved = out.data.grad_fn.saved_tensors
    assert len(saved) == 2 and all(t.dtype == I64 and t.numel() == leaf.shape[0] for t in saved)
    assert rewrap(z, leaf).repeat_interleave(2).data.grad_fn.saved_tensors == ()


def test_integer_and_bool_payloads_carry_no_graph():
    lens = LT(WAVE_LENS)
    counts = draw_counts(lens, 35)
    for dtype in (I64, BOOL):
        x = draw((int(lens.sum()),), dtype, 36)
        with torch.enable_grad():
            out = build('P', x, lens).repeat_interleave(counts_like('P', counts, lens))
        assert not out.data.requires_grad and out.data.grad_fn is None and out.data.dtype == dtype
        assert same_bits(out.cat().data, repeat_cat(x, counts, lens)[0])
