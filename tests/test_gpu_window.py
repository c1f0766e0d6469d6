"""Per-sequence sliding-window pooling on the GPU: every container against the float64 yardstick of
tests/window_util.py (max as bits, sum / mean within the derived bounds, the spread against the yardstick's spread), the
commutation identities field by field, every kernel form and the cut with the dispatch trace, NaN / tie / signed-zero
isolation, autograd of every order, the saved tensors, the read-backs and the degenerate shapes.  Every comparison
prints its worst error over its bound."""
import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from join_util import bits, same_bits
from torchrua_amd import _meta
from window_util import BF16, F16, F32, F64, I64, KS, MODES, draw, n_out, out_lens, pool64, ratio_nan, spread64

pytestmark = pytest.mark.gpu

WAVE_LENS = [63, 64, 65, 129]
_cache = {}


def LT(values):
    return torch.tensor(list(values), dtype=torch.long)


def short_lens(K):
    """0, 1, K - 1, K, K + 1 and the wave borders of the lanes form, shuffled so that a PackedSequence's sort matters."""
    lens = [0, 1, max(K - 1, 0), K, K + 1] + WAVE_LENS
    order = torch.randperm(len(lens), generator=torch.Generator().manual_seed(K)).tolist()
    return LT(lens[i] for i in order)


def build(kind, x, lens, device_lens=False):
    c = ta.C(x.to(DEV), lens.to(DEV)) if device_lens else ta.with_host_sizes(x.to(DEV), lens)
    return cast(c, kind)


def cast(c, kind):
    return {'C': lambda: c, 'L': c.left, 'R': c.right, 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def same_fields(a, b, what):
    assert type(a) is type(b), what
    assert same_bits(a.data, b.data), f'{what}: data {tuple(a.data.shape)} vs {tuple(b.data.shape)}'
    if isinstance(a, ta.P):
        assert torch.equal(a.batch_sizes.cpu(), b.batch_sizes.cpu()), what
        assert torch.equal(a.sorted_indices, b.sorted_indices) and torch.equal(a.unsorted_indices, b.unsorted_indices), what
    else:
        assert a.token_sizes.dtype == b.token_sizes.dtype == I64 and torch.equal(a.token_sizes, b.token_sizes), what


def yardstick(key, x, lens, K, S, mode, ceil_mode):
    """pool64, computed once per case and shared (never modified)."""
    full = (key, K, S, mode, ceil_mode)
    if full not in _cache:
        _cache[full] = pool64(x, lens, K, S, mode, ceil_mode)
    return _cache[full]


def check_forward(out, p, what):
    got = out.cat()
    assert got.token_sizes.cpu().tolist() == p.lens.tolist(), f'{what}: lengths'
    assert got.data.dtype == p.dtype and tuple(got.data.shape) == tuple(p.want.shape), what
    if p.mode == 'max':
        assert same_bits(got.data, p.bits), f'{what}: max is not bit-exact'
    elif p.dtype == I64:
        assert torch.equal(got.data.cpu(), p.want), f'{what}: int64 {p.mode}'
    else:
        r = ratio_nan(got.data, p.want, p.bound)
        print(f'{what}: worst error / bound = {r:.3f}')
        assert r <= 1.0, f'{what}: {r}'
    if isinstance(out, (ta.L, ta.R)):
        t = int(p.lens.max()) if p.lens.numel() else 0
        assert out.data.shape[1] == t, f'{what}: T is {out.data.shape[1]}, the longest new sequence {t}'
        live = torch.arange(t)[None] < p.lens[:, None]
        if isinstance(out, ta.R):
            live = live.flip(1)
        assert not bool(bits(out.data.cpu()[~live]).any()), f'{what}: padding is not zero'
    return got


def check_all(key, x, lens, K, S, kinds='CLPR', modes=MODES, ceils=(False, True), device_lens=(False, True), grad=True):
    """Forward against the yardstick, both commutation identities, and the spread (through autograd) against the
    yardstick's spread for a random cotangent — bit-identical across the layouts."""
    c = ta.with_host_sizes(x.to(DEV), lens)
    for mode in modes:
        if x.dtype == I64 and mode == 'mean':
            continue
        for ceil_mode in ceils:
            p = yardstick(key, x, lens, K, S, mode, ceil_mode)
            ref = c.window_pool(K, S, mode, ceil_mode)
            cot = draw(p.want.shape, p.dtype, 7)
            grad_c = None
            if grad and x.is_floating_point():
                leaf = c.data.detach().clone().requires_grad_()
                ta.C(leaf, c.token_sizes).window_pool(K, S, mode, ceil_mode).data.backward(cot.to(DEV))
                grad_c = leaf.grad
                want, bound = spread64(p, cot)
                r = ratio_nan(grad_c, want, bound)
                print(f'{key} K={K} S={S} {mode} ceil={ceil_mode}: spread worst error / bound = {r:.3f}')
                assert r <= 1.0, (key, K, S, mode, ceil_mode, r)
            for kind in kinds:
                for dl in device_lens:
                    what = f'{key} K={K} S={S} {mode} ceil={ceil_mode} {kind} device_lens={dl}'
                    z = build(kind, x, lens, dl)
                    out = z.window_pool(K, S, mode, ceil_mode)
                    assert type(out) is type(z), what
                    got = check_forward(out, p, what)
                    same_fields(out, cast(ref, kind), f'{what}: X(pool(cat))')
                    same_fields(got, ref, f'{what}: cat(pool)')
                    if grad_c is not None and not dl:
                        leaf = z.data.detach().clone().requires_grad_()
                        res = rewrap(z, leaf).window_pool(K, S, mode, ceil_mode)
                        res.data.backward(cast(ta.C(cot.to(DEV), ref.token_sizes), kind).data)
                        assert same_bits(leaf.grad, cast(ta.C(grad_c, c.token_sizes), kind).data), f'{what}: spread bits'


# ------------------------------------------------------------------ the shared parameters, lanes form
@pytest.mark.parametrize('K, S', KS)
def test_values_every_kind_lanes(K, S):
    lens = short_lens(K)
    x = draw((int(lens.sum()), 4), F32, K * 131 + S % 97)
    with dispatch_trace() as t:
        check_all(('short', 4, F32), x, lens, K, S)
    pools = t.matching(f'seg_window_pool_kernel form=lanes K={K} S={S}')
    assert pools and len(pools) == len([k for k in t.kernels if k == 'seg_window_pool_kernel'])
    assert t.matching('seg_window_spread_kernel form=lanes')
    assert {r.split('mode=')[1].split()[0] for r in pools} == {'max', 'mean', 'sum'}
    assert {r.split(' kind=')[1].split()[0] for r in pools} == {'0', '1', '2', '3'}


@pytest.mark.parametrize('K, S', [(3, 2), (2, 5), (64, 64)])
def test_every_sequence_shorter_than_the_window(K, S):
    lens = LT([1, K - 1, 0, 1, K - 1])
    x = draw((int(lens.sum()), 3), F32, 5)
    check_all(('shorter', K), x, lens, K, S)
    assert ta.with_host_sizes(x.to(DEV), lens).left().max_pool(K, S).data.shape[:2] == (5, 0)
    assert ta.with_host_sizes(x.to(DEV), lens).pack().avg_pool(K, S, ceil_mode=True).data.shape[0] == 4


# ------------------------------------------------------------------ rows: every form, every dtype
@pytest.mark.parametrize('dtype, hidden, form', [
    (F32, (), 'form=lanes W=4'), (I64, (), 'form=lanes W=8'), (BF16, (1,), 'form=lanes W=2'), (F32, (4,), 'form=lanes W=16'),
    (BF16, (64,), 'form=rows chunks=1'), (F32, (72,), 'form=rows chunks=3'), (F16, (2, 8), 'form=rows chunks=1'),
    (F64, (6,), 'form=rows chunks=1'), (I64, (3,), 'form=unaligned chunks=1'), (F32, (25,), 'form=unaligned chunks=1'),
    (BF16, (9,), 'form=unaligned chunks=1'),
])
def test_row_forms(dtype, hidden, form):
    lens = LT([5, 0, 33, 1, 64, 2, 9, 40, 3])                 # nine sequences: more than one workgroup of the lanes form
    x = draw((int(lens.sum()),) + hidden, dtype, 11)
    with dispatch_trace() as t:
        for K, S in [(3, 2), (2, 5), (64, 1)]:
            check_all(('forms', dtype, hidden), x, lens, K, S, device_lens=(False,))
    assert t.matching('seg_window_pool_kernel ' + form), t.records[:4]
    assert dtype == I64 or t.matching('seg_window_spread_kernel ' + form)
    assert not [r for r in t.records if r.startswith('seg_window_') and 'lens' not in r and form.split()[0] not in r]


def test_odd_element_offset():
    """H = 5 bf16 at an odd element offset into a larger buffer: 10-byte rows on a 2-byte boundary (one vector: the lanes
    form, in 2-byte accesses), and H = 25 fp32 one element into its buffer (the unaligned rows form)."""
    lens = LT([7, 0, 40, 3, 65])
    for dtype, H, form in ((BF16, 5, 'form=lanes W=2'), (F32, 25, 'form=unaligned')):
        x = draw((int(lens.sum()), H), dtype, 3)
        buf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 != 0
        z = ta.with_host_sizes(view, lens)
        for mode in MODES:
            with dispatch_trace() as t:
                out = z.window_pool(3, 2, mode, True)
            assert t.matching('seg_window_pool_kernel ' + form), t.records
            check_forward(out, yardstick(('odd', dtype), x, lens, 3, 2, mode, True), f'odd offset {dtype} {mode}')


# ------------------------------------------------------------------ the cut
@pytest.mark.parametrize('K, S', [(3, 2), (2, 5), (3, 1)])
def test_cut_form(K, S):
    """Two sequences just past the cut rule's bound.  (3, 2): the window at 2046 straddles the block border 2048;
    (2, 5): the border falls in the gap 2047 .. 2049; (3, 1): every border is straddled twice."""
    lens = LT([8195, 9000])
    x = draw((int(lens.sum()), 8), F32, 17)
    with dispatch_trace() as t:
        check_all(('cut',), x, lens, K, S, modes=('max', 'mean'), ceils=(True,), device_lens=(False,))
    pools = [r for r in t.records if r.startswith('seg_window_pool_kernel')]
    spreads = [r for r in t.records if r.startswith('seg_window_spread_kernel')]
    assert pools and all('form=rows' in r and 'cut=1' in r and 'blocks=5' in r for r in pools), pools[:2]
    assert spreads and all('form=rows' in r and 'cut=1' in r and 'blocks=5' in r for r in spreads), spreads[:2]
    # the same sequences among many are not cut, and give the same bits
    more = torch.cat([lens, torch.full((1100,), 1, dtype=torch.long)])
    xm = torch.cat([x, draw((1100, 8), F32, 18)])
    with dispatch_trace() as t:
        out = ta.with_host_sizes(xm.to(DEV), more).window_pool(K, S, 'mean', True)
    assert t.matching('seg_window_pool_kernel form=rows cut=0')
    p = yardstick(('cut',), x, lens, K, S, 'mean', True)
    n = int(p.lens.sum())
    assert same_bits(out.data[:n], ta.with_host_sizes(x.to(DEV), lens).window_pool(K, S, 'mean', True).data)


# ------------------------------------------------------------------ identities
def test_identities():
    lens = LT([5, 0, 12, 1, 7])
    x = draw((int(lens.sum()), 6), F32, 23)
    c = ta.with_host_sizes(x.to(DEV), lens)
    for kind in 'CLPR':
        z = cast(c, kind)
        for mode in MODES:
            same_fields(z.window_pool(1, 1, mode).cat(), c, f'(1, 1) {mode} {kind}')
        assert same_bits(z.max_pool(3, 2, True).data, z.window_pool(3, 2, 'max', True).data)
        assert same_bits(z.avg_pool(3).data, z.window_pool(3, None, 'mean', False).data)
        for s in (2, 3, 7):
            want = torch.cat([seq[::s] for seq in torch.split(x, lens.tolist())])
            assert same_bits(z.window_pool(1, s, 'max', True).cat().data, want), f'z[::{s}] {kind}'
    t, sizes = ta.segment_window_pool(c.data, c.token_sizes, 3, 2, 'sum', True)
    assert same_bits(t, c.window_pool(3, 2, 'sum', True).data) and sizes.cpu().tolist() == out_lens(lens, 3, 2, True).tolist()
    # mode='sum' with (K, K) in ceil mode is segment_sum over the windows' sizes (integer-valued data: both sums exact)
    xi = torch.randint(-50, 50, x.shape, generator=torch.Generator().manual_seed(1)).float()
    sizes = LT(min(4, n - a) for n in lens.tolist() for a in range(0, n, 4))
    want = ta.segment_sum(xi.to(DEV), sizes.to(DEV))
    assert same_bits(ta.with_host_sizes(xi.to(DEV), lens).window_pool(4, 4, 'sum', True).data, want)


def test_int64():
    lens = LT([5, 0, 12, 1, 7, 64])
    x = draw((int(lens.sum()), 2), I64, 29)
    assert (x.double().abs().sum() > 2.0 ** 64)                # the sums wrap
    for K, S in [(3, 2), (64, 1), (2, 5)]:
        check_all(('i64',), x, lens, K, S, modes=('max', 'sum'), device_lens=(False,))
    z = ta.with_host_sizes(x.to(DEV).requires_grad_(False), lens)
    assert z.window_pool(2, 2, 'sum').data.grad_fn is None


# ------------------------------------------------------------------ isolation
def test_nan_ties_and_signed_zeros():
    lens = LT([10, 7, 0, 33, 4])
    g = torch.Generator().manual_seed(31)
    values = torch.tensor([-1.0, 0.0, -0.0, 1.0, 1.0, float('nan')])
    for dtype in (F32, BF16):
        x = values[torch.randint(0, 6, (int(lens.sum()), 3), generator=g)].to(dtype)
        for K, S in [(3, 1), (3, 2), (2, 5), (64, 64)]:
            check_all(('ties', dtype), x, lens, K, S, device_lens=(False,))
    # one NaN reaches exactly the windows that hold it
    x = draw((int(lens.sum()), 3), F32, 37)
    x[13, 1] = float('nan')                                     # token 3 of the second sequence
    for mode in MODES:
        out = ta.with_host_sizes(x.to(DEV), lens).window_pool(3, 2, mode, True).data.cpu()
        nan = torch.isnan(out).nonzero().tolist()
        first = n_out(10, 3, 2, True)                           # the pooled rows of the first sequence come before
        want = [[first + u, 1] for u in range(n_out(7, 3, 2, True)) if u * 2 <= 3 < u * 2 + 3]
        assert want and nan == want, (mode, nan, want)


def test_nan_padding_changes_nothing():
    lens = LT([5, 0, 12, 1])
    x = draw((int(lens.sum()), 5), F32, 41)
    c = ta.with_host_sizes(x.to(DEV), lens)
    for kind in 'LR':
        z = cast(c, kind)
        live = torch.arange(12, device=DEV)[None] < lens.to(DEV)[:, None]
        if kind == 'R':
            live = live.flip(1)
        poisoned = torch.where(live[..., None], z.data, torch.full_like(z.data, float('nan')))
        for mode in MODES:
            for K, S in [(3, 2), (2, 5)]:
                leaf = poisoned.clone().requires_grad_()
                out = rewrap(z, leaf).window_pool(K, S, mode, True)
                assert same_bits(out.data, z.window_pool(K, S, mode, True).data), (kind, mode)
                out.data.sum().backward()
                assert not bool(torch.isnan(leaf.grad).any()) and not bool(leaf.grad[~live].any()), (kind, mode)


def test_gaps_and_tails_get_exact_zeros_over_nan_payload():
    lens = LT([12, 9])
    x = torch.full((21, 2), float('nan'))
    leaf = x.to(DEV).requires_grad_()
    ta.with_host_sizes(leaf, lens).window_pool(2, 5, 'max').data.backward(torch.ones(5, 2, device=DEV))
    g = leaf.grad.cpu()
    touched = [0, 5, 10, 12, 17]                                # a NaN window goes to its first NaN: the first token
    assert g[touched].eq(1).all() and g.sum() == 10 and not torch.isnan(g).any()


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize('mode', MODES)
def test_gradient_matches_torch(mode):
    lens = LT([9, 4, 17, 5])
    K, S = 4, 3
    x = draw((int(lens.sum()), 3), F64, 43)
    for ceil_mode in (False, True):
        ref = x.clone().requires_grad_()
        outs = []
        for seq in torch.split(ref, lens.tolist()):
            if mode == 'max':
                outs.append(F.max_pool1d(seq.T[None], K, S, ceil_mode=ceil_mode)[0].T)
            else:
                y = F.avg_pool1d(seq.T[None], K, S, ceil_mode=ceil_mode, count_include_pad=False)[0].T
                if mode == 'sum':
                    cnt = torch.tensor([min(u * S + K, seq.shape[0]) - u * S for u in range(y.shape[0])], dtype=F64)
                    y = y * cnt[:, None]
                outs.append(y)
        want = torch.cat(outs)
        cot = draw(want.shape, F64, 47)
        want.backward(cot)
        for kind in 'CLPR':
            z = build(kind, x, lens)
            leaf = z.data.detach().clone().requires_grad_()
            out = rewrap(z, leaf).window_pool(K, S, mode, ceil_mode)
            got = out.cat().data
            got.backward(cot.to(DEV))
            grad = rewrap(z, leaf.grad).cat().data.cpu()
            tol = 8 * 2.0 ** -53 * float(x.abs().max() + cot.abs().max()) * K
            print(f'{mode} ceil={ceil_mode} {kind}: forward {float((got.detach().cpu() - want.detach()).abs().max()):.2e}, '
                  f'gradient {float((grad - ref.grad).abs().max()):.2e}, tolerance {tol:.2e}')
            assert float((got.detach().cpu() - want.detach()).abs().max()) <= tol
            assert float((grad - ref.grad).abs().max()) <= tol


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('mode', MODES)
def test_gradcheck_every_order(mode, kind):
    lens = LT([5, 2, 4])
    x = draw((11, 2), F64, 53)
    z = build(kind, x, lens)
    fn = lambda data: rewrap(z, data).window_pool(3, 2, mode, True).data
    leaf = z.data.detach().clone().requires_grad_()
    assert torch.autograd.gradcheck(fn, (leaf,), eps=1e-6, atol=1e-7, nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(fn, (leaf,), eps=1e-6, atol=1e-7, nondet_tol=0.0)


def test_what_autograd_saves():
    lens = LT([40, 3, 65])
    x = draw((int(lens.sum()), 16), F32, 59)
    for kind in 'CLPR':
        z = build(kind, x, lens)
        for mode in MODES:
            saved = []
            leaf = z.data.detach().clone().requires_grad_()
            with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
                out = rewrap(z, leaf).window_pool(3, 2, mode, True)
            big = [t for t in saved if t.numel() >= min(out.data.numel(), leaf.numel())]
            if mode == 'max':
                assert [(t.dtype, t.numel()) for t in big] == [(torch.uint8, out.data.numel())], (kind, [t.shape for t in saved])
            else:
                assert not big, (kind, mode, [(t.dtype, tuple(t.shape)) for t in saved])
            assert not [t for t in saved if t.is_floating_point()], (kind, mode)


# ------------------------------------------------------------------ synchronisation
def test_read_backs(monkeypatch):
    lens = LT(WAVE_LENS + [0, 3])
    x = draw((int(lens.sum()), 5), F32, 61)
    hosted = {kind: build(kind, x, lens) for kind in 'CLPR'}
    device = {kind: build(kind, x, lens, device_lens=True) for kind in 'CLPR'}
    fresh = {}
    for kind, z in device.items():
        if kind == 'P':
            fresh[kind] = ta.P(z.data, z.batch_sizes.clone(), z.sorted_indices.clone(), z.unsorted_indices.clone())
        else:
            fresh[kind] = z._replace(token_sizes=z.token_sizes.clone())
    torch.cuda.synchronize()
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    for kind in 'CLPR':
        out = hosted[kind].window_pool(3, 2, 'mean', True)
        out.pack(), out.left(), out.right(), out.cat()
        assert calls == [], f'{kind}: host lengths, yet {calls} was read back'
    for kind in 'CLR':
        out = fresh[kind].window_pool(3, 2, 'max')
        assert calls == [(2, len(lens))], f'{kind}: {calls}'
        out.pack(), out.left(), out.right(), out.cat()
        fresh[kind].window_pool(2, 2, 'sum').left()
        assert calls == [(2, len(lens))], f'{kind}: the casts or a second call read back again: {calls}'
        calls.clear()
    out = fresh['P'].window_pool(3, 2, 'max')
    assert len(calls) <= 1, calls                                # (a P's lengths may be known from its batch_sizes)
    out.pack(), out.left()
    assert len(calls) <= 1, calls


# ------------------------------------------------------------------ degenerate
def test_degenerate():
    for mode in MODES:
        out = ta.C(torch.zeros(0, 4, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)).window_pool(2, 1, mode)
        assert tuple(out.data.shape) == (0, 4) and out.token_sizes.numel() == 0
        zero = LT([0, 0, 0])
        for kind in 'CLPR':
            z = build(kind, torch.zeros(0, 4), zero)
            out = z.window_pool(3, 2, mode, True)
            assert type(out) is type(z) and out.data.numel() == 0 and out.cat().token_sizes.tolist() == [0, 0, 0]
        lens = LT([3, 5])
        for cls, shape in ((ta.C, (8, 0)), (ta.L, (2, 5, 0))):
            out = cls(torch.zeros(shape, device=DEV), lens.to(DEV)).window_pool(2, 2, mode)
            assert out.data.numel() == 0 and out.token_sizes.tolist() == [1, 2]
        x = draw((1, 3), F32, 67)
        for kind in 'CLPR':
            z = build(kind, x, LT([1]))
            assert z.window_pool(64, 64, mode).cat().data.shape[0] == 0
            assert same_bits(z.window_pool(64, 64, mode, True).cat().data, x)
            leaf = z.data.detach().clone().requires_grad_()
            rewrap(z, leaf).window_pool(64, 64, mode).data.sum().backward()          # nothing was pooled: zeros
            assert not bool(leaf.grad.any())
