"""Per-sequence causal depthwise convolution on the GPU: forward and the three gradients in all four containers against
stock torch in float64 (tests/conv_util.py: the yardstick and the derived bounds), the cut geometry and its halo, the
bit-for-bit identities (casts commute, reverse is the mirrored forward, the one-tap identity, in place == out of place),
isolation (NaN, a non-finite weight, NaN padding), gradcheck / gradgradcheck, reproducible weight gradients, the launch
count of the backward, degenerate shapes.

Every comparison prints its worst error over its bound; the last test prints the `causal_conv report:` lines
(profiles/causal_conv_report.txt keeps a run's)."""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from conv_util import (BF16, F16, F32, F64, batch_lengths, conv64, conv_bound, draw, ratio, weight_grad_bounds,
                       weight_grads64)
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

REPORT = {}
NAME = {F32: 'fp32', F64: 'fp64', BF16: 'bf16', F16: 'fp16'}


# ------------------------------------------------------------------ helpers
def LT(*values):
    return torch.tensor(values, dtype=torch.long)


def build(kind, x, lens_host, host_sizes=True):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def lay_of(z):
    return M.lay_pack(z) if isinstance(z, ta.P) else describe(z)


def hidden_of(z):
    return tuple(z.data.shape[1:]) if isinstance(z, (ta.C, ta.P)) else tuple(z.data.shape[2:])


def form_of(hidden, dtype):
    nbytes = int(np.prod(hidden, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return 'lanes' if nbytes <= 16 else ('rows' if nbytes % 16 == 0 else 'rows-unaligned')


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def held(got, want64, bound, what, key):
    r = ratio(got, want64, bound)
    REPORT[key] = max(REPORT.get(key, 0.0), r)
    print(f'{what}: worst error / bound {r:.3f}')
    assert r <= 1.0, f'{what}: {r:.3f} x the bound'


def run(kind, x, w, b, lens, reverse, cot=None, host_sizes=True):
    """y in cat form; with a cotangent (cat form): (y, grad_input in cat form, grad_weight, grad_bias)."""
    z = build(kind, x, lens, host_sizes)
    if cot is None:
        out = z.causal_conv(w, b, reverse=reverse)
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == x.dtype
        return out.cat().data
    leaf = z.data.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    bl = None if b is None else b.detach().clone().requires_grad_(True)
    out = rewrap(z, leaf).causal_conv(wl, bl, reverse=reverse)
    out.data.backward(build(kind, cot, lens, host_sizes).data)              # the cotangent in the same layout
    assert wl.grad.shape == w.shape and wl.grad.dtype == w.dtype
    return out.cat().data.detach(), rewrap(z, leaf.grad).cat().data, wl.grad, None if bl is None else bl.grad


class Case:
    """One batch (cat form, CPU and GPU) with its float64 references, computed once per (reverse, bias) and shared."""

    def __init__(self, lens, hidden, dtype, K, seed):
        self.lens, self.hidden, self.dtype, self.K = lens, tuple(hidden), dtype, K
        n = int(lens.sum())
        self.x, self.cot = draw((n,) + self.hidden, dtype, seed), draw((n,) + self.hidden, dtype, seed + 1)
        self.w, self.b = draw((K,) + self.hidden, dtype, seed + 2), draw(self.hidden, dtype, seed + 3)
        self.dev = {k: getattr(self, k).to(DEV) for k in ('x', 'cot', 'w', 'b')}
        self._want = {}

    def want(self, reverse, bias):
        key = (reverse, bias)
        if key not in self._want:
            b = self.b if bias else None
            y = conv64(self.x, self.w, b, self.lens, reverse)
            gx = conv64(self.cot, self.w, None, self.lens, not reverse)
            gw, gb, _ = weight_grads64(self.cot, self.x, self.K, self.lens, reverse)
            bw, bb = weight_grad_bounds(self.cot, self.x, self.K, self.lens, reverse, gw, gb, self.dtype)
            self._want[key] = dict(y=y, by=conv_bound(self.x, self.w, b, self.lens, reverse, y, self.dtype), gx=gx,
                                   bgx=conv_bound(self.cot, self.w, None, self.lens, not reverse, gx, self.dtype),
                                   gw=gw, bgw=bw, gb=gb, bgb=bb)
        return self._want[key]

    def check(self, kind, reverse, bias, what, host_sizes=True):
        d, wnt = self.dev, self.want(reverse, bias)
        y, gx, gw, gb = run(kind, d['x'], d['w'], d['b'] if bias else None, self.lens, reverse, d['cot'], host_sizes)
        key = f'{NAME[self.dtype]} {form_of(self.hidden, self.dtype)}'
        what = f'{what} {kind} K={self.K} rev={int(reverse)} bias={int(bias)}'
        held(y, wnt['y'], wnt['by'], what + ' fwd', key + ' forward')
        held(gx, wnt['gx'], wnt['bgx'], what + ' grad_input', key + ' grad_input')
        held(gw, wnt['gw'], wnt['bgw'], what + ' grad_weight', key + ' grad_weight')
        if bias:
            held(gb, wnt['gb'], wnt['bgb'], what + ' grad_bias', key + ' grad_bias')
        return y, gx, gw, gb


# ------------------------------------------------------------------ forward and the gradients against float64
# (hidden, dtype, why)
WIDTHS = [
    ((), F32, '1-D payload'),
    ((), BF16, '1-D payload, 2-byte rows'),
    ((3,), F32, '12-byte lanes form'),
    ((3,), F16, '6-byte lanes form'),
    ((2,), F64, '16-byte lanes form in fp64'),
    ((8,), BF16, 'exactly 16 bytes'),
    ((33,), F32, 'unaligned, two chunks, ragged tail'),
    ((33,), BF16, 'unaligned, one chunk'),
    ((64,), F32, 'aligned, two chunks'),
    ((64,), BF16, 'aligned, one chunk'),
    ((64,), F16, 'aligned, one chunk'),
    ((40,), F64, 'aligned, three chunks, the last one partial'),
    ((2, 5), F32, 'multi-dim hidden'),
    ((2, 5), BF16, 'multi-dim hidden'),
]


@pytest.mark.parametrize('hidden,dtype,why', WIDTHS, ids=[f'{NAME[d]}-{"x".join(map(str, h)) or "1d"}' for h, d, _ in WIDTHS])
def test_against_float64(hidden, dtype, why):
    for K in (1, 2, 3, 4, 8):
        case = Case(batch_lengths(K, seed=K), hidden, dtype, K, seed=100 * K + len(hidden))
        for i, kind in enumerate('CLPR'):
            for reverse in (False, True):
                for bias in ((False, True) if K == 4 else ((K + i + reverse) % 2 == 0,)):
                    # device-only lengths for P and R, a host mirror for C and L
                    case.check(kind, reverse, bias, why, host_sizes=kind in 'CL')


# ------------------------------------------------------------------ the cut geometry
CUT_LENS = LT(10240, 9000)


def split_lengths(lens, piece=2048):
    out, first, last = [], [], []
    for n in lens.tolist():
        parts = [piece] * (n // piece) + ([n % piece] if n % piece else [])
        out += parts
        first += [True] + [False] * (len(parts) - 1)
        last += [False] * (len(parts) - 1) + [True]
    return LT(*out), first, last


@pytest.mark.parametrize('K', (4, 8))
def test_cut_blocks_and_their_halo(K):
    """Few but long sequences spread over workgroups per block of 2 048 tokens.  The same rows split into sequences of at
    most 2 048 tokens agree bit for bit on every token at distance >= K - 1 from a split point: the rows in front of a
    block are read across the block boundary, and nowhere else."""
    case = Case(CUT_LENS, (40,), F32, K, seed=7)
    d = case.dev
    pieces, first, last = split_lengths(CUT_LENS)
    for reverse in (False, True):
        with dispatch_trace() as tr:
            y = run('C', d['x'], d['w'], d['b'], CUT_LENS, reverse)
        assert tr.matching(f'seg_conv_rows_kernel cut=1 blocks=5 chunks=2 K={K} rev={int(reverse)}'), tr.records
        ysplit = run('C', d['x'], d['w'], d['b'], pieces, reverse)
        keep = torch.ones(int(CUT_LENS.sum()), dtype=torch.bool)
        off = 0
        for n, is_first, is_last in zip(pieces.tolist(), first, last):
            if reverse and not is_last:
                keep[off + n - (K - 1):off + n] = False
            if not reverse and not is_first:
                keep[off:off + K - 1] = False
            off += n
        assert int((~keep).sum()) == (K - 1) * (len(first) - 2)
        keep = keep.to(DEV)
        assert same_bits(y[keep], ysplit[keep]), f'K={K} rev={reverse}: a block boundary shows'
        assert not same_bits(y[~keep], ysplit[~keep])
        for kind in 'LPR':                                     # and the other layouts give the bits of C
            with dispatch_trace() as tr:
                yk = run(kind, d['x'], d['w'], d['b'], CUT_LENS, reverse)
            assert tr.matching('seg_conv_rows_kernel cut=1'), tr.records
            assert same_bits(yk, y), f'{kind} K={K} rev={reverse}'
    # against float64, gradients included: the backward walks (sequence, block) units too
    for kind, reverse in (('C', False), ('P', True), ('L', True), ('R', False)):
        with dispatch_trace() as tr:
            case.check(kind, reverse, True, 'cut')
        assert tr.matching('seg_conv_rows_kernel cut=1 bwd=1 parts=10'), tr.records
        assert tr.matching('seg_conv_finish_kernel parts=10'), tr.records


# ------------------------------------------------------------------ bit identities
IDENT = [((33,), F32), ((8,), BF16), ((64,), BF16), ((), F32), ((3,), F16), ((40,), F64)]
CASTS = {'C': lambda z: z.cat(), 'L': lambda z: z.left(0), 'P': lambda z: z.pack(), 'R': lambda z: z.right(0)}


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=[f'{NAME[d]}-{"x".join(map(str, h)) or "1d"}' for h, d in IDENT])
def test_bit_identities(hidden, dtype):
    K = 4
    case = Case(batch_lengths(K, seed=3), hidden, dtype, K, seed=11)
    d = case.dev
    z = {kind: build(kind, d['x'], case.lens) for kind in 'CLPR'}
    for reverse in (False, True):
        for b in (d['b'], None):
            y = {kind: z[kind].causal_conv(d['w'], b, reverse=reverse) for kind in 'CLPR'}
            # the operator commutes with the casts, over all ordered pairs of layouts
            for src in 'CLPR':
                for dst in 'CLPR':
                    if src != dst:
                        moved = CASTS[dst](y[src])
                        assert same_bits(moved.data, y[dst].data), f'{src} -> {dst} rev={reverse} bias={b is not None}'
            # reverse is the mirrored forward
            for kind in 'CLPR':
                mirrored = z[kind].rev().causal_conv(d['w'], b, reverse=not reverse).rev()
                assert same_bits(mirrored.data, y[kind].data), f'{kind} rev={reverse}: the mirror differs'
    # one tap of weight 1, no bias: the input's bits
    one = torch.ones((1,) + tuple(hidden), dtype=dtype, device=DEV)
    for kind in 'CLPR':
        for reverse in (False, True):
            assert same_bits(z[kind].causal_conv(one, reverse=reverse).cat().data, d['x']), f'{kind} identity'


@pytest.mark.parametrize('hidden,dtype', [((3,), F32), ((33,), F32), ((64,), BF16), ((), BF16)])
def test_in_place_gives_the_same_bits(hidden, dtype):
    for K, lens in ((4, batch_lengths(4, seed=5)), (8, CUT_LENS)):
        case = Case(lens, hidden, dtype, K, seed=13)
        d = case.dev
        for kind in 'CLPR':
            z = build(kind, d['x'], lens)
            lay = lay_of(z)
            for reverse in (False, True):
                want = O.launch_causal_conv(lay, z.data, d['w'], d['b'], reverse, hidden_of(z))
                buf = z.data.clone()
                got = O.launch_causal_conv(lay, buf, d['w'], d['b'], reverse, hidden_of(z), out=buf)
                assert got is buf and same_bits(buf, want), f'{kind} K={K} rev={reverse}'


# ------------------------------------------------------------------ isolation
@pytest.mark.parametrize('hidden,dtype', [((5,), F32), ((3,), F32), ((16,), BF16), ((), BF16)])
def test_nan_reaches_exactly_the_outputs_that_depend_on_it(hidden, dtype):
    K, lens = 4, LT(5, 40, 0, 7)
    case = Case(lens, hidden, dtype, K, seed=17)
    x = case.dev['x'].clone()
    flat = x.view(x.shape[0], -1)
    col = flat.shape[1] - 1
    hits = (5 + 10, 5 + 38)                                    # tokens 10 and 38 of sequence 1 (the second: near its end)
    for row in hits:
        flat[row, col] = float('nan')
    for kind in 'CLPR':
        for reverse in (False, True):
            y = run(kind, x, case.dev['w'], case.dev['b'], lens, reverse).view(x.shape[0], -1)
            want = torch.zeros_like(y, dtype=torch.bool)
            for row in hits:
                lo, hi = (max(5, row - (K - 1)), row + 1) if reverse else (row, min(45, row + K))
                want[lo:hi, col] = True
            assert torch.equal(torch.isnan(y), want), f'{kind} rev={reverse}'
            clean = run(kind, case.dev['x'], case.dev['w'], case.dev['b'], lens, reverse).view(x.shape[0], -1)
            assert same_bits(y[~want], clean[~want])


@pytest.mark.parametrize('hidden,dtype', [((5,), F32), ((3,), F32), ((16,), BF16)])
def test_infinite_first_tap_leaves_token_0_finite(hidden, dtype):
    """Taps outside the sequence are not evaluated: weight[0] = inf would give inf * 0 = NaN under zero padding."""
    K, lens = 3, LT(1, 2, 9, 40)
    case = Case(lens, hidden, dtype, K, seed=19)
    w = case.dev['w'].clone()
    w[0] = float('inf')
    starts = torch.cumsum(lens, 0) - lens
    for kind in 'CLPR':
        y = run(kind, case.dev['x'], w, case.dev['b'], lens, False)
        assert bool(torch.isfinite(y[starts.to(DEV)]).all()), kind
        assert bool(torch.isfinite(y[(starts + 1)[1:].to(DEV)]).all()), kind         # token 1 misses tap 0 too
        assert not bool(torch.isfinite(y[(starts + 2)[2:].to(DEV)]).any()), kind     # token 2 has every tap
        y = run(kind, case.dev['x'], w, case.dev['b'], lens, True)
        ends = (starts + lens - 1).to(DEV)
        assert bool(torch.isfinite(y[ends]).all()), kind


@pytest.mark.parametrize('hidden,dtype', [((5,), F32), ((3,), F32), ((16,), BF16)])
def test_padding_is_never_read_and_comes_back_as_zeros(hidden, dtype):
    K, lens = 4, LT(5, 40, 0, 7)
    case = Case(lens, hidden, dtype, K, seed=23)
    d = case.dev
    for kind in 'LR':
        z = build(kind, d['x'], lens)
        T = z.data.shape[1]
        pos = torch.arange(T)[None, :]
        live = (pos < lens[:, None]) if kind == 'L' else (pos >= T - lens[:, None])
        live = live.to(DEV)
        dirty = z.data.clone()
        dirty[~live] = float('nan')
        cot = build(kind, d['cot'], lens).data.clone()
        cot[~live] = float('nan')
        for reverse in (False, True):
            want = z.causal_conv(d['w'], d['b'], reverse=reverse).data
            leaf = dirty.clone().requires_grad_(True)
            out = rewrap(z, leaf).causal_conv(d['w'], d['b'], reverse=reverse)
            assert same_bits(out.data, want), f'{kind} rev={reverse}: the padding was read'
            assert bool((out.data[~live] == 0).all())
            out.data.backward(cot)
            assert bool((leaf.grad[~live] == 0).all()) and bool(torch.isfinite(leaf.grad).all())
            wl = d['w'].clone().requires_grad_(True)
            bl = d['b'].clone().requires_grad_(True)
            rewrap(z, dirty).causal_conv(wl, bl, reverse=reverse).data.backward(cot)
            assert bool(torch.isfinite(wl.grad).all()) and bool(torch.isfinite(bl.grad).all())


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('reverse', (False, True))
def test_gradcheck_and_gradgradcheck(kind, reverse):
    """float64, B = 3, lengths [0, 2, 5], H = 3, K = 3: first order through the fused backward, second order through
    the composed one (the convolution and its weight gradient, each the other's adjoint)."""
    lens = LT(0, 2, 5)
    x, w, b = draw((7, 3), F64, 29).to(DEV), draw((3, 3), F64, 31).to(DEV), draw((3,), F64, 37).to(DEV)
    z = build(kind, x, lens)

    def f(data, weight, bias):
        return rewrap(z, data).causal_conv(weight, bias, reverse=reverse).data

    def f_nobias(data, weight):
        return rewrap(z, data).causal_conv(weight, reverse=reverse).data

    args = tuple(t.clone().requires_grad_(True) for t in (z.data, w, b))
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(f, args, eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(f_nobias, args[:2], eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


def test_weight_gradients_are_bitwise_reproducible():
    rng = np.random.RandomState(41)
    many = torch.from_numpy(rng.randint(0, 200, 700).astype(np.int64))
    for lens, hidden, dtype in ((many, (64,), BF16), (many, (3,), F32), (CUT_LENS, (40,), F32)):
        case = Case(lens, hidden, dtype, 4, seed=43)
        d = case.dev
        for kind in 'CP':
            first = run(kind, d['x'], d['w'], d['b'], lens, False, d['cot'])
            for _ in range(2):
                again = run(kind, d['x'], d['w'], d['b'], lens, False, d['cot'])
                assert same_bits(first[2], again[2]) and same_bits(first[3], again[3]), f'{kind} {hidden} {dtype}'


def test_backward_of_the_payload_alone_is_one_launch_without_workspace(monkeypatch):
    case = Case(batch_lengths(4, seed=5), (33,), F32, 4, seed=47)
    d = case.dev
    names, spaces = [], []
    real = O._workspace

    def spy(*args, **kwargs):
        ws = real(*args, **kwargs)
        spaces.append(ws)
        return ws

    monkeypatch.setattr(O, '_workspace', spy)
    for kind in 'CLPR':
        for reverse in (False, True):
            z = build(kind, d['x'], case.lens)
            leaf = z.data.clone().requires_grad_(True)
            out = rewrap(z, leaf).causal_conv(d['w'], d['b'], reverse=reverse)
            assert len(out.data.grad_fn.saved_tensors) == 1              # the weight; no [N, H] tensor is kept
            cot = build(kind, d['cot'], case.lens).data
            del names[:], spaces[:]
            O.set_kernel_hook(lambda name, opening: names.append(name) if opening else None)
            try:
                with dispatch_trace() as tr:
                    out.data.backward(cot)
            finally:
                O.set_kernel_hook(None)
            assert names == ['causal_conv_rev_bwd' if reverse else 'causal_conv_bwd'], names
            assert len(tr.records) == 1 and tr.matching(f'seg_conv_rows_kernel bwd=0 rev={int(not reverse)}'), tr.records
            assert all(ws is None for ws in spaces), 'a workspace was allocated'
            held(rewrap(z, leaf.grad).cat().data, case.want(reverse, True)['gx'], case.want(reverse, True)['bgx'],
                 f'payload-only backward {kind} rev={int(reverse)}', 'fp32 rows-unaligned grad_input')
    # with the weight wanted the payload is saved too, and the one entry point makes the walk and the finish
    z = build('C', d['x'], case.lens)
    wl = d['w'].clone().requires_grad_(True)
    out = z.causal_conv(wl, d['b'])
    assert len(out.data.grad_fn.saved_tensors) == 2
    O.set_kernel_hook(lambda name, opening: names.append(name) if opening else None)
    del names[:], spaces[:]
    try:
        with dispatch_trace() as tr:
            out.data.backward(d['cot'])
    finally:
        O.set_kernel_hook(None)
    assert names == ['causal_conv_bwd'] and tr.kernels == ['seg_conv_rows_kernel', 'seg_conv_finish_kernel'], tr.records
    assert len(spaces) == 1 and spaces[0] is not None


# ------------------------------------------------------------------ degenerate inputs
@pytest.mark.parametrize('dtype', (F32, BF16))
def test_degenerate_inputs(dtype):
    w, b = draw((4, 6), dtype, 53).to(DEV), draw((6,), dtype, 59).to(DEV)

    def both(z, weight, bias):
        leaf = z.data.clone().requires_grad_(True)
        wl, bl = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        out = rewrap(z, leaf).causal_conv(wl, bl)
        assert type(out) is type(z) and out.data.shape == z.data.shape
        out.data.backward(torch.ones_like(out.data))
        return out.data.detach(), leaf.grad, wl.grad, bl.grad

    # B == 0
    for z in (ta.C(torch.empty(0, 6, dtype=dtype, device=DEV), LT().to(DEV)),
              ta.L(torch.empty(0, 5, 6, dtype=dtype, device=DEV), LT().to(DEV))):
        y, gx, gw, gb = both(z, w, b)
        assert y.numel() == 0 and gx.numel() == 0 and not bool(gw.any()) and not bool(gb.any())
    # every sequence empty
    empty = LT(0, 0, 0)
    for kind in 'CLPR':
        if kind == 'P':
            continue                                               # (a PackedSequence of empty sequences cannot be built)
        z = build(kind, torch.empty(0, 6, dtype=dtype, device=DEV), empty)
        y, gx, gw, gb = both(z, w, b)
        assert not bool(y.any()) and not bool(gx.any()) and not bool(gw.any()) and not bool(gb.any())
    # H == 0
    z = build('C', torch.empty(7, 0, dtype=dtype, device=DEV), LT(3, 4))
    y, gx, gw, gb = both(z, torch.empty(4, 0, dtype=dtype, device=DEV), torch.empty(0, dtype=dtype, device=DEV))
    assert y.shape == (7, 0) and gx.shape == (7, 0) and gw.shape == (4, 0) and gb.shape == (0,)
    # K larger than every length
    case = Case(LT(1, 3, 2, 0, 7), (6,), dtype, 8, seed=61)
    for kind in 'CLPR':
        for reverse in (False, True):
            case.check(kind, reverse, True, 'K > every length')
    case = Case(LT(1, 3, 2, 0, 7), (), dtype, 8, seed=67)
    for kind in 'CLPR':
        case.check(kind, False, True, 'K > every length, 1-D')


def test_segment_form_and_refusals_on_the_device():
    case = Case(batch_lengths(3, seed=9), (5,), F32, 3, seed=71)
    d = case.dev
    y = ta.segment_causal_conv(d['x'], d['w'], case.lens.to(DEV), bias=d['b'], reverse=True)
    assert same_bits(y, run('C', d['x'], d['w'], d['b'], case.lens, True))
    with pytest.raises(ta.RuaError):
        ta.segment_causal_conv(d['x'], d['w'].cpu(), case.lens.to(DEV))             # the weight on the host
    with pytest.raises(ta.RuaError):
        ta.segment_causal_conv(d['x'].long(), d['w'].long(), case.lens.to(DEV))     # integer payloads
    z = build('C', d['x'], case.lens)
    with pytest.raises(ta.RuaError):
        O.launch_causal_conv(lay_of(z), z.data, d['w'], d['b'], False, (5,), out=d['w'])            # an unfit target


def test_zz_report():
    """Achieved error over bound, per dtype, kernel form and output (what the tests above measured in this process)."""
    for key in sorted(REPORT):
        print(f'causal_conv report: {key}: worst error / bound {REPORT[key]:.3f}')
    assert all(v <= 1.0 for v in REPORT.values())
