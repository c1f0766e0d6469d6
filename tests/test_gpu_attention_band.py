"""The band form of per-sequence attention on the GPU (grouped-query heads, windows, end-aligned masks) against the float64
yardstick of tests/attention_band_util.py within the bounds of DESIGN 3.2r: the tile edges of every mask and group, the
reductions to the plain form bit for bit, the 4 x 4 pairs of layouts, the band's two edges, batches larger than the grid
and the dispatch trace.  `build`, `padding` and the names are test_gpu_attention's; `run` is restated with the mask."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta
from torchrua_amd.layout import rewrap
import attention_band_util as U
from gpu_util import dispatch_trace
from test_gpu_attention import KINDS, NAMES, PK, PQ, build, padding

pytestmark = pytest.mark.gpu


def run(kinds, q, qlens, k, v, klens, g, host=True, **mask):
    """[out, dq, dk, dv] in cat form on the CPU; the gradients keep their storage shapes, padding rows are zeros."""
    conts = [build(kd, x, n, host) for kd, x, n in ((kinds[0], q, qlens), (kinds[1], k, klens), (kinds[1], v, klens),
                                                    (kinds[0], g, qlens))]
    leaves = [c.data.detach().requires_grad_() for c in conts[:3]]
    qc, kc, vc = (rewrap(c, leaf) for c, leaf in zip(conts, leaves))
    out = qc.attention(kc, vc, **mask)
    assert type(out) is type(qc) and out.data.shape == qc.data.shape and out.data.dtype == qc.data.dtype
    out.data.backward(conts[3].data)
    res = [(qc, out.data.detach()), (qc, leaves[0].grad), (kc, leaves[1].grad), (vc, leaves[2].grad)]
    for (c, d), what in zip(res, NAMES):
        assert d.shape == c.data.shape, f'{what} keeps the storage shape'
        if isinstance(c, (ta.L, ta.R)) and d.numel():
            assert bool((d[padding(c)] == 0).all()), f'padding rows of {what} are zeros'
    return [(d if isinstance(c, ta.C) else rewrap(c, d).cat().data).cpu() for c, d in res]


def draw_case(qlens, klens, heads, D, dtype, seed):
    return [U.draw(n, h, D, dtype, seed + i) for i, (n, h) in enumerate(zip((qlens, klens, klens, qlens), heads + heads[::-1]))]


def kw(align, left, right):
    return dict(align=align, window=(left, right))


QL = [0, 1, 129, 33, 130, 64, 65, 257, 128, 5, 40]
KL = [7, 129, 1, 130, 33, 64, 200, 257, 31, 0, 41]
MASKS = [('end', None, 0), ('end', 40, 0), ('start', 40, 0), ('start', 0, 0), ('start', 33, 7), ('end', 64, None),
         ('start', 300, 300)]
EDGES = ([(64, dt, hd, m) for dt in (U.BF16, U.F16) for hd in ((4, 4), (4, 2), (4, 1)) for m in MASKS] +
         [(D, U.BF16, (4, 2), ('end', 40, 0)) for D in (32, 128)])


@pytest.mark.parametrize('D,dtype,heads,mask', EDGES, ids=str)
def test_tile_edges_forward_and_gradients(D, dtype, heads, mask):
    q, k, v, g = draw_case(QL, KL, heads, D, dtype, 10 * D)
    want, bounds, _ = U.reference(q, QL, k, v, KL, g, mask, None, dtype)
    got = run('CC', q, QL, k, v, KL, g, **kw(*mask))
    for g_, w, b, what in zip(got, want, bounds, NAMES):
        U.check(f'band {str(dtype)[6:]} D={D} heads={heads[0]}/{heads[1]} {mask[0]} {mask[1]} {mask[2]} {what}', g_, w, b)
    dead = (bounds[0] == 0).flatten(1).all(1)                   # the queries without a visible key: exact zeros
    assert bool(dead.any()) and not got[0][dead].any() and not got[1][dead].any()


@pytest.mark.parametrize('band,plain,self_lens,heads', [
    (dict(window=(None, 0)), dict(causal=True), False, (4, 4)),
    (dict(align='end', causal=True), dict(causal=True), True, (4, 4)),
    (dict(window=300), dict(), False, (4, 4)),
    (kw('end', 40, 0), kw('end', 40, 0), False, (4, 2)),        # the group against repeat_interleave'd K / V: out, dq
], ids=str)
def test_reductions_bit_for_bit(band, plain, self_lens, heads):
    kl, G = (QL if self_lens else KL), heads[0] // heads[1]
    q, k, v, g = draw_case(QL, kl, heads, 64, U.BF16, 3)
    got = run('CC', q, QL, k, v, kl, g, **band)
    exp = run('CC', q, QL, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), kl, g, **plain)
    for a, b, what in list(zip(got, exp, NAMES))[:4 if G == 1 else 2]:
        assert torch.equal(a, b), what


def test_all_sixteen_pairs_of_layouts_give_the_same_bits(monkeypatch):
    mask = ('end', 40, 0)
    q, k, v, g = draw_case(PQ, PK, (4, 2), 32, U.F16, 7)
    base = run('CC', q, PQ, k, v, PK, g, **kw(*mask))
    want, bounds, _ = U.reference(q, PQ, k, v, PK, g, mask, None, U.F16)
    for g_, w, b, what in zip(base, want, bounds, NAMES):
        U.check(f'band pairs {what}', g_, w, b)
    for pair, host in [(a + b, True) for a in KINDS for b in KINDS] + [('CC', False), ('RL', False)]:
        for got, exp, what in zip(run(pair, q, PQ, k, v, PK, g, host=host, **kw(*mask)), base, NAMES):
            assert torch.equal(got, exp), (pair, host, what)
    dev_only = [build('C', x, n, host=False) for x, n in ((q, PQ), (k, PK))]
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    dev_only[0].attention(dev_only[1], ta.C(dev_only[1].data, dev_only[1].token_sizes), **kw(*mask))
    assert calls == [(len(PQ),)], calls                         # end alignment takes S - T on the device


def test_rows_see_their_band_and_nothing_else():
    T, S, W = 70, 199, 40
    q, k, v, _ = draw_case([T], [S], (2, 1), 64, U.BF16, 5)
    other_k, other_v = U.draw([S], 1, 64, U.BF16, 55), U.draw([S], 1, 64, U.BF16, 56)
    zq = build('C', q, [T])
    att = lambda k_, v_: zq.attention(build('C', k_, [S]), build('C', v_, [S]), causal=True, window=W, align='end').data  # noqa: E731
    base = att(k, v)
    for t in (0, 22, 23, 54, 55, 69):
        lo, hi = t + S - T - W, t + S - T                       # the first and the last visible key of row t
        outside = torch.ones(S, dtype=torch.bool)
        outside[lo:hi + 1] = False
        assert torch.equal(att(torch.where(outside[:, None, None], other_k, k), torch.where(outside[:, None, None], other_v, v))[t], base[t]), t
        for edge in (lo, hi):
            k2 = k.clone()
            k2[edge] = other_k[edge]
            assert not torch.equal(att(k2, v)[t], base[t]), (t, edge)


def test_more_work_items_than_the_grid():
    POOL, TILES, D = 50, 60, 32                                 # 3 000 sequences x 3 heads > 2 048 workgroups
    gen = torch.Generator().manual_seed(3)
    ql, kl = (torch.randint(0, 7, (POOL,), generator=gen).tolist() for _ in range(2))
    q, k, v, g = draw_case(ql, kl, (3, 1), D, U.F16, 90)
    want, bounds, _ = U.reference(q, ql, k, v, kl, g, ('start', 2, 0), 0.25, U.F16)
    tq, tk, tv, tg = (t.repeat(TILES, 1, 1) for t in (q, k, v, g))
    with dispatch_trace() as tr:
        got = run('CP', tq, ql * TILES, tk, tv, kl * TILES, tg, causal=True, window=2, scale=0.25)
        run('CC', q, ql, k.repeat_interleave(3, 1), v.repeat_interleave(3, 1), kl, g, causal=True)
    for g_, w, b, what in zip(got, want, bounds, NAMES):
        U.check(f'band large batch {what}', g_, w.repeat(TILES, 1, 1), b.repeat(TILES, 1, 1))
    for name in ('seg_attn_band_forward_kernel', 'seg_attn_band_dkdv_kernel', 'seg_attn_band_dq_kernel'):
        assert tr.matching(f'{name} heads=3 kvheads=1 left=2 right=0 end=0 grid=2048'), tr.records
    assert tr.matching('seg_attn_forward_kernel heads=3 causal=1'), tr.records


def test_zz_report():
    for key in sorted(k for k in U.REPORT if k.startswith('band ')):
        print(f'attention report: {key} {U.REPORT[key]:.4f}')
