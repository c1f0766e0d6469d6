"""attention_decode on the GPU against the float64 yardsticks of attention_band_util.reference (out) and
attention_decode_util.lse_reference (lse), within the bounds of DESIGN 3.2s: the tile and split edges of every mask and
group, the 4 x 4 pairs of layouts bit for bit with their read-backs, the band's two edges across splits, a plan that
splits by itself and a batch larger than the grid.  `build`, `padding`, the names and `draw` are the attention tests'.
In EDGES `kv_chunk=None` plans chunk 128 / 3 splits, the same as `kv_chunk=128`, and every split here is ONE 128-key
step; the plan's other choices and walks of several steps are test_gpu_attention_decode_walk.py's."""
import re

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta, _ops
from torchrua_amd.layout import rewrap
import attention_band_util as U
import attention_decode_util as DU
from gpu_util import dispatch_trace
from test_gpu_attention import KINDS, build, padding

pytestmark = pytest.mark.gpu


def run(kinds, q, qlens, k, v, klens, host=True, **kw):
    """(out, lse) in cat form on the CPU, after the checks every call must pass (type, metadata, zero padding)."""
    qc, kc, vc = (build(kd, x, n, host) for kd, x, n in ((kinds[0], q, qlens), (kinds[1], k, klens), (kinds[1], v, klens)))
    out, lse = qc.attention_decode(kc, vc, return_lse=True, **kw)
    assert type(out) is type(qc) and out.data.shape == qc.data.shape and out.data.dtype == qc.data.dtype
    assert out.batch_sizes is qc.batch_sizes if kinds[0] == 'P' else out.token_sizes is qc.token_sizes
    assert lse.dtype == torch.float32 and lse.shape == qc.data.shape[:-1] and not out.data.requires_grad
    if isinstance(qc, (ta.L, ta.R)):
        assert not out.data[padding(qc)].any() and not lse[padding(qc)].any(), 'padding rows are zeros'
    return [(d if isinstance(qc, ta.C) else rewrap(qc, d).cat().data).cpu() for d in (out.data, lse)]


def draw_case(qlens, klens, heads, D, dtype, seed):
    return [U.draw(n, h, D, dtype, seed + i) for i, (n, h) in enumerate(zip((qlens, klens, klens), heads + heads[1:]))]


def kw(align, left, right):
    return dict(causal=False, align=align, window=(left, right))


def check(key, got, q, qlens, k, v, klens, mask, scale, dtype, kv_chunk):
    """out and lse within their bounds; the queries without a visible key: exact zeros and -inf.  Returns them."""
    heads, D = (q.size(1), k.size(1)), q.size(2)
    n_split = _ops.attention_decode_plan(len(qlens), *heads, D, max(qlens), max(klens), kv_chunk)[1]
    (want, *_), (b_out, *_), A = U.reference(q, qlens, k, v, klens, torch.zeros_like(q), mask, scale, dtype)
    b_out = b_out + DU.merge_term(n_split) * A * (b_out > 0)
    assert bool((b_out <= 4 * U.U[dtype] * A).all()), 'the forward bound hides no second rounding'
    U.check(f'decode {key} out', got[0], want, b_out)
    lse, b_lse = DU.lse_reference(q, qlens, k, klens, mask, scale, n_split)
    dead = torch.isinf(lse)
    assert bool((got[1][dead] == -float('inf')).all()) and not got[0][dead.any(1)].any()
    U.check(f'decode {key} lse', got[1].masked_fill(dead, 0.0), lse.masked_fill(dead, 0.0), b_lse)
    return dead


QL = [0, 1, 2, 5, 32, 1, 3, 4, 1, 7, 1, 1]
KL = [7, 129, 1, 130, 33, 64, 200, 257, 31, 0, 128, 300]
MASKS = [('end', None, 0), ('end', 40, 0), ('start', None, None), ('start', 33, 7)]
EDGES = ([(64, dt, hd, m, ch) for dt in (U.BF16, U.F16) for hd in ((4, 4), (4, 2), (8, 1)) for m in MASKS for ch in (None, 128)] +
         [(D, U.BF16, (8, 1), ('end', 40, 0), 128) for D in (32, 128)])


@pytest.mark.parametrize('D,dtype,heads,mask,kv_chunk', EDGES, ids=str)
def test_tile_and_split_edges_forward_and_lse(D, dtype, heads, mask, kv_chunk):
    q, k, v = draw_case(QL, KL, heads, D, dtype, 10 * D)
    got = run('LC' if D == 32 else 'CC', q, QL, k, v, KL, kv_chunk=kv_chunk, **kw(*mask))
    key = f'{str(dtype)[6:]} D={D} heads={heads[0]}/{heads[1]} {mask[0]} {mask[1]} {mask[2]} chunk={kv_chunk}'
    assert bool(check(key, got, q, QL, k, v, KL, mask, None, dtype, kv_chunk).any())


def test_all_sixteen_pairs_of_layouts_give_the_same_bits(monkeypatch):
    PQ, PK = [30, 0, 5, 32], [131, 3, 0, 129]
    q, k, v = draw_case(PQ, PK, (4, 2), 32, U.F16, 7)
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    base = run('CC', q, PQ, k, v, PK, kv_chunk=128)
    check('pairs', base, q, PQ, k, v, PK, ('end', None, 0), None, U.F16, 128)
    for pair in [a + b for a in KINDS for b in KINDS]:
        for got, exp, what in zip(run(pair, q, PQ, k, v, PK, kv_chunk=128), base, ('out', 'lse')):
            assert torch.equal(got, exp), (pair, what)
    assert calls == [], calls                                   # host lengths: nothing is read back
    for pair in ('CC', 'RL'):
        for got, exp, what in zip(run(pair, q, PQ, k, v, PK, host=False, kv_chunk=128), base, ('out', 'lse')):
            assert torch.equal(got, exp), (pair, 'device-only', what)
    del calls[:]
    qd, kd = (build('C', x, n, host=False) for x, n in ((q, PQ), (k, PK)))
    qd.attention_decode(kd, ta.C(build('C', v, PK).data, kd.token_sizes), kv_chunk=128)
    assert calls == [(len(PQ),), (len(PK),)], calls             # device-only lengths: one [B] per side


def test_rows_see_their_band_and_nothing_else_across_splits():
    T, S, W = 3, 300, 40
    q, k, v = draw_case([T], [S], (2, 1), 64, U.BF16, 5)
    other_k, other_v = U.draw([S], 1, 64, U.BF16, 55), U.draw([S], 1, 64, U.BF16, 56)
    zq = build('C', q, [T])
    att = lambda k_, v_: zq.attention_decode(build('C', k_, [S]), build('C', v_, [S]), causal=True, window=W, align='end',  # noqa: E731
                                             kv_chunk=128).data
    base = att(k, v)
    for t in range(T):
        lo, hi = t + S - T - W, t + S - T                       # the first and the last visible key of row t
        outside = torch.ones(S, dtype=torch.bool)
        outside[lo:hi + 1] = False
        assert torch.equal(att(torch.where(outside[:, None, None], other_k, k), torch.where(outside[:, None, None], other_v, v))[t], base[t]), t
        for edge in (lo, hi):
            k2 = k.clone()
            k2[edge] = other_k[edge]
            assert not torch.equal(att(k2, v)[t], base[t]), (t, edge)


def test_the_plan_splits_by_itself():
    ql, kl = [1, 1], [5000, 37]
    q, k, v = draw_case(ql, kl, (4, 1), 32, U.BF16, 11)
    with dispatch_trace() as tr:
        got = run('CC', q, ql, k, v, kl)
    splits = [int(re.search(r'splits=(\d+)', r).group(1)) for r in tr.matching('seg_attn_decode_kernel heads=4 kvheads=1 end=1')]
    assert len(splits) == 1 and splits[0] > 1 and tr.matching('seg_attn_decode_combine_kernel'), tr.records
    check('plan splits', got, q, ql, k, v, kl, ('end', None, 0), None, U.BF16, None)


def test_more_work_items_than_the_grid():
    POOL, TILES, D = 50, 100, 32                                # 5 000 sequences x 1 kv head > 4 096 workgroups
    gen = torch.Generator().manual_seed(3)
    ql, kl = (torch.randint(0, 7, (POOL,), generator=gen).tolist() for _ in range(2))
    q, k, v = draw_case(ql, kl, (3, 1), D, U.F16, 90)
    with dispatch_trace() as tr:
        got = run('CP', q.repeat(TILES, 1, 1), ql * TILES, k.repeat(TILES, 1, 1), v.repeat(TILES, 1, 1), kl * TILES, window=2, scale=0.25)
    assert tr.matching('seg_attn_decode_kernel heads=3 kvheads=1 left=2 right=0 end=1 splits=1 grid=4096'), tr.records
    n = sum(ql)
    for i in (0, 1, TILES - 1):                                 # every tile holds the pool's bits; the pool's are within bound
        assert torch.equal(got[0][i * n:(i + 1) * n], got[0][:n]) and torch.equal(got[1][i * n:(i + 1) * n], got[1][:n])
    check('large batch', [g[:n] for g in got], q, ql, k, v, kl, ('end', 2, 0), 0.25, U.F16, None)


def test_zz_report():
    for key in sorted(k for k in U.REPORT if k.startswith('decode ')):
        print(f'attention report: {key} {U.REPORT[key]:.4f}')
