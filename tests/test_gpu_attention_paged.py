"""attention_paged on the GPU: bit for bit against `attention` over the rows the table names gathered into C containers
(an fp8 pool: dequantised and rounded to q's dtype first, exact for power-of-two scales), and against the float64
yardsticks attention_band_util.reference (out, b_out, A) and attention_decode_util.lse_reference.  The latter has no
no-merge form: it is called with n_split = 1, its smallest merge term, which over-counts here (nothing is merged).
`pool` / `case` are test_gpu_attention_decode_paged.py's: page ids from a seeded permutation, every pool row that is no
live key NaN, every unused table column naming a NaN page.  The shapes are edges: QL crosses the wave (32) and block
(128) column edges for G = 4 (32 / 33 queries: 128 / 132 columns), G = 3 (a query's heads straddle column 32, 64, 128)
and G = 1; KL crosses the 64-key tile and the page edges."""
import math
from itertools import product

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta
from torchrua_amd.layout import rewrap
import attention_band_util as U
import attention_decode_util as DU
from gpu_util import dispatch_trace
from test_gpu_attention import KINDS, build, padding
from test_gpu_attention_decode import draw_case, kw
from test_gpu_attention_decode_fp8 import deq, quantise
from test_gpu_attention_decode_paged import DEV, case, pool

pytestmark = pytest.mark.gpu

QL, KL = [33, 0, 1, 43, 32, 5], [65, 3, 0, 129, 64, 200]
QN, KN = [40, 3, 2], [17, 70, 0]                                # T_b > S_b under align='end': a negative shift
# (the keywords of attention_paged, those of attention for the same mask, the yardsticks' (align, left, right))
DEFAULT = ({}, dict(causal=True, align='end'), ('end', None, 0))
MASKS = [DEFAULT, (kw('end', 40, 0),) * 2 + (('end', 40, 0),), (kw('start', 33, 7),) * 2 + (('start', 33, 7),),
         (dict(causal=False), dict(causal=False, align='end'), ('end', None, None))]
EDGES = ([(QL, KL, D, (U.BF16, U.F16)[i % 2], f8, ps, hd, m)
          for i, (D, f8, ps) in enumerate(product((32, 64, 128), (False, True), (16, 32, 128)))
          for n, (hd, m) in enumerate(product(((4, 1), (6, 2), (8, 8)), MASKS)) if (i + n) % 6 == 0] +
         [(QN, KN, 64, U.F16, False, 16, (6, 2), DEFAULT), (QN, KN, 32, U.BF16, True, 32, (4, 1), DEFAULT)])


def run_paged(kind, q, qlens, paged, host=True, **kwargs):
    """(out, lse) in cat form on the CPU, after the checks every call must pass (type, metadata, zero padding)."""
    qc = build(kind, q, qlens, host)
    out, lse = qc.attention_paged(*paged, return_lse=True, **kwargs)
    assert type(out) is type(qc) and out.data.shape == qc.data.shape and out.data.dtype == qc.data.dtype
    assert out.batch_sizes is qc.batch_sizes if kind == 'P' else out.token_sizes is qc.token_sizes
    assert lse.dtype == torch.float32 and lse.shape == qc.data.shape[:-1] and not out.data.requires_grad
    if isinstance(qc, (ta.L, ta.R)):
        assert not out.data[padding(qc)].any() and not lse[padding(qc)].any(), 'padding rows are zeros'
    return [(d if isinstance(qc, ta.C) else rewrap(qc, d).cat().data).cpu() for d in (out.data, lse)]


def check(key, got, q, qlens, kd, vd, klens, mask, dtype, extra=None):
    """out within b_out (+ `extra(A)`) and lse within its bound of the float64 yardsticks fed the float64 cache `kd` /
    `vd`; the queries without a visible key: exact zeros and -inf.  Returns them."""
    (want, *_), (b_out, *_), A = U.reference(q, qlens, kd, vd, klens, torch.zeros_like(q), mask, None, dtype)
    lse, b_lse = DU.lse_reference(q, qlens, kd, klens, mask, None, 1)
    dead = torch.isinf(lse)
    if extra is not None:
        b_out, b_lse = b_out + extra[0] * A * (b_out > 0), b_lse + extra[1] * ~dead
    U.check(f'paged {key} out', got[0], want, b_out)
    assert bool((got[1][dead] == -float('inf')).all()) and not got[0][dead].any()
    U.check(f'paged {key} lse', got[1].masked_fill(dead, 0.0), lse.masked_fill(dead, 0.0), b_lse)
    return dead


def gathered(q, qlens, k, v, klens, **kwargs):
    """`attention` over the gathered cache: out in cat form on the CPU."""
    return build('C', q, qlens).attention(build('C', k, klens), build('C', v, klens), **kwargs).data.cpu()


@pytest.mark.parametrize('ql,kl,D,dtype,f8,ps,heads,mask', EDGES, ids=str)
def test_column_tile_and_page_edges(ql, kl, D, dtype, f8, ps, heads, mask):
    q, k, v, scales, s8 = case(ql, kl, heads, D, dtype, f8, 10 * D + ps)
    got = run_paged('C', q, ql, pool(k, v, kl, ps), **mask[0], **scales)
    kd, vd = (deq(k, s8[0]), deq(v, s8[1])) if f8 else (k.double(), v.double())
    assert torch.equal(kd.to(dtype).double(), kd) and torch.equal(vd.to(dtype).double(), vd), 'the dequantised cache is exact'
    assert torch.equal(got[0], gathered(q, ql, kd.to(dtype), vd.to(dtype), kl, **mask[1])), 'the bits of attention'
    key = f'{str(dtype)[6:]} D={D} fp8={f8} page={ps} heads={heads[0]}/{heads[1]} {mask[2]}'
    assert bool(check(key, got, q, ql, kd, vd, kl, mask[2], dtype).any()), 'a query without a visible key'


def test_a_scale_that_is_no_power_of_two():
    """amax / 448 as it comes: every score of a (sequence, head) is off by one factor 1 + d, |d| <= 2 e, which moves out by
    at most (exp(4 e smax) - 1) A and lse by 2 e smax; the v_scale multiply adds e A.  smax: the largest
    |scaled score| over all (query, key) pairs, hidden ones included."""
    ql, kl, heads, D, dtype = [40, 3], [131, 200], (4, 2), 64, U.BF16
    q, k, v = draw_case(ql, kl, heads, D, dtype, 21)
    (k8, ks), (v8, vs) = quantise(k, False), quantise(v, False)
    got = run_paged('C', q, ql, pool(k8, v8, kl, 16), k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    kd, vd = deq(k8, ks), deq(v8, vs)
    smax = D ** -0.5 * max(float(torch.einsum('thd,shd->ths', a.double().abs(), b.abs().repeat_interleave(2, 1)).max())
                           for a, b in zip(q.split(ql), kd.split(kl)))
    extra = (1.01 * (math.expm1(4 * U.E * smax) + U.E), 1.01 * 2 * U.E * smax)
    check('amax / 448 as it comes', got, q, ql, kd, vd, kl, DEFAULT[2], dtype, extra)


def test_the_four_q_layouts_give_the_same_bits_and_read_back_once(monkeypatch):
    PQ, PK = [33, 0, 5, 40], [131, 3, 0, 129]
    q, k, v = draw_case(PQ, PK, (6, 2), 32, U.F16, 7)
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    base = run_paged('C', q, PQ, pool(k, v, PK, 32))
    check('layouts', base, q, PQ, k.double(), v.double(), PK, DEFAULT[2], U.F16)
    for kind in KINDS:                                          # run_paged asserts the zero padding rows of L / R
        for got, exp, what in zip(run_paged(kind, q, PQ, pool(k, v, PK, 32)), base, ('out', 'lse')):
            assert torch.equal(got, exp), (kind, what)
    assert calls == [], calls                                   # host lengths: nothing is read back
    for got, exp in zip(run_paged('C', q, PQ, pool(k, v, PK, 32, host=False)), base):
        assert torch.equal(got, exp)
    assert calls == [(len(PK),)], calls                         # device-only kv_sizes: ONE [B] copy


def test_more_work_items_than_the_grid():
    POOL, TILES, D = 50, 14, 32                                 # 700 sequences x 4 kv heads x 1 block > 2 048 workgroups
    gen = torch.Generator().manual_seed(3)
    ql, kl = torch.randint(1, 4, (POOL,), generator=gen).tolist(), torch.randint(0, 71, (POOL,), generator=gen).tolist()
    q, k, v = draw_case(ql, kl, (4, 4), D, U.F16, 90)
    with dispatch_trace() as tr:
        got = run_paged('P', q.repeat(TILES, 1, 1), ql * TILES, pool(k.repeat(TILES, 1, 1), v.repeat(TILES, 1, 1), kl * TILES, 16))
    assert tr.matching('seg_attn_paged_forward_kernel heads=4 kvheads=4 left=-1 right=0 end=1 fp8=0 page=16 grid=2048'), tr.records
    n = sum(ql)
    for i in (1, TILES - 1):                                    # every tile holds the pool's bits; the pool's are within bound
        assert torch.equal(got[0][i * n:(i + 1) * n], got[0][:n]) and torch.equal(got[1][i * n:(i + 1) * n], got[1][:n])
    check('large batch', [g[:n] for g in got], q, ql, k.double(), v.double(), kl, DEFAULT[2], U.F16)


@pytest.mark.parametrize('ps', [16, 64])
def test_shared_pages_and_a_nan_page_past_the_end(ps):
    ql, kl = [35, 50], [2 * ps + 9, 3 * ps + 1]
    q, k, v = draw_case(ql, kl, (6, 2), 64, U.BF16, 77)
    for x in (k, v):
        x[kl[0]:kl[0] + 2 * ps] = x[:2 * ps]                    # a common prefix of two pages
    kp, vp, table, sizes = pool(k, v, kl, ps)
    want = run_paged('C', q, ql, (kp, vp, table, sizes))
    own = table[1, :2].clone()
    for x in (kp, vp):
        x[own.long()] = float('nan')                            # sequence 1's own copies are never read again
    table[1, :2] = table[0, :2]
    table[0, -(-kl[0] // ps):] = own[0]                         # past sequence 0's pages: a NaN page, never read
    got = run_paged('C', q, ql, (kp, vp, table, sizes))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    check(f'shared page={ps}', got, q, ql, k.double(), v.double(), kl, DEFAULT[2], U.BF16)
