"""attention_decode_paged on the GPU: bit for bit against attention_decode over the same keys in a C container at the same
`kv_chunk`, and against the float64 yardsticks of the decode tests.  `run`, `check`, the draws, the masks' keywords and
the QL / KL edge lists (KL crosses every page and step edge of the page sizes used) are test_gpu_attention_decode.py's;
`quantise` and the fp8 `check` test_gpu_attention_decode_fp8.py's.  Every pool row that is no live key is NaN."""
from itertools import product

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta
from torchrua_amd.layout import rewrap
import attention_band_util as U
from test_gpu_attention import KINDS, build, padding
from test_gpu_attention_decode import KL, QL, check, draw_case, kw, run
from test_gpu_attention_decode_fp8 import check as check8, quantise

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def pool(k, v, klens, ps, host=True, seed=0):
    """(k_pages, v_pages, page_table, kv_sizes) on the GPU for the cat-form caches `k` / `v` [N, heads_kv, D]: page ids
    from a seeded permutation, so the sequences' pages interleave; the tails of last pages and a spare page are NaN
    (0x7F.. is a NaN in e4m3, bf16 and f16) and every unused table column names the spare page."""
    n_pg = [-(-n // ps) for n in klens]
    perm = torch.randperm(sum(n_pg) + 1, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    table = perm[:1].repeat(len(klens), max(n_pg) + 1)
    rows, at = [], 1
    for b, n in enumerate(klens):
        table[b, :n_pg[b]] = perm[at:at + n_pg[b]]
        at += n_pg[b]
        s = torch.arange(n)
        rows.append(table[b, s // ps].long() * ps + s % ps)
    pages = []
    for x in (k, v):
        bits = torch.uint8 if x.element_size() == 1 else torch.int16
        flat = torch.full((perm.numel() * ps, *x.shape[1:]), 0x7F if x.element_size() == 1 else 0x7FFF, dtype=bits)
        flat[torch.cat(rows)] = x.view(bits)
        pages.append(flat.view(x.dtype).view(perm.numel(), ps, *x.shape[1:]).to(DEV))
    return (*pages, table.to(DEV), build('C', k, klens, host).token_sizes)


def run_paged(kind, q, qlens, paged, host=True, **kwargs):
    """(out, lse) in cat form on the CPU, after the checks `run` makes of a contiguous call."""
    qc = build(kind, q, qlens, host)
    out, lse = qc.attention_decode_paged(*paged, return_lse=True, **kwargs)
    assert type(out) is type(qc) and out.data.shape == qc.data.shape and out.data.dtype == qc.data.dtype
    assert lse.dtype == torch.float32 and lse.shape == qc.data.shape[:-1] and not out.data.requires_grad
    if isinstance(qc, (ta.L, ta.R)):
        assert not out.data[padding(qc)].any() and not lse[padding(qc)].any(), 'padding rows are zeros'
    return [(d if isinstance(qc, ta.C) else rewrap(qc, d).cat().data).cpu() for d in (out.data, lse)]


def case(qlens, klens, heads, D, dtype, f8, seed):
    """(q, k, v, the scale keywords of both calls, the arguments of the float64 check between `q, qlens` and `klens`)."""
    q, k, v = draw_case(qlens, klens, heads, D, dtype, seed)
    if not f8:
        return q, k, v, {}, None
    (k8, ks), (v8, vs) = quantise(k, True), quantise(v, True)
    return q, k8, v8, dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV)), (ks, vs)


def both(key, q, qlens, k, v, klens, scales, s8, ps, mask, dtype, kv_chunk):
    """The paged call equals the contiguous one bit for bit and is within the float64 bounds; returns the dead queries."""
    want = run('CC', q, qlens, k, v, klens, kv_chunk=kv_chunk, **kw(*mask), **scales)
    got = run_paged('C', q, qlens, pool(k, v, klens, ps), kv_chunk=kv_chunk, **kw(*mask), **scales)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), key
    if s8 is None:
        return check(f'paged {key}', got, q, qlens, k, v, klens, mask, None, dtype, kv_chunk)
    return check8(f'paged {key}', got, q, qlens, k, s8[0], v, s8[1], klens, mask, dtype, kv_chunk)


MASKS = [('end', 40, 0), ('start', 33, 7)]
EDGES = [(D, (U.BF16, U.F16)[(i + n) % 2], f8, ps, ch, m)
         for i, (D, f8, ps) in enumerate(product((32, 64, 128), (False, True), (16, 32, 128)))
         for n, (ch, m) in enumerate(product((None, 128), MASKS)) if (i + n) % 4 != 3]


@pytest.mark.parametrize('D,dtype,f8,ps,kv_chunk,mask', EDGES, ids=str)
def test_page_step_and_split_edges(D, dtype, f8, ps, kv_chunk, mask):
    q, k, v, scales, s8 = case(QL, KL, (4, 2), D, dtype, f8, 10 * D)
    key = f'{str(dtype)[6:]} D={D} fp8={f8} page={ps} {mask[0]} {mask[1]} {mask[2]} chunk={kv_chunk}'
    assert bool(both(key, q, QL, k, v, KL, scales, s8, ps, mask, dtype, kv_chunk).any())


@pytest.mark.parametrize('f8', [False, True])
@pytest.mark.parametrize('ps', [16, 256])
def test_a_split_walks_several_steps_and_many_pages(ps, f8):
    ql, kl = [4, 1, 2], [700, 385, 5]
    q, k, v, scales, s8 = case(ql, kl, (8, 2), 64, U.BF16, f8, 33)
    both(f'walk page={ps} fp8={f8}', q, ql, k, v, kl, scales, s8, ps, ('end', None, 0), U.BF16, 384)


@pytest.mark.parametrize('ps', [16, 64])
def test_two_sequences_share_pages(ps):
    ql, kl = [2, 3], [2 * ps + 9, 3 * ps + 1]
    q, k, v = draw_case(ql, kl, (4, 2), 64, U.F16, 77)
    for x in (k, v):
        x[kl[0]:kl[0] + 2 * ps] = x[:2 * ps]                    # a common prefix of two pages
    kp, vp, table, sizes = pool(k, v, kl, ps)
    for x in (kp, vp):
        x[table[1, :2].long()] = float('nan')                   # sequence 1's own copies are never read again
    table[1, :2] = table[0, :2]
    want = run('CC', q, ql, k, v, kl, kv_chunk=128)
    got = run_paged('C', q, ql, (kp, vp, table, sizes), kv_chunk=128)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_four_q_layouts_give_the_same_bits_and_read_back_once(monkeypatch):
    PQ, PK = [30, 0, 5, 32], [131, 3, 0, 129]
    q, k, v = draw_case(PQ, PK, (4, 2), 32, U.F16, 7)
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    base = run('CC', q, PQ, k, v, PK, kv_chunk=128)
    for kind in KINDS:                                          # run_paged asserts the zero padding rows of L / R
        for got, exp, what in zip(run_paged(kind, q, PQ, pool(k, v, PK, 32), kv_chunk=128), base, ('out', 'lse')):
            assert torch.equal(got, exp), (kind, what)
    assert calls == [], calls                                   # host lengths: nothing is read back
    paged = pool(k, v, PK, 32, host=False)
    for got, exp in zip(run_paged('C', q, PQ, paged, kv_chunk=128), base):
        assert torch.equal(got, exp)
    assert calls == [(len(PK),)], calls                         # device-only kv_sizes: ONE [B] copy
