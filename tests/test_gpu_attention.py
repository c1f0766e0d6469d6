"""Per-sequence attention on the GPU against the float64 yardstick of tests/attention_util.py within the bounds of DESIGN
3.2r: the tile edges of every D, dtype and mask, the 4 x 4 pairs of layouts bit for bit, batches larger than the grid, the
causal diagonal, the segment form, degenerate batches, the read-backs and the dispatch trace."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta
from torchrua_amd.layout import rewrap
import attention_util as U
from gpu_util import DEV, dispatch_trace

pytestmark = pytest.mark.gpu

KINDS = ('C', 'L', 'P', 'R')
NAMES = ('out', 'dq', 'dk', 'dv')


def build(kind, x, lens, host=True):
    lens = torch.as_tensor(lens, dtype=torch.long)
    c = ta.with_host_sizes(x.to(DEV), lens) if host else ta.C(x.to(DEV), lens.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def padding(z):
    T = z.data.size(1)
    pos, n = torch.arange(T, device=DEV).unsqueeze(0), z.token_sizes.to(DEV).unsqueeze(1)
    return pos >= n if isinstance(z, ta.L) else pos < T - n


def run(kinds, q, qlens, k, v, klens, g, causal=False, scale=None, host=True, built=None):
    """[out, dq, dk, dv] in cat form on the CPU, after the checks every call must pass (type, metadata, zero padding)."""
    conts = built or [build(kd, x, n, host) for kd, x, n in ((kinds[0], q, qlens), (kinds[1], k, klens), (kinds[1], v, klens),
                                                              (kinds[0], g, qlens))]
    leaves = [c.data.detach().requires_grad_() for c in conts[:3]]
    qc, kc, vc = (rewrap(c, leaf) for c, leaf in zip(conts, leaves))
    out = qc.attention(kc, vc, causal=causal, scale=scale)
    assert type(out) is type(qc) and out.data.shape == qc.data.shape and out.data.dtype == qc.data.dtype
    assert out.batch_sizes is qc.batch_sizes if kinds[0] == 'P' else out.token_sizes is qc.token_sizes
    out.data.backward(conts[3].data)
    res = [(qc, out.data.detach()), (qc, leaves[0].grad), (kc, leaves[1].grad), (vc, leaves[2].grad)]
    for (c, d), what in zip(res, NAMES):
        if isinstance(c, (ta.L, ta.R)) and d.numel():
            assert bool((d[padding(c)] == 0).all()), f'padding rows of {what} are zeros'
    return [(d if isinstance(c, ta.C) else rewrap(c, d).cat().data).cpu() for c, d in res]


def draw_case(qlens, klens, heads, D, dtype, seed):
    return [U.draw(n, heads, D, dtype, seed + i) for i, n in enumerate((qlens, klens, klens, qlens))]


def check_all(key, got, want, bounds):
    for g_, w, b, what in zip(got, want, bounds, NAMES):
        U.check(f'{key} {what}', g_, w, b)


# ------------------------------------------------------------------ the tile edges
QL = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 5, 64]
KL = [7, 0, 33, 32, 31, 65, 64, 63, 129, 128, 127, 257, 0, 1]


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('dtype', [U.BF16, U.F16])
@pytest.mark.parametrize('D', [32, 64, 128])
def test_tile_edges_forward_and_gradients(D, dtype, causal):
    q, k, v, g = draw_case(QL, KL, 3, D, dtype, 10 * D)
    want, bounds, A = U.reference(q, QL, k, v, KL, g, causal, None, dtype)
    got = run('CC', q, QL, k, v, KL, g, causal)
    assert bool((bounds[0] <= 4 * U.U[dtype] * A).all()), 'the forward bound hides no second rounding'
    check_all(f'{str(dtype)[6:]} D={D} causal={int(causal)}', got, want, bounds)
    # S = 0 < T: exact zeros, forward and gradients (sequences 1 and 12)
    for b in (1, 12):
        lo = sum(QL[:b])
        assert not got[0][lo:lo + QL[b]].any() and not got[1][lo:lo + QL[b]].any()


# ------------------------------------------------------------------ the 4 x 4 pairs of layouts, and the read-backs
PQ, PK = [130, 0, 5, 40], [131, 3, 0, 129]


def test_all_sixteen_pairs_of_layouts_give_the_same_bits():
    q, k, v, g = draw_case(PQ, PK, 2, 32, U.F16, 7)
    base = run('CC', q, PQ, k, v, PK, g)
    want, bounds, _ = U.reference(q, PQ, k, v, PK, g, False, None, U.F16)
    check_all('pairs', base, want, bounds)
    for a in KINDS:
        for b in KINDS:
            for got, exp, what in zip(run(a + b, q, PQ, k, v, PK, g), base, NAMES):
                assert torch.equal(got, exp), (a, b, what)
    for kinds in ('CC', 'RL'):                                  # device-only lengths give the same bits
        for got, exp, what in zip(run(kinds, q, PQ, k, v, PK, g, host=False), base, NAMES):
            assert torch.equal(got, exp), (kinds, what)


def test_read_backs(monkeypatch):
    q, k, v, g = draw_case(PQ, PK, 2, 32, U.BF16, 7)
    sides = {kd: [build(kd, x, n) for x, n in ((q, PQ), (k, PK), (v, PK), (g, PQ))] for kd in KINDS}
    dev_only = [build('C', x, n, host=False) for x, n in ((q, PQ), (k, PK), (v, PK), (g, PQ))]
    dev_only[2] = ta.C(dev_only[2].data, dev_only[1].token_sizes)
    torch.cuda.synchronize()
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    for a in KINDS:
        for b in KINDS:
            built = [sides[a][0], sides[b][1], sides[b][2], sides[a][3]]
            run(a + b, q, PQ, k, v, PK, g, built=built)
            assert calls == [], (a, b, calls)
    dev_only[0].attention(dev_only[1], dev_only[2])             # the forward: the q side alone
    assert calls == [(len(PQ),)], calls
    run('CC', q, PQ, k, v, PK, g, built=dev_only)               # ... the kv side when a gradient is requested, once
    run('CC', q, PQ, k, v, PK, g, built=dev_only)
    assert calls == [(len(PQ),), (len(PK),)], calls


# ------------------------------------------------------------------ more work items than the grid
def test_more_work_items_than_the_grid():
    POOL, TILES, H, D = 50, 60, 3, 32                           # 3 000 sequences x 3 heads > 2 048 workgroups
    gen = torch.Generator().manual_seed(3)
    ql, kl = (torch.randint(0, 7, (POOL,), generator=gen).tolist() for _ in range(2))
    q, k, v, g = draw_case(ql, kl, H, D, U.F16, 90)
    want, bounds, _ = U.reference(q, ql, k, v, kl, g, True, 0.25, U.F16)
    tile = lambda ts: [t.repeat(TILES, 1, 1) for t in ts]      # noqa: E731  (a sequence does not depend on its neighbours)
    tq, tk, tv, tg = tile((q, k, v, g))
    with dispatch_trace() as tr:
        got = run('CP', tq, ql * TILES, tk, tv, kl * TILES, tg, True, 0.25)
    check_all('large batch', got, tile(want), tile(bounds))
    for name in ('seg_attn_forward_kernel', 'seg_attn_dkdv_kernel', 'seg_attn_dq_kernel'):
        assert tr.matching(f'{name} grid=2048 causal=1'), tr.records


# ------------------------------------------------------------------ the causal diagonal
def test_causal_rows_do_not_see_later_keys():
    n, H, D = 129, 2, 64
    q, k, v, _ = draw_case([n], [n], H, D, U.BF16, 5)
    other_k, other_v = U.draw([n], H, D, U.BF16, 55), U.draw([n], H, D, U.BF16, 56)
    zq = build('C', q, [n])
    base = zq.attention(build('C', k, [n]), build('C', v, [n]), causal=True).data
    for t in (0, 30, 31, 32, 63, 64, 95, 127):
        k2, v2 = k.clone(), v.clone()
        k2[t + 1:], v2[t + 1:] = other_k[t + 1:], other_v[t + 1:]
        out = zq.attention(build('C', k2, [n]), build('C', v2, [n]), causal=True).data
        assert torch.equal(out[:t + 1], base[:t + 1]), t
        assert not torch.equal(out[t + 1:], base[t + 1:]), t


# ------------------------------------------------------------------ the segment form, degenerate batches, the trace
def test_segment_form_equals_the_container_form():
    q, k, v, _ = draw_case(PQ, PK, 2, 32, U.F16, 8)
    zq, zk, zv = build('C', q, PQ), build('C', k, PK), build('C', v, PK)
    seg = ta.segment_attention(zq.data, zq.token_sizes, zk.data, zv.data, zk.token_sizes, causal=True, scale=0.2)
    assert torch.equal(seg, ta.attention(zq, zk, zv, causal=True, scale=0.2).data)


@pytest.mark.parametrize('lens', [[], [0, 0, 0]])
def test_degenerate_batches_launch_nothing(lens):
    x = torch.zeros(0, 2, 32, dtype=U.BF16)
    with dispatch_trace() as tr:
        for a in (KINDS if lens else 'CLR'):
            for b in ('C', 'L'):
                out = build(a, x, lens).attention(build(b, x, lens), build(b, x, lens))
                assert out.data.numel() == 0 and out.data.dtype == U.BF16
    assert [r for r in tr.records if r.startswith('seg_attn')] == [], tr.records


def test_dispatch_trace_names_the_kernels():
    q, k, v, g = draw_case([40], [70], 3, 64, U.BF16, 2)
    with dispatch_trace() as tr:
        run('LP', q, [40], k, v, [70], g, True)
    assert tr.matching('seg_attn_forward_kernel D=64 heads=3 causal=1 kind=1 kvkind=2 grid=3'), tr.records
    assert {'seg_attn_delta_kernel', 'seg_attn_dkdv_kernel', 'seg_attn_dq_kernel'} <= set(tr.kernels), tr.records


def test_zz_report():
    for key in sorted(U.REPORT):
        print(f'attention report: {key} {U.REPORT[key]:.4f}')
