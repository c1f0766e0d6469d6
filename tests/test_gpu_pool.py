"""Per-sequence softmax-weighted sum (softmax_pool) on the GPU: the reference's stored results, every kernel form
against a float64 per-sequence torch evaluation, layout commutation bit for bit, padding, special values, gradients.

The yardstick is tests/pool_util.py:exact (float64) and the bounds are the ones stated there — 1e-5 times the sum of the
absolute terms of each result, plus one unit in the last place for bf16 / f16 payloads.  `ratio` is error / bound."""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from pool_util import DTYPES as DT, exact, load_cases, prod, ratio

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
REPORT = {}


def note(key, value):
    REPORT[key] = max(REPORT.get(key, 0.0), float(value))


# ------------------------------------------------------------------ helpers
def build(kind, x, lens_host, host_sizes=True):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def shifted(t):
    """The same contiguous tensor at a base that is off 16 bytes."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def run(kind, v, s, lens, cot=None, host_sizes=True, raw_scores=False, shift=False):
    """(out, grad_values in cat form, grad_scores in cat form, the two gradients in storage form) of the operator
    applied in layout `kind` to the cat-form data."""
    zv, zs = build(kind, v, lens, host_sizes), build(kind, s, lens, host_sizes)
    vd, sd = zv.data.detach().clone(), zs.data.detach().clone()
    if shift:
        vd, sd = shifted(vd), shifted(sd)
    if cot is None:
        out = rewrap(zv, vd).softmax_pool(sd if raw_scores else rewrap(zs, sd))
        return out, None, None, None, None
    vd.requires_grad_(True)
    sd.requires_grad_(True)
    out = rewrap(zv, vd).softmax_pool(sd if raw_scores else rewrap(zs, sd))
    assert out.shape == (lens.numel(),) + tuple(v.shape[1:]) and out.dtype == v.dtype
    out.backward(cot)
    return (out.detach(), rewrap(zv, vd.grad).cat().data, rewrap(zs, sd.grad).cat().data, vd.grad, sd.grad)


def check(got, v, s, cot, lens, what, key):
    out, gv, gs = got[:3]
    e = exact(v, s, cot, lens)
    r = [ratio(out, e['out'], e['b_out'], v.dtype)]
    if cot is not None:
        r += [ratio(gv, e['gv'], e['b_gv'], v.dtype), ratio(gs, e['gs'], e['b_gs'], v.dtype)]
    print(f'{what}: error / bound: ' + ', '.join(f'{x:.3f}' for x in r))
    for name, x in zip(('out', 'grad_values', 'grad_scores'), r):
        note(f'{key} {str(v.dtype)[6:]} {name}', x)
    for name, x in zip(('out', 'grad_values', 'grad_scores'), r):
        assert x <= 1.0, f'{what}: {name} at {x:.3f} of its bound'


def randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def inputs(lens, hidden, shidden, dtype, seed, scale=2.0):
    n = int(lens.sum())
    return (randn((n,) + hidden, dtype, seed), randn((n,) + shidden, dtype, seed + 1, scale),
            randn((lens.numel(),) + hidden, dtype, seed + 2))


def lengths(B, lo, hi, seed, empties=0):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi + 1, B)
    if empties:
        lens[rng.choice(B, empties, replace=False)] = 0
    return torch.from_numpy(lens.astype(np.int64))


# ------------------------------------------------------------------ fixtures from the reference
CASES = load_cases()


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture(name, kind):
    c = CASES[name]
    dtype, lens = DT[c['dtype']], c['lens']
    v, s, cot = (c[k].to(dtype).to(DEV) for k in ('v', 's', 'cot'))
    got = run(kind, v, s, lens, cot)
    check(got, v, s, cot, lens, f'{name} {kind}', 'fixtures')
    # ... and the reference's own stored results: the kernels within their bound, the reference within half of it
    e = exact(v, s, cot, lens)
    for k, b, g in (('out', 'b_out', got[0]), ('gv', 'b_gv', got[1]), ('gs', 'b_gs', got[2])):
        assert ratio(g, c[k], 1.5 * e[b], dtype) <= 1.0, f'{name} {kind}: {k} against the reference'


# ------------------------------------------------------------------ every kernel form
FORM_LENS = torch.tensor([0, 1, 31, 32, 33, 129, 2100, 64], dtype=torch.long)
# (id, kind, hidden, score hidden, dtype, shift, forward record, backward record)
FORMS = [
    ('lanes_2B', 'C', (), (), BF16, False, 'seg_pool_lanes_kernel W=2 kind=0', 'seg_pool_backward_kernel form=lanes W=2'),
    ('lanes_4B', 'L', (), (), F32, False, 'seg_pool_lanes_kernel W=4 kind=1', 'seg_pool_backward_kernel form=lanes W=4 kind=1'),
    ('lanes_8B', 'P', (2,), (), F32, False, 'seg_pool_lanes_kernel W=8 kind=2', 'seg_pool_backward_kernel form=lanes W=8 kind=2'),
    ('lanes_16B', 'R', (8,), (), BF16, False, 'seg_pool_lanes_kernel W=16 AL=1 kind=3', 'seg_pool_backward_kernel form=lanes W=16 kind=3'),
    ('lanes_16B_heads', 'C', (4, 2), (4,), F16, False, 'seg_pool_lanes_kernel W=16 D=2', 'seg_pool_backward_kernel form=lanes D=2'),
    ('lanes_f64', 'C', (2,), (2,), F64, False, 'seg_pool_lanes_kernel T=f64 D=1', 'seg_pool_backward_kernel T=f64 form=lanes'),
    ('rows_aligned', 'C', (64,), (), F32, False, 'seg_pool_rows_kernel AL=1 lane=1 D=64 chunks=2',
     'seg_pool_backward_kernel AL=1 form=team UE=4 S=16'),
    ('rows_heads_bf16', 'P', (4, 16), (4,), BF16, False, 'seg_pool_rows_kernel AL=1 lane=1 D=16 kind=2',
     'seg_pool_backward_kernel AL=1 form=team UE=8 S=2 kind=2'),
    ('rows_odd_heads', 'L', (3, 5), (3,), F32, False, 'seg_pool_rows_kernel AL=0 lane=0 D=5 kind=1',
     'seg_pool_backward_kernel AL=0 form=team UE=1 S=8 kind=1'),
    ('rows_odd_wide', 'R', (125,), (), BF16, False, 'seg_pool_rows_kernel AL=0 lane=0 D=125 kind=3',
     'seg_pool_backward_kernel AL=0 form=team UE=1 S=64 kind=3'),
    ('rows_per_column', 'C', (64,), (64,), F32, False, 'seg_pool_rows_kernel AL=1 lane=0 D=1',
     'seg_pool_backward_kernel AL=0 form=team UE=1 S=1'),
    ('rows_shifted', 'C', (64,), (), F32, True, 'seg_pool_rows_kernel AL=0 lane=1 D=64',
     'seg_pool_backward_kernel AL=0 form=team UE=4 S=16'),
    ('rows_wide_f64', 'P', (2, 40), (2,), F64, False, 'seg_pool_rows_kernel T=f64 AL=1 lane=1 D=40',
     'seg_pool_backward_kernel T=f64 AL=1 form=team UE=2 S=32'),
    ('rows_wide_bf16', 'C', (1024,), (), BF16, False, 'seg_pool_rows_kernel AL=1 lane=1 D=1024 chunks=16',
     'seg_pool_backward_kernel AL=1 form=team UE=8 S=64'),
    ('rows_very_wide', 'C', (2048,), (), F32, False, 'seg_pool_rows_kernel AL=1 lane=1 D=2048 chunks=64',
     'seg_pool_backward_kernel AL=1 form=team UE=4 S=64'),
]


@pytest.mark.parametrize('form', FORMS, ids=[f[0] for f in FORMS])
def test_kernel_form(form):
    fid, kind, hidden, shidden, dtype, shift, fwd_rec, bwd_rec = form
    v, s, cot = inputs(FORM_LENS, hidden, shidden, dtype, 11)
    with dispatch_trace() as tr:
        got = run(kind, v, s, FORM_LENS, cot, shift=shift)
    assert tr.matching(fwd_rec), f'{fid}: wanted {fwd_rec}, got {tr.records}'
    assert tr.matching(bwd_rec), f'{fid}: wanted {bwd_rec}, got {tr.records}'
    check(got, v, s, cot, FORM_LENS, fid, 'forms')


BLOCKS = torch.tensor([0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 5, 0, 4100], dtype=torch.long)
LONG = torch.tensor([8197, 10240, 5], dtype=torch.long)


@pytest.mark.parametrize('lens', (BLOCKS, LONG), ids=('blocks', 'long'))
@pytest.mark.parametrize('hidden,shidden,dtype', [((), (), F32), ((8,), (), BF16), ((64,), (), F32), ((3, 5), (3,), F32),
                                                  ((4, 16), (4,), BF16)], ids=str)
def test_block_boundaries_and_long_sequences(lens, hidden, shidden, dtype):
    v, s, cot = inputs(lens, hidden, shidden, dtype, 21, scale=3.0)
    for kind in 'CP':
        check(run(kind, v, s, lens, cot), v, s, cot, lens, f'{kind} {hidden}', 'blocks' if lens is BLOCKS else 'long')


# ------------------------------------------------------------------ bit for bit
COMMUTE = [((), (), F32), ((8,), (), BF16), ((64,), (), F32), ((3, 5), (3,), F32), ((4, 16), (4,), BF16), ((2,), (2,), F64)]


@pytest.mark.parametrize('hidden,shidden,dtype', COMMUTE, ids=str)
def test_layouts_lengths_alignment_and_score_forms_give_the_same_bits(hidden, shidden, dtype):
    lens = torch.cat([lengths(30, 0, 70, 5), torch.tensor([256, 257, 2048, 2049, 4500, 0, 1])])
    v, s, cot = inputs(lens, hidden, shidden, dtype, 31, scale=3.0)
    want = run('C', v, s, lens, cot)
    for what, got in (('device-only lengths', run('C', v, s, lens, cot, host_sizes=False)),
                      ('L', run('L', v, s, lens, cot)), ('R', run('R', v, s, lens, cot)), ('P', run('P', v, s, lens, cot)),
                      ('shifted base', run('C', v, s, lens, cot, shift=True)),
                      ('shifted base, P', run('P', v, s, lens, cot, shift=True)),
                      ('raw scores', run('C', v, s, lens, cot, raw_scores=True)),
                      ('raw scores, L', run('L', v, s, lens, cot, raw_scores=True))):
        for name, a, b in zip(('out', 'grad_values', 'grad_scores'), got[:3], want[:3]):
            assert torch.equal(a, b), f'{what}: {name} differs from the CattedSequence result'
    assert torch.equal(ta.segment_softmax_pool(v, s, lens.to(DEV)), want[0])


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden,shidden,dtype', [((64,), (), F32), ((4, 16), (4,), BF16), ((), (), F32)], ids=str)
def test_consistent_with_softmax_and_reduce_sum(kind, hidden, shidden, dtype):
    """softmax_pool(v, s) against reduce_sum of v * s.softmax() broadcast, within the forward bound (no factor on it).
    The composed side runs the library's softmax and reduce_sum in fp32: for a bf16 payload on the exactly upcast
    inputs, because composed IN bf16 the spelling rounds every weight and every product to bf16 before it sums, which is
    a property of the spelling and not of either operator."""
    lens = lengths(40, 0, 90, 6)
    v, s, _ = inputs(lens, hidden, shidden, dtype, 41)
    zv, zs = build(kind, v, lens), build(kind, s, lens)
    got = zv.softmax_pool(zs)
    G, H = prod(shidden), prod(hidden)
    tok = tuple(zv.data.shape[:zv.data.dim() - len(hidden)])
    w = rewrap(zs, zs.data.float()).softmax().data
    wide = (w.reshape(tok + (G, 1)) * zv.data.float().reshape(tok + (G, H // G))).reshape(zv.data.shape)
    composed = ta.reduce_sum(rewrap(zv, wide.contiguous()))
    assert composed.dtype == F32 and got.dtype == dtype
    e = exact(v, s, None, lens, want_grad=False)
    r = ratio(got, composed, e['b_out'], dtype)
    print(f'composed {kind} {hidden} {dtype}: error / bound: {r:.3f}')
    note(f'composed {str(dtype)[6:]}', r)
    assert r <= 1.0


# ------------------------------------------------------------------ semantics
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden,shidden', [((), ()), ((64,), ()), ((4, 16), (4,))], ids=str)
def test_empty_sequences(kind, hidden, shidden):
    lens = torch.tensor([0, 0, 5, 0, 1, 0, 0, 40, 3, 0], dtype=torch.long)
    v, s, cot = inputs(lens, hidden, shidden, F32, 51)
    got = run(kind, v, s, lens, cot)
    check(got, v, s, cot, lens, f'empties {kind}', 'empties')
    assert bool((got[0][lens.to(DEV) == 0] == 0).all())


@pytest.mark.parametrize('hidden,shidden', [((), ()), ((64,), ())], ids=str)
def test_only_empty_sequences_and_no_sequences(hidden, shidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        B = lens.numel()
        v = torch.empty((0,) + hidden, device=DEV, requires_grad=True)
        s = torch.empty((0,) + shidden, device=DEV, requires_grad=True)
        out = ta.segment_softmax_pool(v, s, lens.to(DEV))
        assert out.shape == (B,) + hidden and bool((out == 0).all())
        out.sum().backward()
        assert v.grad.shape == v.shape and s.grad.shape == s.shape
        if B:
            pad = torch.full((B, 4) + hidden, float('nan'), device=DEV)
            spad = torch.full((B, 4) + shidden, float('nan'), device=DEV)
            for cls in (ta.L, ta.R):
                assert bool((cls(pad, lens.to(DEV)).softmax_pool(spad) == 0).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden,shidden', [((), ()), ((4,), ()), ((4, 16), (4,))], ids=str)
def test_nan_and_infinities_stay_in_their_sequence_and_column(kind, hidden, shidden):
    inf, nan = float('inf'), float('nan')
    lens = torch.tensor([6, 3, 40, 5, 300, 4, 7], dtype=torch.long)
    v, s, _ = inputs(lens, hidden, shidden, F32, 61)
    off = torch.cumsum(lens, 0) - lens
    sc, vc = (0,) * len(shidden), (0,) * len(hidden)
    s[(int(off[0]) + 2,) + sc] = nan                         # a NaN score
    s[(int(off[1]) + 1,) + sc] = inf                         # a +inf score
    s[(slice(int(off[3]), int(off[3]) + 5),) + sc] = -inf    # a score column of -inf only
    s[(int(off[4]) + 17,) + sc] = -inf                       # an inf VALUE at weight 0 ...
    v[(int(off[4]) + 17,) + vc] = inf
    s[(int(off[6]) + 1,) + sc] = -inf                        # ... and a finite value at weight 0
    out = run(kind, v, s, lens)[0]
    want = exact(v, s, None, lens, want_grad=False)
    assert torch.equal(torch.isnan(out).cpu(), torch.isnan(want['out'])), 'NaN positions'
    assert bool(torch.isnan(out[0]).reshape(-1)[0]) and bool(torch.isnan(out[4]).reshape(-1)[0])
    assert bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(out[5]).all()) and bool(torch.isfinite(out[6]).all())
    assert ratio(out, want['out'], want['b_out']) <= 1.0


@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden,shidden', [((), ()), ((8,), ()), ((64,), ()), ((3, 5), (3,))], ids=str)
def test_padding_is_never_read_and_its_gradient_is_zero(kind, hidden, shidden):
    lens = lengths(40, 0, 50, 7)
    v, s, cot = inputs(lens, hidden, shidden, F32, 71)
    zv, zs = build(kind, v, lens), build(kind, s, lens)
    T = zv.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)

    def dirty(t):
        m = live.reshape(live.shape + (1,) * (t.dim() - 2)).expand_as(t)
        junk = torch.tensor([float('nan'), float('inf'), 1e9, float('-inf')], device=DEV)
        return torch.where(m, t, junk[torch.arange(t.numel(), device=DEV) % 4].reshape(t.shape)), m
    res = []
    for vd, sd in ((zv.data.clone(), zs.data.clone()), (dirty(zv.data)[0], dirty(zs.data)[0])):
        vd.requires_grad_(True)
        sd.requires_grad_(True)
        out = rewrap(zv, vd).softmax_pool(sd)
        out.backward(cot)
        res.append((out.detach(), vd.grad, sd.grad))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    mv, ms = dirty(zv.data)[1], dirty(zs.data)[1]
    assert bool((res[1][1][~mv] == 0).all()) and bool((res[1][2][~ms] == 0).all())
    assert bool(torch.isfinite(res[1][1]).all()) and bool(torch.isfinite(res[1][2]).all())


def test_sliced_values():
    lens = lengths(30, 1, 40, 10)
    n = int(lens.sum())
    big = randn((n, 24), F32, 81).requires_grad_(True)
    s = randn((n,), F32, 82).requires_grad_(True)
    cot = randn((lens.numel(), 12), F32, 83)
    x = big[:, ::2]
    assert not x.is_contiguous()
    out = ta.segment_softmax_pool(x, s, lens.to(DEV))
    out.backward(cot)
    want = run('C', x.detach().contiguous(), s.detach(), lens, cot)
    assert torch.equal(out.detach(), want[0]) and torch.equal(s.grad, want[2])
    assert torch.equal(big.grad[:, ::2], want[1]) and bool((big.grad[:, 1::2] == 0).all())


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('hidden,shidden', [((), ()), ((3,), ()), ((2, 3), (2,))], ids=str)
def test_gradcheck(kind, hidden, shidden):
    lens = torch.tensor([3, 1, 0, 5, 2], dtype=torch.long)
    v, s, _ = inputs(lens, hidden, shidden, F64, 91, scale=1.0)
    zv, zs = build(kind, v, lens), build(kind, s, lens)

    def f(vd, sd):
        return rewrap(zv, vd).softmax_pool(rewrap(zs, sd))
    vl, sl = zv.data.detach().clone().requires_grad_(True), zs.data.detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (vl, sl), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize('hidden,shidden,dtype', [((8,), (), BF16), ((4, 16), (4,), BF16), ((125,), (), F16), ((), (), F16)],
                         ids=str)
def test_every_output_is_rounded_once_with_and_without_autograd(hidden, shidden, dtype):
    """Under autograd the kernel hands a bf16 / f16 `out` unrounded (fp32) and ATen rounds it; without, the kernel rounds
    it itself.  One rounding of the same fp32 value either way: the same bits."""
    v, s, cot = inputs(FORM_LENS, hidden, shidden, dtype, 141)
    with torch.no_grad():
        plain = ta.segment_softmax_pool(v, s, FORM_LENS.to(DEV))
    assert plain.dtype == dtype and torch.equal(plain, run('C', v, s, FORM_LENS, cot)[0])


def test_a_hidden_shape_with_a_zero_dim_gives_empty_results_and_zero_gradients():
    lens = torch.tensor([2, 0, 3], device=DEV)
    for hidden, shidden in (((0,), ()), ((4, 0), (4,)), ((0, 4), (0,))):
        v = torch.randn((5,) + hidden, device=DEV, requires_grad=True)
        s = torch.randn((5,) + shidden, device=DEV, requires_grad=True)
        out = ta.segment_softmax_pool(v, s, lens)
        assert out.shape == (3,) + hidden
        out.sum().backward()
        assert v.grad.shape == v.shape and s.grad.shape == s.shape and bool((s.grad == 0).all())


def test_gradients_flow_to_either_input_alone():
    lens = lengths(20, 0, 30, 12)
    v, s, cot = inputs(lens, (16,), (), F32, 101)
    both = run('C', v, s, lens, cot)
    vl = v.clone().requires_grad_(True)
    ta.segment_softmax_pool(vl, s, lens.to(DEV)).backward(cot)
    sl = s.clone().requires_grad_(True)
    ta.segment_softmax_pool(v, sl, lens.to(DEV)).backward(cot)
    assert torch.equal(vl.grad, both[1]) and torch.equal(sl.grad, both[2])


def test_create_graph_raises():
    lens = torch.tensor([3, 2], dtype=torch.long)
    v, s, cot = inputs(lens, (4,), (), F32, 111)
    v.requires_grad_(True)
    s.requires_grad_(True)
    out = ta.segment_softmax_pool(v, s, lens.to(DEV))
    g, = torch.autograd.grad(out, v, cot, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.parametrize('dtype', (F32, BF16))
def test_saved_tensors_hold_nothing_of_payload_size_but_the_inputs(dtype):
    lens = lengths(20, 1, 30, 12)
    v, s, _ = inputs(lens, (16,), (), dtype, 121)
    v.requires_grad_(True)
    s.requires_grad_(True)
    out = ta.with_host_sizes(v, lens).softmax_pool(s)
    saved = out.grad_fn.saved_tensors
    big = [t for t in saved if t.numel() >= v.numel()]
    assert len(big) == 1 and big[0].data_ptr() == v.data_ptr()
    assert sorted(t.numel() for t in saved) == sorted([v.numel(), s.numel(), out.numel(), lens.numel()])


def test_no_aten_softmax_mul_or_sum_kernel_runs():
    from torch.profiler import ProfilerActivity, profile
    lens = lengths(50, 1, 60, 13)
    v, s, cot = inputs(lens, (64,), (), BF16, 131)
    z = ta.with_host_sizes(v.requires_grad_(True), lens)
    s.requires_grad_(True)
    z.softmax_pool(s).backward(cot)                   # (warm-up: lengths, offsets)
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        z.softmax_pool(s).backward(cot)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    banned = [n for n in names if n.startswith('aten::') and any(w in n for w in ('softmax', 'mul', 'sum', 'exp'))]
    assert not banned, banned


def test_refusals():
    lens = torch.tensor([2, 3], device=DEV)
    v = torch.randn(5, 4, 6, device=DEV)
    with pytest.raises(ta.RuaError):                   # integer payload
        ta.segment_softmax_pool(torch.arange(5, device=DEV), torch.arange(5, device=DEV), lens)
    with pytest.raises(ta.RuaError):                   # scores of another dtype
        ta.segment_softmax_pool(v, torch.randn(5, device=DEV, dtype=torch.float64), lens)
    for shape in ((4,), (5, 6), (5, 4, 6, 1), (5, 1), (5, 4, 3)):
        with pytest.raises(ta.RuaError):               # not the token dims + a prefix of the hidden dims
            ta.segment_softmax_pool(v, torch.randn(shape, device=DEV), lens)
    for shape in ((5,), (5, 4), (5, 4, 6)):
        assert ta.segment_softmax_pool(v, torch.randn(shape, device=DEV), lens).shape == (2, 4, 6)
    c = ta.C(v, lens)
    with pytest.raises(ta.RuaError):                   # a container of another type
        c.softmax_pool(ta.L(torch.randn(2, 3, device=DEV), lens))
    with pytest.raises(ta.RuaError):                   # a CPU tensor
        c.softmax_pool(torch.randn(5))
    p = ta.with_host_sizes(v, lens.cpu()).pack()
    other = ta.with_host_sizes(torch.randn(5, device=DEV), torch.tensor([4, 1])).pack()
    with pytest.raises(ta.RuaError):                   # PackedSequences with different batch_sizes
        p.softmax_pool(other)


def test_zz_report():
    """The worst error / bound of this run, per group, dtype and result (for the GPU test log)."""
    for key in sorted(REPORT):
        print(f'softmax_pool report: {key}: {REPORT[key]:.3f}')
