"""Per-sequence cummax / cummin / logcumsumexp on the GPU: every kernel form against the yardsticks of
tests/cumext_util.py (torch.cummax / cummin exact in both outputs; float64 torch.logcumsumexp at the bound derived
there), the bit-for-bit identities (casts commute, reverse is the mirrored forward scan, cut == uncut, unaligned ==
aligned), special values, padding, empty inputs, layouts and widths, gradients, and one ListMLE loss."""
import math

import pytest
import torch

import torchrua_amd as ta
import cumext_util as U
from cumext_util import BF16, F16, F32, F64, I64, CROSSING, CUT, RAGGED
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

OPS = ('cummax', 'cummin', 'logcumsumexp')
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------ helpers
def LT(*values):
    return torch.tensor(values, dtype=torch.long)


def build(kind, x, lens_host, host_sizes=True):
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def lay_of(z):
    return M.lay_pack(z) if isinstance(z, ta.P) else describe(z)


def shifted(t):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def apply(op, z, reverse):
    """(values container, indices container or None) of `op` on the container z."""
    out = getattr(z, op)(reverse=reverse)
    if op == 'logcumsumexp':
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == z.data.dtype
        return out, None
    assert isinstance(out, ta.SeqCum) and type(out.values) is type(z) and type(out.indices) is type(z)
    assert out.values.data.shape == z.data.shape == out.indices.data.shape
    assert out.values.data.dtype == z.data.dtype and out.indices.data.dtype == I64
    if not isinstance(z, ta.P):
        assert out.values.token_sizes is z.token_sizes and out.indices.token_sizes is z.token_sizes
    return out.values, out.indices


def run(op, kind, x, lens, reverse, cot=None, host_sizes=True):
    """(values, indices, grad), each in cat form (None where there is none)."""
    z = build(kind, x, lens, host_sizes)
    leaf = z.data.detach().clone().requires_grad_(cot is not None)
    v, i = apply(op, rewrap(z, leaf), reverse)
    g = None
    if cot is not None:
        v.data.backward(build(kind, cot, lens, host_sizes).data)
        g = rewrap(z, leaf.grad).cat().data
    return v.cat().data.detach(), None if i is None else i.cat().data, g


def same_bits(a, b):
    if a.is_floating_point():
        a, b = a.contiguous(), b.contiguous()
        w = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.shape == b.shape and torch.equal(a.view(w), b.view(w))
    return torch.equal(a, b)


def check(op, x, lens, reverse, v, i, g, cot, what, key):
    """The three outputs (cat form) against the yardsticks."""
    xc, lc = x.cpu(), lens.cpu()
    if op == 'logcumsumexp':
        U.check_lse(v, xc, lc, reverse, what, key)
        if g is not None:
            U.check_lse_grad(g, xc, v, cot, lc, reverse, what, key)
        return
    wv, wi = U.seg_cumextreme(xc, lc, op == 'cummax', reverse)
    assert same_bits(v.cpu(), wv), f'{what}: values differ from torch.{op}'
    assert torch.equal(i.cpu(), wi), f'{what}: indices differ from torch.{op}'
    if g is not None:
        c64 = cot.cpu().double()
        want = U.seg_run_sum(c64, wi, lc, reverse)
        bound = U.BAR * U.seg_run_sum(c64.abs(), wi, lc, reverse)
        if x.dtype in (BF16, F16):
            bound = bound + 0.5 * U.ulp_at(want, x.dtype)
        err = (g.cpu().double() - want).abs()
        assert bool((err[bound == 0] == 0).all()), f'{what}: a token that never wins has a gradient'
        if (bound > 0).any():
            ratio = (err[bound > 0] / bound[bound > 0]).max().item()
            U.note(f'{key} {op} grad', ratio)
            assert ratio <= 1.0, f'{what}: gradient {ratio:.3f} x the bar'


# ------------------------------------------------------------------ every kernel form, at the smallest shape that reaches it
KERNEL = {'cummax': 'seg_cumextreme', 'cummin': 'seg_cumextreme', 'logcumsumexp': 'seg_logcumsumexp'}
# (id, kind, lens, hidden, dtype, shift the base?, form and key=value pairs of the record)
PATHS = [
    ('lanes_2B', 'C', RAGGED, (), BF16, False, 'lanes_kernel T=bf16 W=2 AL=0'),
    ('lanes_4B', 'P', RAGGED, (), F32, False, 'lanes_kernel T=f32 W=4 AL=0'),
    ('lanes_8B', 'L', RAGGED, (), F64, False, 'lanes_kernel T=f64 W=8 AL=0 kind=1'),
    ('lanes_16B', 'C', RAGGED, (8,), BF16, False, 'lanes_kernel T=bf16 W=16 AL=1'),
    ('lanes_16B_shifted', 'C', RAGGED, (8,), BF16, True, 'lanes_kernel T=bf16 W=2 AL=0'),
    ('rows_aligned', 'C', RAGGED, (64,), F32, False, 'rows_kernel T=f32 AL=1 cut=0'),
    ('rows_aligned_R', 'R', RAGGED, (64,), F32, False, 'rows_kernel T=f32 AL=1 cut=0 kind=3'),
    ('rows_odd_width', 'C', RAGGED, (125,), F32, False, 'rows_kernel T=f32 AL=0 cut=0'),
    ('rows_shifted_base', 'C', RAGGED, (64,), F32, True, 'rows_kernel T=f32 AL=0 cut=0'),
    ('rows_P_f16', 'P', RAGGED, (24,), F16, False, 'rows_kernel T=f16 AL=1 cut=0 kind=2'),
    ('cut_partial', 'C', CUT, (64,), F32, False, 'rows_kernel T=f32 AL=1 cut=1 phase=partial'),
    ('cut_finish', 'C', CUT, (64,), F32, False, 'rows_kernel T=f32 AL=1 cut=1 phase=finish'),
]


@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path, op, reverse):
    pid, kind, lens, hidden, dtype, shift, rec = path
    n = int(lens.sum())
    x = U.draw((n,) + hidden, dtype, 11).to(DEV)
    cot = U.draw((n,) + hidden, dtype, 12).to(DEV)
    if shift:                                        # (forward only: autograd's leaf would be a fresh, aligned copy)
        z = ta.with_host_sizes(shifted(x), lens)
        with dispatch_trace() as tr:
            out, idx = apply(op, z, reverse)
        v, i, g, cot = out.data, None if idx is None else idx.data, None, None
    else:
        with dispatch_trace() as tr:
            v, i, g = run(op, kind, x, lens, reverse, cot)
    want = f'{KERNEL[op]}_{rec} rev={int(reverse)}'
    assert tr.matching(want), f'{pid}: wanted {want}, got {tr.records}'
    if g is not None:                                # the backward: the library's own kernel, against the direction
        assert tr.matching(f'{KERNEL[op]}_bwd_{rec} rev={int(not reverse)}'), f'{pid}: backward, got {tr.records}'
    check(op, x, lens, reverse, v, i, g, cot, f'{pid} {op} rev={int(reverse)}', pid)


@pytest.mark.parametrize('op', ('cummax', 'cummin'))
def test_int64_and_indices_only(op):
    lens = RAGGED
    for hidden in ((), (3,), (20,)):
        x = U.draw((int(lens.sum()),) + hidden, I64, 13).to(DEV)
        for kind in 'CLPR':
            for reverse in (False, True):
                v, i, _ = run(op, kind, x, lens, reverse)
                check(op, x, lens, reverse, v, i, None, None, f'int64 {kind} {hidden}', 'int64')
    lay = describe(ta.with_host_sizes(x, lens))
    code = ta._lib.MAX if op == 'cummax' else ta._lib.MIN
    v, i = O.launch_cumextreme(lay, x, code, False, (20,))
    v2, none = O.launch_cumextreme(lay, x, code, False, (20,), want_indices=False)
    none2, i2 = O.launch_cumextreme(lay, x, code, False, (20,), want_values=False)
    assert none is None and none2 is None and torch.equal(v, v2) and torch.equal(i, i2)


# ------------------------------------------------------------------ bit for bit
IDENT = [((), F32), ((8,), BF16), ((64,), F32), ((125,), F32), ((3,), F64)]
IDENT_IDS = [f'{h}-{d}'.replace('torch.', '') for h, d in IDENT]


def outputs(op, z, reverse):
    v, i = apply(op, z, reverse)
    return [v] + ([] if i is None else [i])


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('op', OPS)
def test_casts_commute_bit_for_bit(op, hidden, dtype, reverse):
    x = U.draw((int(CROSSING.sum()),) + hidden, dtype, 21).to(DEV)
    if op != 'logcumsumexp':
        x = (x * 1.5).round()                            # a handful of distinct values: most tokens tie
    c = ta.with_host_sizes(x, CROSSING)
    p = c.pack()
    for k, yc in enumerate(outputs(op, c, reverse)):
        fn = lambda z: outputs(op, z, reverse)[k]          # noqa: E731
        assert same_bits(fn(ta.C(x, CROSSING.to(DEV))).data, yc.data), 'C with and without a host mirror of the lengths'
        assert same_bits(fn(c.left(0)).data, yc.left(0).data), 'C <-> L'
        assert same_bits(fn(c.right(0)).data, yc.right(0).data), 'C <-> R'
        assert same_bits(fn(p).data, yc.pack().data), 'C <-> P'
        assert same_bits(fn(p).cat().data, yc.data), 'P -> C'
        assert same_bits(fn(c.left(0)).cat().data, yc.data) and same_bits(fn(c.right(0)).cat().data, yc.data)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('op', OPS)
def test_reverse_is_the_forward_scan_of_the_reversed_sequences(op, hidden, dtype, kind):
    x = U.draw((int(CROSSING.sum()),) + hidden, dtype, 22).to(DEV)
    if op != 'logcumsumexp':
        x = (x * 1.5).round()
    z = build(kind, x, CROSSING)
    v, i = apply(op, z, True)
    mv, mi = apply(op, z.rev(), False)
    assert same_bits(mv.rev().data, v.data)
    if i is not None:                                    # len - 1 - the mirrored positions (padding rows stay 0)
        lens = build(kind, torch.ones_like(x, dtype=I64), CROSSING).cumsum(reverse=True).cummax().values
        assert torch.equal(torch.where(lens.data > 0, lens.data - 1 - mi.rev().data, 0), i.data)


LONG = LT(8197, 8192 + 2048, 5)


def launch(op, lay, x, reverse, hidden, cut=True):
    if op == 'logcumsumexp':
        return [O.launch_logcumsumexp(lay, x, reverse, hidden, cut=cut)]
    return list(O.launch_cumextreme(lay, x, ta._lib.MAX if op == 'cummax' else ta._lib.MIN, reverse, hidden, cut=cut))


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('op', OPS)
def test_cut_form_equals_the_uncut_one(op, hidden, dtype, reverse):
    x = U.draw((int(LONG.sum()),) + hidden, dtype, 23).to(DEV)
    c = ta.with_host_sizes(x, LONG)
    lay = describe(c)
    wide = x[0].numel() * x.element_size() > 16
    with dispatch_trace() as tr:
        y_cut = launch(op, lay, x, reverse, hidden)
    assert bool(tr.matching(f'{KERNEL[op]}_rows_kernel cut=1 phase=partial')) == wide, tr.records
    assert bool(tr.matching(f'{KERNEL[op]}_rows_kernel cut=1 phase=finish')) == wide, tr.records
    with dispatch_trace() as tr:
        y_plain = launch(op, lay, x, reverse, hidden, cut=False)
    assert not tr.matching(f'{KERNEL[op]}_rows_kernel cut=1') and len(tr.records) == 1, tr.records
    for a, b in zip(y_cut, y_plain):
        assert same_bits(a, b)
    for a, b in zip(outputs(op, c.pack(), reverse), y_cut):
        assert same_bits(a.cat().data, b)
    # the backward kernels, cut against uncut, on the forward's own outputs
    cot = U.draw(tuple(x.shape), dtype, 24).to(DEV)
    if op == 'logcumsumexp':
        a = O.launch_logcumsumexp_backward(lay, cot, x, y_cut[0], reverse, hidden)
        b = O.launch_logcumsumexp_backward(lay, cot, x, y_cut[0], reverse, hidden, cut=False)
    else:
        a = O.launch_cumextreme_backward(lay, cot, y_cut[1], reverse, hidden)
        b = O.launch_cumextreme_backward(lay, cot, y_cut[1], reverse, hidden, cut=False)
    assert same_bits(a, b)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('op', OPS)
def test_unaligned_bases_give_the_same_bits(op, hidden, dtype):
    x = U.draw((int(CROSSING.sum()),) + hidden, dtype, 24).to(DEV)
    lay = describe(ta.with_host_sizes(x, CROSSING))
    for reverse in (False, True):
        for a, b in zip(launch(op, lay, shifted(x), reverse, hidden), launch(op, lay, x, reverse, hidden)):
            assert same_bits(a, b)


# ------------------------------------------------------------------ special values
def specials(dtype, hidden):
    """Sequences of ties (4 distinct values), of +-0.0, with NaN runs, of -inf only, and ordinary ones."""
    lens = LT(7, 40, 33, 64, 70, 2100, 1, 0, 129)
    n = int(lens.sum())
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 4, (n,) + hidden, generator=gen).to(dtype)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    x[off[0]:off[0] + 7] = torch.tensor([1, 1, 0, NAN, 2, NAN, 3], dtype=dtype).reshape((7,) + (1,) * len(hidden))
    x[off[1]:off[2]] = torch.where(torch.rand((40,) + hidden, generator=gen) > 0.5, 0.0, -0.0).to(dtype)
    x[off[2]:off[3]] = -INF
    x[off[3] + 10:off[3] + 13] = NAN
    x[off[3] + 40] = NAN
    x[off[4]:off[4] + 3] = -INF
    x[off[4] + 50] = INF
    x[off[5] + 2050] = NAN
    return x.to(DEV), lens


@pytest.mark.parametrize('hidden,dtype', [((), F32), ((8,), BF16), ((20,), F16), ((64,), F32), ((3,), F64)], ids=str)
@pytest.mark.parametrize('op', ('cummax', 'cummin'))
def test_cumextreme_special_values_are_exact_in_every_layout(op, hidden, dtype):
    x, lens = specials(dtype, hidden)
    for kind in 'CLPR':
        for reverse in (False, True):
            v, i, _ = run(op, kind, x, lens, reverse)
            check(op, x, lens, reverse, v, i, None, None, f'specials {kind} rev={int(reverse)}', 'specials')


@pytest.mark.parametrize('op', ('cummax', 'cummin'))
def test_int64_extremes(op):
    lo, hi = torch.iinfo(I64).min, torch.iinfo(I64).max
    x = torch.tensor([lo, lo, 5, hi, hi, 0, hi, lo, lo, -1, lo], dtype=I64).to(DEV)
    lens = LT(7, 0, 4)
    for kind in 'CLPR':
        for reverse in (False, True):
            v, i, _ = run(op, kind, x, lens, reverse)
            check(op, x, lens, reverse, v, i, None, None, f'int64 extremes {kind}', 'int64')


@pytest.mark.parametrize('hidden,dtype', [((), F32), ((8,), BF16), ((64,), F32), ((3,), F64)], ids=str)
def test_logcumsumexp_special_values(hidden, dtype):
    """Leading -inf runs, an interior +inf, a NaN that poisons only its own tail; -inf tokens get zero gradient and
    their neighbours finite ones.  (Short sequences: the derived bound counts every position, -inf ones too.)"""
    lens = LT(12, 40, 33, 64, 5, 0, 20)
    n = int(lens.sum())
    x = U.draw((n,) + hidden, dtype, 6)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    x[off[0]:off[0] + 5] = -INF                       # a leading run of -inf ...
    x[off[0] + 8] = -INF                              # ... and an interior one
    x[off[1] + 20] = INF
    x[off[2] + 7] = NAN
    x[off[3]:off[4]] = -INF                           # a sequence of -inf only
    x = x.to(DEV)
    cot = U.draw((n,) + hidden, dtype, 7).to(DEV)
    for kind in 'CLPR':
        for reverse in (False, True):
            v, _, g = run('logcumsumexp', kind, x, lens, reverse, cot)
            U.check_lse(v, x, lens, reverse, f'lse specials {kind}', 'lse_specials')
            vc = v.cpu()
            s0 = vc[off[0]:off[1]]
            assert bool((s0[:5] == -INF).all()) if not reverse else bool(torch.isfinite(s0).all())
            assert bool((vc[off[3]:off[4]] == -INF).all()) and not bool(torch.isnan(vc[off[4]:]).any())
            gc = g.cpu()
            g0 = gc[off[0]:off[1]]
            minus = (x.cpu()[off[0]:off[1]] == -INF)
            assert bool((g0[minus] == 0).all()) and bool(torch.isfinite(g0).all()), '-inf tokens: zero gradient'
            assert bool((g0[~minus] != 0).any())
            assert bool((gc[off[3]:off[4]] == 0).all())
            fin = torch.ones(n, dtype=torch.bool)
            fin[off[1]:off[3]] = False                 # (the sequences with +inf / NaN: checked through the forward)
            U.check_lse_grad(g[fin], x[fin], v[fin], cot[fin], LT(12, 0, 0, 64, 5, 0, 20), reverse, f'lse specials {kind}',
                             'lse_specials')


def test_logcumsumexp_offsets_do_not_overflow():
    lens = RAGGED
    base = U.draw((int(lens.sum()), 8), F32, 8)
    for shift in (80.0, -80.0):
        x = (base + shift).to(DEV)
        for reverse in (False, True):
            v, _, g = run('logcumsumexp', 'C', x, lens, reverse, torch.ones_like(x))
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all())
            U.check_lse(v, x, lens, reverse, f'offset {shift}', 'lse_offset')
            U.check_lse_grad(g, x, v, torch.ones_like(x), lens, reverse, f'offset {shift}', 'lse_offset')


# ------------------------------------------------------------------ padding, empties, layouts and widths
@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden', [(), (8,), (64,)], ids=str)
@pytest.mark.parametrize('op', OPS)
def test_padding_rows_are_zero_whatever_the_input_holds(op, kind, hidden):
    lens = torch.cat([LT(0, 50, 3), torch.randint(0, 50, (20,), generator=torch.Generator().manual_seed(7))])
    x = U.draw((int(lens.sum()),) + hidden, F32, 41).to(DEV)
    cot = U.draw(tuple(x.shape), F32, 42).to(DEV)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    T = z.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)
    live = live.reshape(live.shape + (1,) * len(hidden)).expand_as(z.data)
    noise = torch.full_like(z.data, NAN)
    for reverse in (False, True):
        clean = [o.data for o in outputs(op, z, reverse)]
        dirty_in = torch.where(live, z.data, noise).requires_grad_(True)
        outs = outputs(op, z._replace(data=dirty_in), reverse)
        for o, cl in zip(outs, clean):
            assert same_bits(o.data.detach(), cl) and bool((o.data.detach()[~live] == 0).all())
        outs[0].data.backward(torch.where(live, cz.data, noise))
        ref_in = z.data.clone().requires_grad_(True)
        outputs(op, z._replace(data=ref_in), reverse)[0].data.backward(cz.data)
        assert same_bits(dirty_in.grad, ref_in.grad) and bool((dirty_in.grad[~live] == 0).all())


@pytest.mark.parametrize('op', OPS)
def test_empty_inputs(op):
    for lens in (LT(0, 0, 0), LT()):
        for hidden in ((), (64,)):
            x = torch.zeros((0,) + hidden, device=DEV)
            zs = [ta.C(x, lens.to(DEV)), ta.with_host_sizes(x, lens)]
            if lens.numel():
                zs += [ta.L(torch.zeros((3, 0) + hidden, device=DEV), lens.to(DEV)),
                       ta.R(torch.zeros((3, 0) + hidden, device=DEV), lens.to(DEV))]
            for z in zs:
                for reverse in (False, True):
                    for o in outputs(op, z, reverse):
                        assert o.data.numel() == 0
    fn = {'cummax': ta.segment_cummax, 'cummin': ta.segment_cummin, 'logcumsumexp': ta.segment_logcumsumexp}[op]
    out = fn(torch.zeros(0, 4, device=DEV), LT(0, 0).to(DEV))
    assert (out if op == 'logcumsumexp' else out[0]).shape == (0, 4)


@pytest.mark.parametrize('op', OPS)
def test_sliced_input_and_segment_form(op):
    lens = torch.randint(1, 40, (30,), generator=torch.Generator().manual_seed(10))
    n = int(lens.sum())
    big = U.draw((n, 24), F32, 71).to(DEV).requires_grad_(True)
    cot = U.draw((n, 12), F32, 72).to(DEV)
    x = big[:, ::2]
    assert not x.is_contiguous()
    fn = {'cummax': ta.segment_cummax, 'cummin': ta.segment_cummin, 'logcumsumexp': ta.segment_logcumsumexp}[op]
    out = fn(x, lens.to(DEV), reverse=True)
    y = out if op == 'logcumsumexp' else out[0]
    y.backward(cot)
    v, i, g = run(op, 'C', x.detach().contiguous(), lens, True, cot)
    assert same_bits(y.detach(), v) and (i is None or torch.equal(out[1], i))
    assert same_bits(big.grad[:, ::2], g) and bool((big.grad[:, 1::2] == 0).all())


@pytest.mark.parametrize('hidden,dtype', [((3,), BF16), ((12,), F16), ((125,), F32), ((125,), F64), ((500,), BF16)],
                         ids=('6B', '24B', '500B', '1000B', '1000B_bf16'))
@pytest.mark.parametrize('op', OPS)
def test_odd_row_widths(op, hidden, dtype):
    lens = LT(0, 1, 33, 70, 129)
    x = U.draw((int(lens.sum()),) + hidden, dtype, 51).to(DEV)
    cot = U.draw(tuple(x.shape), dtype, 52).to(DEV)
    for kind in 'CP':
        v, i, g = run(op, kind, x, lens, False, cot)
        check(op, x, lens, False, v, i, g, cot, f'odd width {hidden} {kind}', 'odd_widths')


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('hidden', [(), (3,), (20,)], ids=str)
@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('op', OPS)
def test_gradcheck(op, kind, hidden):
    lens = LT(5, 0, 1, 9, 34)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((int(lens.sum()),) + hidden, generator=gen, dtype=F64)
    if op != 'logcumsumexp':                           # distinct values: the derivative exists
        x = torch.randperm(x.numel(), generator=gen).double().reshape(x.shape) / 7
    z = build(kind, x.to(DEV), lens)
    for reverse in (False, True):
        fn = lambda d: apply(op, rewrap(z, d), reverse)[0].data          # noqa: E731
        leaf = z.data.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(fn, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
        if op != 'logcumsumexp':
            assert torch.autograd.gradgradcheck(fn, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


def test_logcumsumexp_create_graph_raises():
    x = torch.randn(9, 4, device=DEV, requires_grad=True)
    y = ta.segment_logcumsumexp(x, LT(4, 5).to(DEV))
    with pytest.raises(ta.RuaError, match='second derivatives'):
        torch.autograd.grad(y.sum(), x, create_graph=True)


def test_what_the_graph_saves():
    x = torch.randn(9, 4, device=DEV, requires_grad=True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        v, i = ta.segment_cummax(x, LT(4, 5).to(DEV))
    assert len(saved) == 1 and saved[0].dtype == I64 and saved[0].data_ptr() == i.data_ptr()
    assert v.requires_grad and not i.requires_grad
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = ta.segment_logcumsumexp(x, LT(4, 5).to(DEV))
    assert sorted(t.data_ptr() for t in saved) == sorted((x.data_ptr(), y.data_ptr()))
    # int64 payloads pass through without a graph
    v, i = ta.segment_cummin(torch.arange(9, device=DEV), LT(4, 5).to(DEV))
    assert v.grad_fn is None and i.grad_fn is None


def test_second_order_backward_launches_are_the_library_kernels():
    x = torch.randn(40, 8, device=DEV, requires_grad=True)
    lens = LT(7, 33).to(DEV)
    with dispatch_trace() as tr:
        v, _ = ta.segment_cummax(x, lens)
        g, = torch.autograd.grad(v.square().sum(), x, create_graph=True)
        g.sum().backward()
    names = tr.kernels
    # forward, its backward (the run sum), the backward of that (the per-element gather) and the run sum again
    assert names == ['seg_cumextreme_rows_kernel', 'seg_cumextreme_bwd_rows_kernel', 'seg_reorder_elems_kernel',
                     'seg_cumextreme_bwd_rows_kernel'], names


# ------------------------------------------------------------------ one use: ListMLE
def test_listmle_against_the_padded_torch_spelling():
    """Plackett-Luce: sum over the list of logcumsumexp(sorted scores, from the end) - sorted scores, lists ordered by
    relevance.  The padded float64 torch spelling masks the padding by hand."""
    lens = LT(1, 5, 17, 64, 100, 0, 33)
    n = int(lens.sum())
    scores = U.draw((n,), F64, 81).to(DEV).requires_grad_(True)
    relevance = U.draw((n,), F64, 82).to(DEV)
    c = ta.with_host_sizes(scores, lens)
    order = ta.with_host_sizes(relevance, lens).sort(descending=True).indices
    s = c.reorder(order)
    loss = (s.logcumsumexp(reverse=True).data - s.data).sum()
    loss.backward()
    want_in = scores.detach().cpu().clone().requires_grad_(True)
    total = 0
    for sp, rp in zip(U.pieces(want_in, lens), U.pieces(relevance.cpu(), lens)):
        if sp.numel():
            o = sp[torch.sort(rp, descending=True, stable=True)[1]]
            total = total + (torch.logcumsumexp(o.flip(0), 0).flip(0) - o).sum()
    total.backward()
    assert math.isclose(loss.item(), total.item(), rel_tol=1e-12, abs_tol=1e-12)
    assert torch.allclose(scores.grad.cpu(), want_in.grad, rtol=1e-11, atol=1e-12)
