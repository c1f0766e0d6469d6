"""Per-sequence cumsum on the GPU: the reference's stored results (tests/golden/r8_cumsum.npz) in all four containers,
every kernel form against a float64 per-sequence torch.cumsum, the bit-for-bit identities (casts commute, reverse is
the mirrored forward scan, cut == uncut, unaligned == aligned, -0.0), aliasing, padding, special values, gradients.

Bounds (none of them comes from what the kernels give):
  fp32 / fp64   |got - want| <= 1e-5 * sum_{s<=t} |x_s|  (the suffix sum for `reverse`; the corresponding sums of |cot|
                for gradients) — the project's bound for sums (tests/test_gpu_golden.py).  The scan adds at most
                3 + 3 + 64 + (blocks) terms in a chain, each rounding once: below 80 * 2^-24 = 4.8e-6 of that sum for
                the longest sequences used here, and the stored reference is within 5e-6 (tests/test_cumsum_surface.py).
  bf16 / f16    the same plus one unit in the last place of the payload dtype at the wanted value: the output is rounded
                once from an fp32 value that may straddle a rounding boundary.
  int64         exact.
"""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from test_cumsum_surface import load_cases, seg_cumsum
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64, I64 = torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int64
DT = {'fp32': F32, 'fp64': F64, 'bf16': BF16, 'fp16': F16, 'int64': I64}
BAR = 1e-5
REPORT = {}


# ------------------------------------------------------------------ helpers
def ulp_at(v64, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at the float64 values `v64`."""
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)
    _, e = torch.frexp(v64.abs().clamp_min(2.0 ** -140))            # |v| = m * 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(v64), (e - 1 - bits).clamp_min(lowest))


def check(got, want, absum64, what, key):
    """`got` (payload dtype, any device) against `want`, with `absum64` the float64 sum of |terms| behind each element."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, what
    if got.numel() == 0:
        return
    if got.dtype == I64:
        assert torch.equal(got, want), f'{what}: int64 result differs'
        return
    w = want.double()
    bound = BAR * absum64
    if got.dtype in (BF16, F16):
        bound = bound + ulp_at(w, got.dtype)
    ratio = ((got.double() - w).abs() / bound.clamp_min(1e-300)).max().item()
    k = f'{key} {got.dtype}'
    REPORT[k] = max(REPORT.get(k, 0.0), ratio)
    print(f'{what}: worst error / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: {ratio:.3f} x the bound'


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


def run(kind, x, lens_host, reverse, cot=None, host_sizes=True):
    """(y in cat form, grad in cat form or None) of the operator applied in layout `kind`."""
    z = build(kind, x, lens_host, host_sizes)
    if cot is None:
        out = z.cumsum(reverse=reverse)
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == x.dtype
        return out.cat().data, None
    leaf = z.data.detach().clone().requires_grad_(True)
    out = rewrap(z, leaf).cumsum(reverse=reverse)
    out.data.backward(build(kind, cot, lens_host, host_sizes).data)          # the cotangent in the same layout
    return out.cat().data.detach(), rewrap(z, leaf.grad).cat().data


def check_both(x, cot, lens, reverse, y, g, what, key, want_y=None, want_g=None):
    """y and g (cat form) against float64 — or against the given wanted values — at the bound of the docstring."""
    xc, lens = x.cpu(), lens.cpu()
    if x.dtype == I64:
        check(y, seg_cumsum(xc, lens, reverse) if want_y is None else want_y, None, what, key)
        return
    x64 = xc.double()
    check(y, seg_cumsum(x64, lens, reverse) if want_y is None else want_y, seg_cumsum(x64.abs(), lens, reverse),
          what + ' fwd', key)
    if g is not None:
        c64 = cot.cpu().double()
        check(g, seg_cumsum(c64, lens, not reverse) if want_g is None else want_g,
              seg_cumsum(c64.abs(), lens, not reverse), what + ' grad', key)


def payload(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == I64:
        return torch.randint(-1000, 1001, shape, generator=g, dtype=I64).to(DEV)
    return torch.randn(shape, generator=g, dtype=F64 if dtype == F64 else F32).to(dtype).to(DEV)


def lengths(B, lo, hi, seed, empties=0):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi + 1, B)
    if empties:
        lens[rng.choice(B, empties, replace=False)] = 0
    return torch.from_numpy(lens.astype(np.int64))


def LT(*values):
    return torch.tensor(values, dtype=torch.long)


def shifted(t):
    """The same values at a base address off 16 bytes (by one element)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


# ------------------------------------------------------------------ fixtures from the reference
CASES = load_cases()


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture(name, kind):
    c = CASES[name]
    dtype, lens = DT[c['dtype']], c['lens']
    assert c['x'].dim() == (1 if c['H'] == 0 else 2)
    x = c['x'].to(dtype).to(DEV)
    cot = None if dtype == I64 else c['cot'].to(dtype).to(DEV)
    for reverse, ykey, gkey in ((False, 'y', 'gx'), (True, 'yrev', 'gxrev')):
        y, g = run(kind, x, lens, reverse, cot)
        check_both(x, cot, lens, reverse, y, g, f'{name} {kind} rev={int(reverse)}', 'fixtures', want_y=c[ykey],
                   want_g=c.get(gkey))


# ------------------------------------------------------------------ every kernel form, at the smallest shape that reaches it
RAGGED = LT(0, 1, 31, 32, 33, 129, 2100, 64)
# (id, kind, lens, hidden, dtype, shift the base?, forward record without rev=)
PATHS = [
    ('lanes_2B', 'C', RAGGED, (), BF16, False, 'seg_cumsum_lanes_kernel T=bf16 W=2 AL=1'),
    ('lanes_4B', 'P', RAGGED, (), F32, False, 'seg_cumsum_lanes_kernel T=f32 W=4 AL=1'),
    ('lanes_8B', 'C', RAGGED, (), F64, False, 'seg_cumsum_lanes_kernel T=f64 W=8 AL=1'),
    ('lanes_8B_i64', 'L', RAGGED, (), I64, False, 'seg_cumsum_lanes_kernel T=i64 W=8 AL=1 kind=1'),
    ('lanes_16B', 'C', RAGGED, (8,), BF16, False, 'seg_cumsum_lanes_kernel T=bf16 W=16 AL=1'),
    ('lanes_16B_shifted', 'C', RAGGED, (8,), BF16, True, 'seg_cumsum_lanes_kernel T=bf16 W=2 AL=0'),
    ('rows_aligned', 'C', RAGGED, (64,), F32, False, 'seg_cumsum_rows_kernel T=f32 AL=1 cut=0'),
    ('rows_aligned_R', 'R', RAGGED, (64,), F32, False, 'seg_cumsum_rows_kernel T=f32 AL=1 cut=0 kind=3'),
    ('rows_odd_width', 'C', RAGGED, (125,), F32, False, 'seg_cumsum_rows_kernel T=f32 AL=0 cut=0'),
    ('rows_shifted_base', 'C', RAGGED, (64,), F32, True, 'seg_cumsum_rows_kernel T=f32 AL=0 cut=0'),
    ('rows_P_f16', 'P', RAGGED, (24,), F16, False, 'seg_cumsum_rows_kernel T=f16 AL=1 cut=0 kind=2'),
    ('cut_partial', 'C', LT(8197, 8192 + 2048), (64,), F32, False, 'seg_cumsum_rows_kernel T=f32 AL=1 cut=1 phase=partial'),
    ('cut_finish', 'C', LT(8197, 8192 + 2048), (64,), F32, False, 'seg_cumsum_rows_kernel T=f32 AL=1 cut=1 phase=finish'),
]


@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path, reverse):
    pid, kind, lens, hidden, dtype, shift, rec = path
    n = int(lens.sum())
    x = payload((n,) + hidden, dtype, 11)
    cot = None if dtype == I64 else payload((n,) + hidden, dtype, 12)
    if shift:                                        # (a CattedSequence: the storage IS the payload)
        x = shifted(x)
    if shift:                                        # (forward only: autograd's leaf would be a fresh, aligned copy)
        cot = None
    with dispatch_trace() as tr:
        y, g = run(kind, x, lens, reverse, cot)
    assert tr.matching(f'{rec} rev={int(reverse)}'), f'{pid}: wanted {rec} rev={int(reverse)}, got {tr.records}'
    if cot is not None:                              # the backward is the same kernel in the other direction
        assert tr.matching(f'{rec} rev={int(not reverse)}'), f'{pid}: backward, got {tr.records}'
    check_both(x, cot, lens, reverse, y, g, f'{pid} rev={int(reverse)}', pid)


# ------------------------------------------------------------------ bit for bit
IDENT = [((), F32), ((8,), BF16), ((64,), F32), ((125,), F32), ((3,), F64), ((), I64)]
IDENT_IDS = [f'{h}-{d}'.replace('torch.', '') for h, d in IDENT]
CROSSING = LT(0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 5, 0, 4100)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
def test_casts_commute_bit_for_bit(hidden, dtype, reverse):
    x = payload((int(CROSSING.sum()),) + hidden, dtype, 21)
    fn = lambda z: z.cumsum(reverse=reverse)          # noqa: E731
    c = ta.with_host_sizes(x, CROSSING)
    yc = fn(c)
    assert torch.equal(fn(ta.C(x, CROSSING.to(DEV))).data, yc.data), 'C with and without a host mirror of the lengths'
    assert torch.equal(fn(c.left(0)).data, yc.left(0).data), 'C <-> L'
    assert torch.equal(fn(c.right(0)).data, yc.right(0).data), 'C <-> R'
    p, yp = c.pack(), yc.pack()
    assert torch.equal(fn(p).data, yp.data), 'C <-> P'
    assert torch.equal(fn(p).cat().data, yc.data), 'P -> C'
    assert torch.equal(fn(p.left(0)).data, fn(p).left(0).data), 'P <-> L'
    assert torch.equal(fn(p.right(0)).data, fn(c.left(0)).right(0).data), 'R <-> L'
    assert torch.equal(fn(c.left(0)).cat().data, yc.data) and torch.equal(fn(c.right(0)).cat().data, yc.data)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('kind', 'CLPR')
def test_reverse_is_the_forward_scan_of_the_reversed_sequences(hidden, dtype, kind):
    x = payload((int(CROSSING.sum()),) + hidden, dtype, 22)
    z = build(kind, x, CROSSING)
    assert torch.equal(z.rev().cumsum().rev().data, z.cumsum(reverse=True).data)
    assert torch.equal(z.rev().cumsum(reverse=True).rev().data, z.cumsum().data)


LONG = LT(8197, 8192 + 2048, 5)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
def test_cut_form_equals_the_uncut_one(hidden, dtype, reverse):
    """Few but long sequences: cut across workgroups (workspace) — the same bits as with the workspace withheld."""
    x = payload((int(LONG.sum()),) + hidden, dtype, 23)
    c = ta.with_host_sizes(x, LONG)
    lay = describe(c)
    wide = x[0].numel() * x.element_size() > 16
    with dispatch_trace() as tr:
        y_cut = O.launch_cumsum(lay, x, reverse, hidden)
    assert bool(tr.matching('seg_cumsum_rows_kernel cut=1 phase=partial')) == wide, tr.records
    assert bool(tr.matching('seg_cumsum_rows_kernel cut=1 phase=finish')) == wide, tr.records
    with dispatch_trace() as tr:
        y_plain = O.launch_cumsum(lay, x, reverse, hidden, cut=False)
    assert not tr.matching('seg_cumsum_rows_kernel cut=1') and len(tr.records) == 1, tr.records
    assert torch.equal(y_cut, y_plain)
    assert torch.equal(c.cumsum(reverse=reverse).data, y_cut)
    assert torch.equal(c.left(0).cumsum(reverse=reverse).cat().data, y_cut)      # (512 units of 128 bytes or fewer: cut too)
    assert torch.equal(c.pack().cumsum(reverse=reverse).cat().data, y_cut)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
def test_unaligned_bases_give_the_same_bits(hidden, dtype):
    x = payload((int(CROSSING.sum()),) + hidden, dtype, 24)
    lay = describe(ta.with_host_sizes(x, CROSSING))
    for reverse in (False, True):
        want = O.launch_cumsum(lay, x, reverse, hidden)
        assert torch.equal(O.launch_cumsum(lay, shifted(x), reverse, hidden), want)
        assert torch.equal(O.launch_cumsum(lay, x, reverse, hidden, out=shifted(torch.empty_like(x))), want)


@pytest.mark.parametrize('hidden,dtype', [h for h in IDENT if h[1] != I64], ids=IDENT_IDS[:-1])
def test_negative_zero_gives_the_same_bits_in_every_form(hidden, dtype):
    """Sequences of -0.0 only, of +0.0 and -0.0 mixed, and -0.0 in front of ordinary values: a carry that one form adds
    and another skips would show in the sign of a zero."""
    lens = LT(1, 33, 40, 64, 2049, 70, 8197, 8192 + 2048)
    n = int(lens.sum())
    x = payload((n,) + hidden, dtype, 25)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    x[off[0]:off[3]] = -0.0                                           # three sequences of -0.0 only
    x[off[3]:off[5]] = torch.where(x[off[3]:off[5]] > 0, 0.0, -0.0).to(dtype)     # +0.0 and -0.0 mixed
    x[off[5]:off[5] + 35] = -0.0                                      # -0.0 past the first tile, then values
    x[off[6]:off[6] + 4096] = -0.0                                    # two blocks of -0.0 in a cut sequence
    x[off[7]:] = -0.0                                               # a cut sequence of -0.0 only
    c = ta.with_host_sizes(x, lens)
    lay = describe(c)
    for reverse in (False, True):
        y = c.cumsum(reverse=reverse).data
        assert bool(torch.signbit(y[off[0]:off[3]]).all()) and bool(torch.signbit(y[off[7]:]).all()), 'sums of -0.0 are -0.0'
        assert bool((y[off[0]:off[5]] == 0).all())
        bits = y.view(torch.int16 if dtype in (BF16,) else {F32: torch.int32, F64: torch.int64}[dtype])
        for other in (O.launch_cumsum(lay, x, reverse, hidden, cut=False),
                      O.launch_cumsum(lay, shifted(x), reverse, hidden),
                      c.left(0).cumsum(reverse=reverse).cat().data, c.right(0).cumsum(reverse=reverse).cat().data,
                      c.pack().cumsum(reverse=reverse).cat().data,
                      c.rev().cumsum(reverse=not reverse).rev().data):
            assert torch.equal(other.view(bits.dtype), bits)


# ------------------------------------------------------------------ aliasing, padding, shapes
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,), (125,)], ids=str)
def test_in_place(kind, hidden):
    lens = torch.cat([lengths(30, 0, 90, 6), LT(700, 2100)])
    z = build(kind, payload((int(lens.sum()),) + hidden, F32, 31), lens)
    lay = lay_of(z)
    for reverse in (False, True):
        y = O.launch_cumsum(lay, z.data, reverse, hidden)
        buf = z.data.clone()
        assert O.launch_cumsum(lay, buf, reverse, hidden, out=buf) is buf and torch.equal(buf, y)


def test_in_place_cut():
    x = payload((int(LONG.sum()), 64), F32, 32)
    lay = describe(ta.with_host_sizes(x, LONG))
    y = O.launch_cumsum(lay, x, False, (64,))
    buf = x.clone()
    with dispatch_trace() as tr:
        O.launch_cumsum(lay, buf, False, (64,), out=buf)
    assert tr.matching('seg_cumsum_rows_kernel cut=1 phase=finish') and torch.equal(buf, y)


def test_sliced_input():
    lens = lengths(30, 1, 40, 10)
    n = int(lens.sum())
    big = payload((n, 24), F32, 71).requires_grad_(True)
    cot = payload((n, 12), F32, 72)
    x = big[:, ::2]
    assert not x.is_contiguous()
    y = ta.segment_cumsum(x, lens.to(DEV))
    y.backward(cot)
    want_y, want_g = run('C', x.detach().contiguous(), lens, False, cot)
    assert torch.equal(y.detach(), want_y)
    assert torch.equal(big.grad[:, ::2], want_g) and bool((big.grad[:, 1::2] == 0).all())
    assert torch.equal(ta.segment_cumsum(x.detach(), lens.to(DEV), reverse=True), run('C', x.detach().contiguous(), lens, True)[0])


@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden', [(), (8,), (64,)], ids=str)
def test_padding_rows_are_zero_whatever_the_input_holds(kind, hidden):
    lens = lengths(40, 0, 50, 7)
    x = payload((int(lens.sum()),) + hidden, F32, 41)
    cot = payload(x.shape, F32, 42)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    T = z.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)
    live = live.reshape(live.shape + (1,) * len(hidden)).expand_as(z.data)
    junk = torch.tensor([float('nan'), float('inf'), 1e9, float('-inf')], device=DEV)
    noise = junk[torch.arange(z.data.numel(), device=DEV) % 4].reshape(z.data.shape)
    for reverse in (False, True):
        clean = z.cumsum(reverse=reverse).data
        dirty_in = torch.where(live, z.data, noise).requires_grad_(True)
        out = z._replace(data=dirty_in).cumsum(reverse=reverse).data
        assert torch.equal(out.detach(), clean) and bool((out.detach()[~live] == 0).all())
        out.backward(torch.where(live, cz.data, noise))
        ref_in = z.data.clone().requires_grad_(True)
        z._replace(data=ref_in).cumsum(reverse=reverse).data.backward(cz.data)
        assert torch.equal(dirty_in.grad, ref_in.grad) and bool((dirty_in.grad[~live] == 0).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_empty_sequences(kind, hidden):
    lens = LT(0, 0, 5, 0, 1, 0, 0, 40, 3, 0)
    x = payload((int(lens.sum()),) + hidden, F32, 81)
    for reverse in (False, True):
        y, _ = run(kind, x, lens, reverse)
        check_both(x, None, lens, reverse, y, None, f'empties {kind}', 'empties')


@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_only_empty_sequences_and_no_sequences(hidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        x = torch.empty((0,) + hidden, device=DEV)
        c = ta.C(x, lens.to(DEV))
        padded = [ta.L(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV)),
                  ta.R(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV))] if lens.numel() else []
        for z in [c] + padded:
            assert z.cumsum().data.shape == z.data.shape and z.cumsum(reverse=True).data.shape == z.data.shape
        assert ta.segment_cumsum(x, lens.to(DEV)).shape == x.shape
        xg = x.clone().requires_grad_(True)
        ta.segment_cumsum(xg, lens.to(DEV)).sum().backward()
        assert xg.grad.shape == x.shape
    pad = torch.full((3, 4) + hidden, float('nan'), device=DEV)          # all padding: all zeros
    assert bool((ta.L(pad, torch.zeros(3, dtype=torch.long, device=DEV)).cumsum().data == 0).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (4,), (64,)], ids=str)
def test_nan_and_infinities_poison_only_what_follows_them(kind, hidden):
    inf, nan = float('inf'), float('nan')
    lens = LT(6, 3, 40, 5, 300, 4, 2100)
    x = payload((int(lens.sum()),) + hidden, F32, 91)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    col = (0,) * len(hidden)
    x[(off[0] + 2,) + col] = nan
    x[(off[1] + 1,) + col] = inf
    x[(off[3],) + col] = -inf
    x[(off[4] + 170,) + col] = nan                     # past the first tiles
    x[(off[5],) + col] = inf                           # +inf, then -inf: NaN from there on
    x[(off[5] + 2,) + col] = -inf
    x[(off[6] + 2050,) + col] = inf                    # in the second block
    for reverse in (False, True):
        y, _ = run(kind, x, lens, reverse)
        want = seg_cumsum(x.cpu().double(), lens, reverse)
        y = y.cpu()
        assert torch.equal(torch.isnan(y), torch.isnan(want)), 'NaN positions'
        assert torch.equal(torch.isinf(y), torch.isinf(want)) and torch.equal(y[torch.isinf(y)].double(), want[torch.isinf(want)])
        fin = torch.isfinite(want)
        absum = seg_cumsum(torch.where(torch.isfinite(x.cpu()), x.cpu(), torch.zeros(())).double().abs(), lens, reverse)
        assert ((y.double() - want).abs()[fin] <= BAR * absum[fin]).all()
        # the sequence that holds nothing special, and the other columns, are untouched
        assert bool(torch.isfinite(y[off[2]:off[3]]).all())
        if hidden:
            assert bool(torch.isfinite(y[..., 1:]).all())


@pytest.mark.parametrize('row_bytes', (6, 24, 500, 1000))
def test_odd_row_widths(row_bytes):
    lens = lengths(60, 0, 80, 9)
    x = payload((int(lens.sum()), row_bytes // 2), BF16, 61)
    cot = payload(x.shape, BF16, 62)
    for kind in 'CP':
        for reverse in (False, True):
            y, g = run(kind, x, lens, reverse, cot)
            check_both(x, cot, lens, reverse, y, g, f'{row_bytes}-byte rows {kind}', 'row widths')


def test_unsupported_payloads_are_refused():
    lens = torch.tensor([2, 3], device=DEV)
    with pytest.raises(ta.RuaError):
        ta.segment_cumsum(torch.arange(5, device=DEV, dtype=torch.int32), lens)
    with pytest.raises(ta.RuaError):
        ta.C(torch.ones(5, device=DEV, dtype=torch.bool), lens).cumsum()
    with pytest.raises(ta.RuaError):
        ta.C(torch.arange(5, device=DEV, dtype=torch.int32), lens).pack().cumsum(reverse=True)


@pytest.mark.parametrize('kind', 'CLPR')
def test_int64_is_exact_and_wraps(kind):
    lens = LT(4, 0, 70, 2100, 3)
    x = payload((int(lens.sum()), 3), I64, 95)
    x[:3] = 2 ** 62                                    # 3 * 2^62 passes 2^63: the sum wraps
    x[80:90] = -2 ** 62
    pieces = [np.cumsum(p.numpy().astype(np.uint64), axis=0).astype(np.int64) for p in torch.split(x.cpu(), lens.tolist())]
    want = torch.from_numpy(np.concatenate(pieces))
    y, _ = run(kind, x, lens, False)
    assert torch.equal(y.cpu(), want) and int(want[2, 0]) < 0
    assert torch.equal(y.cpu(), seg_cumsum(x.cpu(), lens, False))
    assert torch.equal(run(kind, x, lens, True)[0].cpu(), seg_cumsum(x.cpu(), lens, True))
    assert not ta.C(x, lens.to(DEV)).cumsum().data.requires_grad


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('hidden', [(), (3,), (20,)], ids=str)
def test_gradcheck_and_gradgradcheck(kind, hidden, reverse):
    lens = LT(3, 1, 0, 5, 2)
    z = build(kind, payload((int(lens.sum()),) + hidden, F64, 101), lens)

    def f(data):
        return rewrap(z, data).cumsum(reverse=reverse).data
    leaf = z.data.detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradgradcheck(f, (leaf,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_autograd_saves_nothing_and_the_backward_is_the_library_kernel():
    lens = lengths(20, 1, 30, 12)
    x = payload((int(lens.sum()), 16), F32, 121).requires_grad_(True)
    y = ta.with_host_sizes(x, lens).cumsum().data
    assert y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 0
    cot = payload(y.shape, F32, 122)
    with dispatch_trace() as tr, torch.autograd.profiler.profile() as prof:
        y.backward(cot)
    assert [r.split(' ', 1)[0] for r in tr.records] == ['seg_cumsum_rows_kernel'], tr.records
    assert tr.matching('seg_cumsum_rows_kernel rev=1')
    names = {e.key for e in prof.key_averages()}
    assert not any('cumsum' in n and n.startswith('aten::') for n in names), names
    check(x.grad, seg_cumsum(cot.cpu().double(), lens, True), seg_cumsum(cot.cpu().double().abs(), lens, True),
          'backward of the forward scan', 'backward')
    # and of the reverse scan: the forward one
    x2 = x.detach().clone().requires_grad_(True)
    y2 = ta.with_host_sizes(x2, lens).pack().cumsum(reverse=True).data
    with dispatch_trace() as tr:
        y2.sum().backward()
    assert tr.matching('seg_cumsum_rows_kernel rev=0 kind=2'), tr.records


def test_zz_report():
    """The worst achieved error / bound of this run, per group and dtype (for the GPU test log)."""
    for key in sorted(REPORT):
        print(f'cumsum report: {key}: {REPORT[key]:.3e} of the bound')
