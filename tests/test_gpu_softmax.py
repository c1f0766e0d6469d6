"""Per-sequence softmax / log_softmax on the GPU: the reference's stored results (tests/golden/r7_softmax.npz), every
kernel form against a float64 per-sequence torch.softmax, layout commutation bit for bit, aliasing, padding, special
values, gradients.

Bounds (none of them comes from what the kernels give):
  fp32 / fp64 forward   relative 1e-5 on 100 % of the elements (softmax outputs are positive: no floor);
                        log_softmax: 1e-5 * max(1, |y|)
  gradients             softmax: |d| <= 1e-5 * y * (|g| + sum|g y|);  log_softmax: 1e-5 * (|g| + exp(y) * sum|g|)
                        (the conditioning of g - sum: a relative bound cannot hold where the difference cancels)
  bf16 / f16 forward    at most 1 ulp of the payload dtype from the float64 (fixtures: the reference's fp32) result
                        rounded to that dtype: an output is rounded once from an fp32 value that is itself within
                        1e-5, far below half an ulp (2^-9, 2^-12), so it lands on one of the two neighbours
  bf16 / f16 gradients  the backward consumes the ROUNDED y: held to the float64 evaluation of the same formula on
                        that y and g, 1 ulp of the payload dtype plus the fp32 bound above
"""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from test_softmax_surface import load_cases
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT = {'fp32': F32, 'fp64': F64, 'bf16': BF16, 'fp16': F16}
BAR = 1e-5
REPORT = {}


def note(key, value):
    REPORT[key] = max(REPORT.get(key, 0.0), float(value))


# ------------------------------------------------------------------ helpers
def seg_sum(v, lens):
    """[N, *H] -> the per-sequence sum spread back over the sequence's rows (float64 torch)."""
    pieces = [p.sum(dim=0) for p in torch.split(v, lens.tolist(), dim=0)]
    if not pieces:
        return v.clone()
    return torch.repeat_interleave(torch.stack(pieces), lens.to(v.device), dim=0)


def exact(x, lens, log, cot=None):
    """float64 per-sequence torch.softmax / log_softmax of the cat-form payload (and its gradient under `cot`)."""
    x64 = x.double().clone().requires_grad_(cot is not None)
    fn = torch.log_softmax if log else torch.softmax
    pieces = [fn(p, dim=0) for p in torch.split(x64, lens.tolist(), dim=0)]
    y = torch.cat(pieces) if pieces else x64.clone()
    if cot is None:
        return y.detach(), None
    g, = torch.autograd.grad((y * cot.double()).sum(), x64)
    return y.detach(), g


def ulps(a, b):
    """Distance in representable values between two bf16 / f16 tensors (NaN positions must agree)."""
    assert a.dtype == b.dtype and a.dtype in (BF16, F16)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), 'NaN positions differ'

    def ordered(t):
        v = t.view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7fff), v)
    d = (ordered(a) - ordered(b)).abs()
    return torch.where(na, torch.zeros_like(d), d)


def check_forward(got, want64, log, what, key):
    """`got` in the payload dtype against the float64 (or reference) result."""
    if got.numel() == 0:
        return
    if got.dtype in (BF16, F16):
        d = ulps(got, want64.to(got.dtype))
        exact_share = (d == 0).double().mean().item()
        print(f'{what}: {got.dtype} exact {100 * exact_share:.1f} %, worst {int(d.max())} ulp')
        note(f'{key} {got.dtype} fwd ulp', d.max().item())
        assert int(d.max()) <= 1, f'{what}: {int(d.max())} ulp'
        return
    w = want64.double()
    err = (got.double() - w).abs() / (w.abs().clamp_min(1.0) if log else w)
    worst = err.max().item()
    print(f'{what}: worst relative error {worst:.2e}')
    note(f'{key} {got.dtype} fwd rel', worst)
    assert worst <= BAR, f'{what}: {worst:.2e}'


def grad_norm(y64, cot, lens, log):
    c = cot.double().abs()
    if log:
        return c + y64.exp() * seg_sum(c, lens)
    return y64 * (c + seg_sum(c * y64, lens))


def check_grad(got, y_used, cot, lens, log, what, key, want64=None):
    """fp32 / fp64: against `want64` (float64 autograd or the reference) at the normalised bound.  bf16 / f16: against
    the float64 formula on the rounded y the backward really consumed."""
    if got.numel() == 0:
        return
    if got.dtype in (BF16, F16):
        y64, g64 = y_used.double(), cot.double()
        if log:
            w = g64 - y64.exp() * seg_sum(g64, lens)
            norm = g64.abs() + y64.exp() * seg_sum(g64.abs(), lens)
        else:
            w = y64 * (g64 - seg_sum(g64 * y64, lens))
            norm = y64 * (g64.abs() + seg_sum((g64 * y64).abs(), lens))
        eps = 2.0 ** -7 if got.dtype == BF16 else 2.0 ** -10            # one ulp, relative (upper end of a binade)
        tiny = 2.0 ** -133 if got.dtype == BF16 else 2.0 ** -24         # ... and of the subnormals
        bound = eps * w.abs() + tiny + BAR * norm
        excess = ((got.double() - w).abs() / bound).max().item()
        note(f'{key} {got.dtype} grad / bound', excess)
        assert excess <= 1.0, f'{what}: gradient at {excess:.2f} x its bound'
        return
    y64 = y_used.double()
    err = ((got.double() - want64.double()).abs() / grad_norm(y64, cot, lens, log).clamp_min(1e-300)).max().item()
    print(f'{what}: worst normalised gradient error {err:.2e}')
    note(f'{key} {got.dtype} grad norm', err)
    assert err <= BAR, f'{what}: {err:.2e}'


def build(kind, x, lens_host, host_sizes=True):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def run(kind, x, lens_host, log, cot=None, host_sizes=True):
    """(y in cat form, grad in cat form or None) of the operator applied in layout `kind`."""
    z = build(kind, x, lens_host, host_sizes)
    if cot is None:
        out = z.log_softmax() if log else z.softmax()
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == x.dtype
        return out.cat().data, None
    leaf = z.data.detach().clone().requires_grad_(True)
    zz = rewrap(z, leaf)
    out = zz.log_softmax() if log else zz.softmax()
    cz = rewrap(z, build(kind, cot, lens_host, host_sizes).data)             # the cotangent in the same layout
    out.data.backward(cz.data)
    return out.cat().data.detach(), rewrap(z, leaf.grad).cat().data


def randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


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
    shape_ok = c['x'].dim() == (1 if c['H'] == 0 else 2)
    assert shape_ok
    x, cot = c['x'].to(dtype).to(DEV), c['cot'].to(dtype).to(DEV)
    for log, ykey, gkey in ((False, 'y', 'gx'), (True, 'ylog', 'gxlog')):
        y, g = run(kind, x, lens, log, cot)
        what = f'{name} {kind} {"log_softmax" if log else "softmax"}'
        check_forward(y, c[ykey].to(DEV), log, what, 'fixtures')
        check_grad(g, y if dtype in (BF16, F16) else c['ylog' if log else 'y'].to(DEV), cot, lens, log, what,
                   'fixtures', want64=c[gkey].to(DEV))


# ------------------------------------------------------------------ every kernel form
# (id, kind, host sizes?, lens, hidden, dtypes, forward records, backward records)
def _paths():
    many_short = lengths(300, 1, 64, 1, empties=5)
    few_long = torch.tensor([300, 5000, 2049, 777, 2048], dtype=torch.long)
    mid = torch.cat([lengths(160, 8, 512, 2), torch.tensor([512])])
    longish = lengths(12, 1500, 3000, 3)
    outlier = torch.cat([lengths(64, 1, 64, 4), torch.tensor([3000])])
    cut = torch.tensor([9000, 20000], dtype=torch.long)
    return [
        ('lanes_1d', 'C', True, many_short, (), (F32, BF16, F16, F64),
         'seg_softmax_lanes_kernel', 'seg_softmax_backward_lanes_kernel'),
        ('lanes_16B_P', 'P', True, many_short, (8,), (BF16,),
         'seg_softmax_lanes_kernel W=16', 'seg_softmax_backward_lanes_kernel W=16'),
        ('lanes_long_blocks', 'C', True, few_long, (2,), (F32, BF16),
         'seg_softmax_lanes_kernel', 'seg_softmax_backward_lanes_kernel'),
        ('lanes_left', 'L', True, many_short, (), (F32,),
         'seg_softmax_lanes_kernel kind=1', 'seg_softmax_backward_lanes_kernel kind=1'),
        ('resident_C', 'C', True, mid, (64,), (F32, BF16, F16, F64),
         'seg_softmax_resident_kernel AL=1 cut=0 cap=512', 'seg_softmax_backward_resident_kernel AL=1 cut=0 cap=256'),
        ('resident_P', 'P', True, mid, (128,), (BF16,),
         'seg_softmax_resident_kernel AL=1 kind=2', 'seg_softmax_backward_resident_kernel AL=1 kind=2'),
        ('resident_R_odd', 'R', True, many_short, (125,), (F32, BF16),
         'seg_softmax_resident_kernel AL=0 cap=64', 'seg_softmax_backward_resident_kernel AL=0 cap=64'),
        ('resident_outlier_dev_lens', 'C', False, outlier, (64,), (F32,),
         'seg_softmax_resident_kernel AL=1 cap=512', 'seg_softmax_backward_resident_kernel AL=1 cap=256'),
        ('stream', 'C', True, longish, (64,), (F32, BF16),
         'seg_softmax_stream_kernel AL=1 cut=0 cap=0', 'seg_softmax_backward_stream_kernel AL=1 cut=0 cap=0'),
        ('stream_left', 'L', True, longish, (32,), (F32,),
         'seg_softmax_stream_kernel cut=0 kind=1', 'seg_softmax_backward_stream_kernel cut=0 kind=1'),
        ('cut', 'C', True, cut, (64,), (F32, BF16),
         'seg_softmax_stream_kernel cut=1 phase=finish', 'seg_softmax_backward_stream_kernel cut=1 phase=finish'),
        ('cut_P_odd', 'P', True, cut, (33,), (F32,),
         'seg_softmax_stream_kernel AL=0 cut=1 phase=partial', 'seg_softmax_backward_stream_kernel AL=0 cut=1 phase=partial'),
    ]


PATHS = _paths()


@pytest.mark.parametrize('log', (False, True), ids=('softmax', 'log_softmax'))
@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path, log):
    pid, kind, host_sizes, lens, hidden, dtypes, fwd_rec, bwd_rec = path
    n = int(lens.sum())
    for dtype in dtypes:
        x = randn((n,) + hidden, dtype, 11, scale=2.0)
        cot = randn((n,) + hidden, dtype, 12)
        with dispatch_trace() as tr:
            y, g = run(kind, x, lens, log, cot, host_sizes)
        assert tr.matching(fwd_rec), f'{pid}: wanted {fwd_rec}, got {tr.records}'
        assert tr.matching(bwd_rec), f'{pid}: wanted {bwd_rec}, got {tr.records}'
        y64, g64 = exact(x, lens, log, cot)
        what = f'{pid} {dtype} {"log_softmax" if log else "softmax"}'
        check_forward(y, y64, log, what, pid)
        check_grad(g, y if dtype in (BF16, F16) else y64, cot, lens, log, what, pid, want64=g64)


# ------------------------------------------------------------------ layout and aliasing
COMMUTE = [((), F32), ((8,), BF16), ((64,), F32), ((125,), F32), ((64,), BF16), ((3,), F64)]


@pytest.mark.parametrize('hidden,dtype', COMMUTE, ids=[f'{h}-{d}'.replace('torch.', '') for h, d in COMMUTE])
@pytest.mark.parametrize('log', (False, True), ids=('softmax', 'log_softmax'))
def test_casts_commute_bit_for_bit(hidden, dtype, log):
    """Lengths on both sides of every threshold (32, 256, 512, 2 048) and some empty sequences: every form, one fold order."""
    lens = torch.cat([lengths(40, 0, 70, 5), torch.tensor([256, 257, 512, 513, 600, 2048, 2049, 4500, 0, 1])])
    x = randn((int(lens.sum()),) + hidden, dtype, 21, scale=3.0)
    fn = (lambda z: z.log_softmax()) if log else (lambda z: z.softmax())
    c = ta.with_host_sizes(x, lens)
    c_dev = ta.C(x, lens.to(DEV))                     # lengths on the device only: another resident / stream decision
    yc = fn(c)
    assert torch.equal(fn(c_dev).data, yc.data), 'C with and without a host mirror of the lengths'
    assert torch.equal(fn(c.left(0)).data, yc.left(0).data), 'C <-> L'
    assert torch.equal(fn(c.right(0)).data, yc.right(0).data), 'C <-> R'
    p, yp = c.pack(), yc.pack()
    assert torch.equal(fn(p).data, yp.data), 'C <-> P'
    assert torch.equal(fn(p).cat().data, yc.data), 'P -> C'
    assert torch.equal(fn(p.left(0)).data, fn(p).left(0).data), 'P <-> L'
    assert torch.equal(fn(c.left(0)).cat().data, yc.data) and torch.equal(fn(c.right(0)).cat().data, yc.data)


def test_cut_form_commutes_with_the_uncut_one():
    """Few but long sequences: cut across workgroups in C (workspace) — the same bits as every other form."""
    lens = torch.tensor([9000, 20000, 5], dtype=torch.long)
    x = randn((int(lens.sum()), 32), F32, 22, scale=3.0)
    c = ta.with_host_sizes(x, lens)
    lay = describe(c)
    with dispatch_trace() as tr:
        y_cut = c.softmax().data
    assert tr.matching('seg_softmax_stream_kernel cut=1 phase=partial')
    lib = ta.load_library()
    y_plain = torch.empty_like(x)                      # the same launch without a workspace: one workgroup per unit
    with dispatch_trace() as tr:
        assert lib.rua_segment_softmax(lay.ref(), x.data_ptr(), y_plain.data_ptr(), 32, 0, 0, None,
                                       torch.cuda.current_stream().cuda_stream) == 0
    assert tr.matching('seg_softmax_stream_kernel cut=0')
    assert torch.equal(y_cut, y_plain)
    assert torch.equal(c.left(0).softmax().cat().data, y_cut)
    cot = randn(x.shape, F32, 23)
    g_cut = O.launch_softmax_backward(lay, y_cut, cot, False, (32,))
    g_plain = torch.empty_like(x)
    assert lib.rua_segment_softmax_backward(lay.ref(), y_cut.data_ptr(), cot.data_ptr(), g_plain.data_ptr(), 32, 0, 0,
                                            None, torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(g_cut, g_plain)


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,), (125,)], ids=str)
def test_in_place(kind, hidden):
    lens = torch.cat([lengths(30, 0, 90, 6), torch.tensor([700])])
    x = randn((int(lens.sum()),) + hidden, F32, 31)
    cot = randn(x.shape, F32, 32)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    lay = M.lay_pack(z) if kind == 'P' else describe(z)
    for log in (False, True):
        y = O.launch_softmax(lay, z.data, log, hidden)
        buf = z.data.clone()
        assert O.launch_softmax(lay, buf, log, hidden, out=buf) is buf and torch.equal(buf, y)
        g = O.launch_softmax_backward(lay, y, cz.data, log, hidden)
        gbuf = cz.data.clone()
        O.launch_softmax_backward(lay, y, gbuf, log, hidden, out=gbuf)
        assert torch.equal(gbuf, g)
    with pytest.raises(ta.RuaError):                   # y must not alias grad_in
        O.launch_softmax_backward(lay, y, cz.data, False, hidden, out=y)


@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden', [(), (8,), (64,)], ids=str)
def test_padding_rows_are_zero_whatever_the_input_holds(kind, hidden):
    lens = lengths(40, 0, 50, 7)
    x = randn((int(lens.sum()),) + hidden, F32, 41)
    cot = randn(x.shape, F32, 42)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    T = z.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)
    live = live.reshape(live.shape + (1,) * len(hidden)).expand_as(z.data)
    junk = torch.tensor([float('nan'), float('inf'), 1e9, float('-inf')], device=DEV)
    noise = junk[torch.arange(z.data.numel(), device=DEV) % 4].reshape(z.data.shape)
    for log in (False, True):
        clean = (z.log_softmax() if log else z.softmax()).data
        dirty_in = torch.where(live, z.data, noise).requires_grad_(True)
        zz = z._replace(data=dirty_in)
        out = (zz.log_softmax() if log else zz.softmax()).data
        assert torch.equal(out.detach(), clean) and bool((out.detach()[~live] == 0).all())
        out.backward(torch.where(live, cz.data, noise))
        ref_in = z.data.clone().requires_grad_(True)
        zr = z._replace(data=ref_in)
        (zr.log_softmax() if log else zr.softmax()).data.backward(cz.data)
        assert torch.equal(dirty_in.grad, ref_in.grad) and bool((dirty_in.grad[~live] == 0).all())
        assert bool(torch.isfinite(dirty_in.grad).all())


@pytest.mark.parametrize('dtype', (F32, BF16))
@pytest.mark.parametrize('hidden', [(), (2,), (8,), (64,)], ids=str)
def test_unaligned_bases_give_the_same_bits(hidden, dtype):
    lens = torch.cat([lengths(50, 0, 70, 8), torch.tensor([600])])
    n = int(lens.sum())
    x = randn((n,) + hidden, dtype, 51)
    cot = randn(x.shape, dtype, 52)
    want_y, want_g = run('C', x, lens, False, cot)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
        flat[1:] = t.reshape(-1)
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    xs, cs = shifted(x), shifted(cot)
    c = ta.with_host_sizes(xs, lens)
    y = c.softmax().data
    assert torch.equal(y, want_y)
    ys = shifted(y)
    g = O.launch_softmax_backward(describe(c), ys, cs, False, hidden, out=shifted(torch.empty_like(x)))
    assert torch.equal(g, want_g)


@pytest.mark.parametrize('row_bytes', (2, 4, 6, 8, 24, 500, 1000))
def test_row_widths(row_bytes):
    lens = lengths(60, 0, 80, 9)
    x = randn((int(lens.sum()), row_bytes // 2), BF16, 61, scale=2.0)
    cot = randn(x.shape, BF16, 62)
    for kind in 'CP':
        for log in (False, True):
            y, g = run(kind, x, lens, log, cot)
            y64, _ = exact(x, lens, log)
            check_forward(y, y64, log, f'{row_bytes}-byte rows {kind}', 'row widths')
            check_grad(g, y, cot, lens, log, f'{row_bytes}-byte rows {kind}', 'row widths')


def test_sliced_input():
    lens = lengths(30, 1, 40, 10)
    n = int(lens.sum())
    big = randn((n, 24), F32, 71).requires_grad_(True)
    cot = randn((n, 12), F32, 72)
    x = big[:, ::2]
    assert not x.is_contiguous()
    y = ta.segment_softmax(x, lens.to(DEV))
    y.backward(cot)
    want_y, want_g = run('C', x.detach().contiguous(), lens, False, cot)
    assert torch.equal(y.detach(), want_y)
    assert torch.equal(big.grad[:, ::2], want_g) and bool((big.grad[:, 1::2] == 0).all())


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_empty_sequences(kind, hidden):
    lens = torch.tensor([0, 0, 5, 0, 1, 0, 0, 40, 3, 0], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F32, 81)
    for log in (False, True):
        y, _ = run(kind, x, lens, log)
        check_forward(y, exact(x, lens, log)[0], log, f'empties {kind}', 'empties')


@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_only_empty_sequences_and_no_sequences(hidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        x = torch.empty((0,) + hidden, device=DEV)
        c = ta.C(x, lens.to(DEV))
        padded = [ta.L(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV)),
                  ta.R(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV))] if lens.numel() else []
        for z in [c] + padded:
            assert z.softmax().data.shape == z.data.shape and z.log_softmax().data.shape == z.data.shape
        assert ta.segment_softmax(x, lens.to(DEV)).shape == x.shape
        xg = x.clone().requires_grad_(True)
        ta.segment_log_softmax(xg, lens.to(DEV)).sum().backward()
        assert xg.grad.shape == x.shape
    pad = torch.full((3, 4) + hidden, float('nan'), device=DEV)          # all padding: all zeros
    assert bool((ta.L(pad, torch.zeros(3, dtype=torch.long, device=DEV)).softmax().data == 0).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (4,), (64,)], ids=str)
def test_nan_and_infinities_stay_in_their_sequence_and_column(kind, hidden):
    inf, nan = float('inf'), float('nan')
    lens = torch.tensor([6, 3, 40, 5, 300, 4, 7], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F32, 91)
    off = torch.cumsum(lens, 0) - lens
    col = (0,) * len(hidden)
    x[(int(off[0]) + 2,) + col] = nan                        # a NaN
    x[(int(off[1]) + 1,) + col] = inf                        # +inf
    x[(slice(int(off[3]), int(off[3]) + 5),) + col] = -inf   # a column of -inf only
    x[(int(off[4]) + 17,) + col] = -inf                      # one -inf among finite values
    x[(int(off[5]),) + col] = inf                            # two +inf
    x[(int(off[5]) + 3,) + col] = inf
    for log in (False, True):
        y, _ = run(kind, x, lens, log)
        want, _ = exact(x, lens, log)
        assert torch.equal(torch.isnan(y), torch.isnan(want)), 'NaN positions'
        ok = ~torch.isnan(want)
        assert torch.equal(torch.isinf(y) & ok, torch.isinf(want) & ok), 'infinite positions'
        fin = torch.isfinite(want)
        err = ((y.double() - want).abs() / (want.abs().clamp_min(1.0) if log else want.clamp_min(1e-300)))[fin & (want != 0)]
        assert err.max().item() <= BAR
        assert bool((y[fin & (want == 0)] == 0).all())
        # the sequences that hold nothing special are what they are without their neighbours
        clean = exact(x[int(off[2]):int(off[2]) + 40], lens[2:3], log)[0]
        assert bool(torch.isfinite(y[int(off[2]):int(off[2]) + 40]).all())
        assert ((y[int(off[2]):int(off[2]) + 40].double() - clean).abs() <= BAR * clean.abs().clamp_min(1e-30 if not log else 1.0)).all()


def test_integer_payloads_are_refused():
    lens = torch.tensor([2, 3], device=DEV)
    with pytest.raises(ta.RuaError):
        ta.segment_softmax(torch.arange(5, device=DEV), lens)
    with pytest.raises(ta.RuaError):
        ta.C(torch.arange(5, device=DEV, dtype=torch.int32), lens).log_softmax()


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('log', (False, True), ids=('softmax', 'log_softmax'))
@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('hidden', [(), (3,), (20,)], ids=str)
def test_gradcheck_and_gradgradcheck(kind, hidden, log):
    lens = torch.tensor([3, 1, 0, 5, 2], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F64, 101)
    z = build(kind, x, lens)

    def f(data):
        out = rewrap(z, data)
        return (out.log_softmax() if log else out.softmax()).data
    leaf = z.data.detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradgradcheck(f, (leaf,), eps=1e-6, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize('kind', 'LR')
def test_second_order_with_poisoned_padding(kind):
    lens = torch.tensor([3, 1, 0, 5], dtype=torch.long)
    x = randn((int(lens.sum()), 3), F64, 111)
    z = build(kind, x, lens)
    live = build(kind, torch.ones_like(x), lens).data != 0
    for log in (False, True):
        leaf = torch.where(live, z.data, torch.full_like(z.data, 1e9)).requires_grad_(True)
        out = (z._replace(data=leaf).log_softmax() if log else z._replace(data=leaf).softmax()).data
        cot = torch.where(live, randn(out.shape, F64, 112), torch.full_like(out, float('inf')))
        g, = torch.autograd.grad(out, leaf, cot, create_graph=True)
        assert bool(torch.isfinite(g).all()) and bool((g[~live] == 0).all())
        gg, = torch.autograd.grad((g * g).sum(), leaf)
        assert bool(torch.isfinite(gg).all()) and bool((gg[~live] == 0).all())


def test_autograd_saves_only_the_output():
    lens = lengths(20, 1, 30, 12)
    x = randn((int(lens.sum()), 16), F32, 121).requires_grad_(True)
    y = ta.with_host_sizes(x, lens).softmax().data
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].data_ptr() == y.data_ptr()


# ------------------------------------------------------------------ property, report
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('dtype', (F32, F64))
def test_softmax_sums_to_one(kind, dtype):
    lens = torch.cat([lengths(100, 0, 300, 13), torch.tensor([3000])])
    x = randn((int(lens.sum()), 8), dtype, 131, scale=3.0)
    z = build(kind, x, lens)
    total = ta.reduce_sum(z.softmax())
    want = (lens > 0).to(dtype).to(DEV)[:, None].expand_as(total)
    worst = (total - want).abs().max().item()
    note(f'sum to one {dtype}', worst)
    assert worst <= BAR
    assert (ta.reduce_logsumexp(z.log_softmax())[lens.to(DEV) > 0].abs() <= BAR).all()


def test_zz_report():
    """The worst figures of this run, per path and dtype (for the GPU test log)."""
    for key in sorted(REPORT):
        print(f'softmax report: {key}: {REPORT[key]:.3e}')
