"""Per-sequence var_mean / standardize on the GPU: the reference's stored results (tests/golden/r11_standardize.npz),
every kernel form against float64, layout commutation bit for bit, aliasing, padding, special values, offsets,
gradients.  The bounds are those of tests/norm_util.py (none comes from what the kernels give).

Gradients of standardize are held to the float64 evaluation of the backward formula on the y and rstd the forward
produced (BAR norm); against the fixtures' independent gradient the bound is (BAR + 4 u rho) norm, plus for a 16-bit payload what the rounding of the saved y can move
(norm_util.std_grad_rounded_y).  The saved rstd is held to float64 directly.  Gradients of var_mean
are held to the float64 formula on the mean the forward produced, at the issue's bound; against the fixtures' independent
gradient the mean's own rounding (4 u |mu|) enters the deviation's term (norm_util.vm_grad_bound)."""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
import norm_util as U
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
REPORT = {}


def note(key, value):
    REPORT[key] = max(REPORT.get(key, 0.0), float(value))


# ------------------------------------------------------------------ helpers
def ratio(got, want, bound, what, key):
    """max |got - want| / bound where the expected value is finite; NaN masks must agree; bound 0 means exact."""
    if got.numel() == 0:
        return
    fin = torch.isfinite(bound)
    assert torch.equal(torch.isnan(got) | ~fin, ~fin), f'{what}: NaN positions'
    if not bool(fin.any()):
        return
    e, b = (got.double() - want.double()).abs()[fin], bound[fin]
    assert bool((e[b == 0] == 0).all()), f'{what}: must be exact where the bound is 0'
    r = float((e / b.clamp_min(1e-300)).max())
    print(f'{what}: {r:.3f} of its bound')
    note(key, r)
    assert r <= 1.0, f'{what}: at {r:.2f} x its bound'


def build(kind, x, lens_host, host_sizes=True):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def run_std(kind, x, lens, c, eps, cot=None, host_sizes=True):
    """(y, rstd, grad) in cat form of standardize applied in layout `kind` (rstd / grad None without a cotangent)."""
    z = build(kind, x, lens, host_sizes)
    if cot is None:
        out = z.standardize(eps=eps, correction=c)
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == x.dtype
        return out.cat().data, None, None
    leaf = z.data.detach().clone().requires_grad_(True)
    out = rewrap(z, leaf).standardize(eps, c)
    rstd = out.data.grad_fn.saved_tensors[1].detach()
    out.data.backward(build(kind, cot, lens, host_sizes).data)
    return out.cat().data.detach(), rstd, rewrap(z, leaf.grad).cat().data


def run_vm(kind, x, lens, c, cv=None, cm=None, host_sizes=True):
    """(var, mean, saved mean, grad in cat form) of var_mean applied in layout `kind`."""
    z = build(kind, x, lens, host_sizes)
    if cv is None:
        var, mean = z.var_mean(correction=c)
        assert var.shape == mean.shape == (lens.numel(),) + tuple(x.shape[1:]) and var.dtype == mean.dtype == x.dtype
        return var, mean, None, None
    leaf = z.data.detach().clone().requires_grad_(True)
    var, mean = rewrap(z, leaf).var_mean(c)
    kept = var.grad_fn.saved_tensors[1].detach()
    torch.autograd.backward([var, mean], [cv, cm])
    return var.detach(), mean.detach(), kept, rewrap(z, leaf.grad).cat().data


def check_all(kind, x, lens, c, eps, cot, cv, cm, what, key, host_sizes=True, ref=None):
    """standardize forward / backward and var_mean forward / backward of one input against float64 (and, with `ref`, a
    fixture's independent results)."""
    dt = x.dtype
    ex = U.Exact(x, lens)
    mu = ex.mean.abs()[ex.ids]
    y, rstd, g = run_std(kind, x, lens, c, eps, cot, host_sizes)
    ratio(y, ex.y(c, eps), ex.y_bound(c, eps, dt), f'{what} y', f'{key} {dt} y')
    ratio(rstd, ex.rstd(c, eps), ex.rstd_bound(c, eps, dt), f'{what} rstd', f'{key} {dt} rstd')
    want, norm = U.std_grad(y, rstd, cot, lens, c)
    ratio(g, want, U.std_grad_bound(want, norm, dt), f'{what} grad y', f'{key} {dt} grad y')
    var, mean, kept, gx = run_vm(kind, x, lens, c, cv, cm, host_sizes)
    ratio(var, ex.var(c), ex.var_bound(c, dt), f'{what} var', f'{key} {dt} var')
    ratio(mean, ex.mean, ex.mean_bound(dt), f'{what} mean', f'{key} {dt} mean')
    want, absdev, kv, km = U.vm_grad(x, kept, cv, cm, lens, c)
    ratio(gx, want, U.vm_grad_bound(want, absdev, kv, km, mu, dt), f'{what} grad var_mean', f'{key} {dt} grad vm')
    if ref is not None:
        ry, rgy, rvar, rmean, rgvm = (t.to(DEV) if t is not None else None for t in ref)
        rho = (ex.mean.abs() / torch.sqrt(ex.var(0) + eps))[ex.ids]
        ratio(y, ry, ex.y_bound(c, eps, dt), f'{what} y vs reference', f'{key} {dt} y')
        if rgy is not None:
            # (bf16 / f16: the backward consumes the ROUNDED y it saved; norm_util.std_grad_rounded_y is what that
            # rounding can move the gradient by, derived from the number format)
            w64, n64 = U.std_grad(ex.y(c, eps), ex.rstd(c, eps), cot, lens, c)
            bound = U.std_grad_bound(w64, n64, dt, rho) + U.std_grad_rounded_y(ex.y(c, eps), ex.rstd(c, eps), cot, lens, c, dt)
            ratio(g, rgy, bound, f'{what} grad y vs reference', f'{key} {dt} grad y ref')
        ratio(var, rvar, ex.var_bound(c, dt), f'{what} var vs reference', f'{key} {dt} var')
        ratio(mean, rmean, ex.mean_bound(dt), f'{what} mean vs reference', f'{key} {dt} mean')
        w64, absdev, kv, km = U.vm_grad(x, ex.mean, cv, cm, lens, c)
        ratio(gx, rgvm, U.vm_grad_bound(w64, absdev, kv, km, mu, dt, independent=True), f'{what} grad var_mean vs reference',
              f'{key} {dt} grad vm ref')


def randn(shape, dtype, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    work = F64 if dtype == F64 else F32
    return (offset + torch.randn(shape, generator=g, dtype=work) * scale).to(dtype).to(DEV)


def lengths(B, lo, hi, seed, empties=0):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi + 1, B)
    if empties:
        lens[rng.choice(B, empties, replace=False)] = 0
    return torch.from_numpy(lens.astype(np.int64))


# ------------------------------------------------------------------ fixtures from the reference
CASES = U.load_cases()


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture(name, kind):
    c = CASES[name]
    dt, lens = U.DTYPES[c['dtype']], c['lens']
    x, cot, cv, cm = (c[k].to(dt).to(DEV) for k in ('x', 'cot', 'cv', 'cm'))
    if int(lens.sum()) == 0:
        return
    for key, (cr, eps) in U.COMBOS.items():
        ref = (c['y' + key], c.get('gy' + key), c[f'var{cr}'], c['mean'], c[f'gvm{cr}'])
        check_all(kind, x, lens, cr, eps, cot, cv, cm, f'{name} {kind} c={cr} eps={eps}', 'fixtures', ref=ref)


# ------------------------------------------------------------------ every kernel form
# (id, kind, host sizes?, lens, hidden, dtypes, forward record, backward record) — the shapes of test_gpu_softmax._paths
def _paths():
    many_short = lengths(300, 1, 64, 1, empties=5)
    few_long = torch.tensor([300, 5000, 2049, 777, 2048], dtype=torch.long)
    mid = torch.cat([lengths(160, 8, 512, 2), torch.tensor([512])])
    longish = lengths(12, 1500, 3000, 3)
    outlier = torch.cat([lengths(64, 1, 64, 4), torch.tensor([3000])])
    cut = torch.tensor([9000, 20000], dtype=torch.long)
    return [
        ('lanes_1d', 'C', True, many_short, (), (F32, BF16, F16, F64), 'lanes', 'lanes', ''),
        ('lanes_16B_P', 'P', True, many_short, (8,), (BF16,), 'lanes', 'lanes', 'W=16'),
        ('lanes_long_blocks', 'C', True, few_long, (2,), (F32, BF16), 'lanes', 'lanes', ''),
        ('lanes_left', 'L', True, many_short, (), (F32,), 'lanes', 'lanes', 'kind=1'),
        ('resident_C', 'C', True, mid, (64,), (F32, BF16, F16, F64), 'resident AL=1 cut=0 cap=480',
         'resident AL=1 cut=0 cap=224', ''),
        ('resident_P', 'P', True, mid, (128,), (BF16,), 'resident AL=1 kind=2', 'resident AL=1 kind=2', ''),
        ('resident_R_odd', 'R', True, many_short, (125,), (F32, BF16), 'resident AL=0 cap=64', 'resident AL=0 cap=64', ''),
        ('resident_outlier_dev_lens', 'C', False, outlier, (64,), (F32,), 'resident AL=1 cap=480', 'resident AL=1 cap=224', ''),
        ('stream', 'C', True, longish, (64,), (F32, BF16), 'stream AL=1 cut=0 cap=0', 'stream AL=1 cut=0 cap=0', ''),
        ('stream_left', 'L', True, longish, (32,), (F32,), 'stream cut=0 kind=1', 'stream cut=0 kind=1', ''),
        ('cut', 'C', True, cut, (64,), (F32, BF16), 'stream cut=1 phase=finish', 'stream cut=1 phase=finish', ''),
        ('cut_P_odd', 'P', True, cut, (33,), (F32,), 'stream AL=0 cut=1 phase=partial', 'stream AL=0 cut=1 phase=partial', ''),
    ]


PATHS = _paths()


def _rec(prefix, spec, extra, op=None):
    form, *pairs = spec.split()
    return ' '.join([f'{prefix}_{form}_kernel'] + pairs + ([extra] if extra else []) + ([f'op={op}'] if op else []))


@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path):
    pid, kind, host_sizes, lens, hidden, dtypes, fwd, bwd, extra = path
    n, B = int(lens.sum()), lens.numel()
    for dtype in dtypes:
        x = randn((n,) + hidden, dtype, 11, scale=2.0, offset=3.0)
        cot, cv, cm = randn((n,) + hidden, dtype, 12), randn((B,) + hidden, dtype, 13), randn((B,) + hidden, dtype, 14)
        with dispatch_trace() as tr:
            check_all(kind, x, lens, 0, 1e-5, cot, cv, cm, f'{pid} {dtype}', pid, host_sizes)
        want = [_rec('seg_norm', fwd, extra, 'standardize'), _rec('seg_norm_backward', bwd, extra),
                _rec('seg_norm', fwd.replace('resident', 'stream').replace('cap=480', 'cap=0').replace('cap=64', 'cap=0'),
                     extra, 'var_mean'),
                'seg_var_mean_backward_kernel']
        for rec in want:
            assert tr.matching(rec), f'{pid}: wanted {rec}, got {tr.records}'


# ------------------------------------------------------------------ layout and aliasing
COMMUTE = [((), F32), ((8,), BF16), ((64,), F32), ((125,), F32), ((64,), BF16), ((3,), F64)]


@pytest.mark.parametrize('hidden,dtype', COMMUTE, ids=[f'{h}-{d}'.replace('torch.', '') for h, d in COMMUTE])
def test_casts_commute_bit_for_bit(hidden, dtype):
    """Lengths on both sides of every threshold (32, 256, the resident caps 224 and 480, 2 048, 4 500) and some empty
    sequences: every form, one fold order."""
    lens = torch.cat([lengths(40, 0, 70, 5), torch.tensor([224, 225, 256, 257, 480, 481, 600, 2048, 2049, 4500, 0, 1])])
    x = randn((int(lens.sum()),) + hidden, dtype, 21, scale=3.0, offset=5.0)
    c = ta.with_host_sizes(x, lens)
    c_dev = ta.C(x, lens.to(DEV))                     # lengths on the device only: another resident / stream decision
    p = c.pack()
    yc = c.standardize()
    assert torch.equal(c_dev.standardize().data, yc.data), 'C with and without a host mirror of the lengths'
    assert torch.equal(c.left(0).standardize().data, yc.left(0).data), 'C <-> L'
    assert torch.equal(c.right(0).standardize().data, yc.right(0).data), 'C <-> R'
    assert torch.equal(p.standardize().data, yc.pack().data), 'C <-> P'
    assert torch.equal(p.standardize().cat().data, yc.data), 'P -> C'
    assert torch.equal(p.left(0).standardize().data, p.standardize().left(0).data), 'P <-> L'
    assert torch.equal(c.left(0).standardize().cat().data, yc.data) and torch.equal(c.right(0).standardize().cat().data, yc.data)
    var, mean = c.var_mean()
    for z, what in ((c_dev, 'C dev'), (c.left(0), 'L'), (c.right(0), 'R'), (p, 'P')):
        v2, m2 = z.var_mean()
        assert torch.equal(v2.view(torch.uint8), var.view(torch.uint8)), f'var {what}'          # (bits: NaN == NaN)
        assert torch.equal(m2.view(torch.uint8), mean.view(torch.uint8)), f'mean {what}'
    # the backward's sums follow the same order
    cot = randn(x.shape, dtype, 22)
    cc = ta.with_host_sizes(cot, lens)
    rstd = O.launch_standardize(describe(c), x, hidden, want_rstd=True)[1]
    gc = O.launch_standardize_backward(describe(c), yc.data, rstd, cot, hidden)
    for z, zy, zg in ((c.left(0), yc.left(0), cc.left(0)), (c.right(0), yc.right(0), cc.right(0)), (p, yc.pack(), cc.pack())):
        lay = M.lay_pack(z) if isinstance(z, ta.P) else describe(z)
        g = O.launch_standardize_backward(lay, zy.data, rstd, zg.data, hidden)
        assert torch.equal(rewrap(z, g).cat().data, gc), type(z).__name__


def test_cut_form_equals_the_uncut_one():
    """Few but long sequences: cut across workgroups through the workspace — the same bits as the same ABI call with
    ws = NULL, forward and backward."""
    lens = torch.tensor([9000, 20000, 5], dtype=torch.long)
    H = 32
    x = randn((int(lens.sum()), H), F32, 23, scale=3.0, offset=7.0)
    c = ta.with_host_sizes(x, lens)
    lay, lib, stream = describe(c), ta.load_library(), torch.cuda.current_stream().cuda_stream
    with dispatch_trace() as tr:
        y_cut, rstd_cut = O.launch_standardize(lay, x, (H,), want_rstd=True)
        var_cut, mean_cut = O.launch_var_mean(lay, x, (H,))
    assert tr.matching('seg_norm_stream_kernel cut=1 phase=partial op=standardize')
    assert tr.matching('seg_norm_stream_kernel cut=1 phase=finish op=var_mean')
    y, rstd = torch.empty_like(x), torch.empty_like(rstd_cut)
    var, mean = torch.empty_like(var_cut), torch.empty_like(mean_cut)
    with dispatch_trace() as tr:
        assert lib.rua_segment_standardize(lay.ref(), x.data_ptr(), y.data_ptr(), rstd.data_ptr(), H, 0, 0, 1e-5, None, stream) == 0
        assert lib.rua_segment_var_mean(lay.ref(), x.data_ptr(), var.data_ptr(), mean.data_ptr(), H, 0, 1, None, stream) == 0
    assert len(tr.matching('seg_norm_stream_kernel cut=0')) == 2
    assert torch.equal(y_cut, y) and torch.equal(rstd_cut, rstd) and torch.equal(var_cut, var) and torch.equal(mean_cut, mean)
    assert torch.equal(c.left(0).standardize().cat().data, y_cut)
    cot = randn(x.shape, F32, 24)
    with dispatch_trace() as tr:
        g_cut = O.launch_standardize_backward(lay, y_cut, rstd_cut, cot, (H,))
    assert tr.matching('seg_norm_backward_stream_kernel cut=1 phase=finish')
    g = torch.empty_like(x)
    assert lib.rua_segment_standardize_backward(lay.ref(), y.data_ptr(), rstd.data_ptr(), cot.data_ptr(), g.data_ptr(), H, 0, 0,
                                                None, stream) == 0
    assert torch.equal(g_cut, g)


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,), (125,)], ids=str)
def test_in_place(kind, hidden):
    lens = torch.cat([lengths(30, 0, 90, 6), torch.tensor([700])])
    x = randn((int(lens.sum()),) + hidden, F32, 31, offset=2.0)
    cot = randn(x.shape, F32, 32)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    lay = M.lay_pack(z) if kind == 'P' else describe(z)
    y, rstd = O.launch_standardize(lay, z.data, hidden, want_rstd=True)
    buf = z.data.clone()
    assert O.launch_standardize(lay, buf, hidden, out=buf)[0] is buf and torch.equal(buf, y)
    g = O.launch_standardize_backward(lay, y, rstd, cz.data, hidden)
    gbuf = cz.data.clone()
    O.launch_standardize_backward(lay, y, rstd, gbuf, hidden, out=gbuf)
    assert torch.equal(gbuf, g)
    with pytest.raises(ta.RuaError):                   # y must not alias grad_in
        O.launch_standardize_backward(lay, y, rstd, cz.data, hidden, out=y)


@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden', [(), (8,), (64,)], ids=str)
def test_padding_rows_are_zero_whatever_the_input_holds(kind, hidden):
    lens = lengths(40, 0, 50, 7)
    x = randn((int(lens.sum()),) + hidden, F32, 41, offset=1.0)
    cot = randn(x.shape, F32, 42)
    cv, cm = randn((40,) + hidden, F32, 43), randn((40,) + hidden, F32, 44)
    z, cz = build(kind, x, lens), build(kind, cot, lens)
    T = z.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)
    live = live.reshape(live.shape + (1,) * len(hidden)).expand_as(z.data)
    junk = torch.tensor([float('nan'), float('inf'), 1e9, float('-inf')], device=DEV)
    noise = junk[torch.arange(z.data.numel(), device=DEV) % 4].reshape(z.data.shape)

    def both(data, cotangent):
        leaf = data.clone().requires_grad_(True)
        out = z._replace(data=leaf).standardize().data
        out.backward(cotangent)
        leaf2 = data.clone().requires_grad_(True)
        var, mean = z._replace(data=leaf2).var_mean(0)     # (correction 0: the singletons' gradient is finite)
        torch.autograd.backward([var, mean], [cv, cm])
        return out.detach(), leaf.grad, var.detach(), mean.detach(), leaf2.grad
    clean = both(z.data, cz.data)
    dirty = both(torch.where(live, z.data, noise), torch.where(live, cz.data, noise))
    for a, b in zip(clean, dirty):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for t in (dirty[0], dirty[1], dirty[4]):           # y and the two gradients: exactly 0 on padding, finite elsewhere
        assert bool((t[~live] == 0).all()) and bool(torch.isfinite(t).all())


@pytest.mark.parametrize('dtype', (F32, BF16))
@pytest.mark.parametrize('hidden', [(), (2,), (8,), (64,)], ids=str)
def test_unaligned_bases_give_the_same_bits(hidden, dtype):
    """The payload shifted by one element (2 bytes in bf16, 4 in fp32 — torch cannot hold an fp32 tensor off 4 bytes)."""
    lens = torch.cat([lengths(50, 0, 70, 8), torch.tensor([600])])
    n = int(lens.sum())
    x = randn((n,) + hidden, dtype, 51, offset=1.0)
    cot = randn(x.shape, dtype, 52)
    lay = describe(ta.with_host_sizes(x, lens))
    want_y, rstd = O.launch_standardize(lay, x, hidden, want_rstd=True)
    want_g = O.launch_standardize_backward(lay, want_y, rstd, cot, hidden)
    want_v, want_m = O.launch_var_mean(lay, x, hidden)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
        flat[1:] = t.reshape(-1)
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    xs, cs = shifted(x), shifted(cot)
    y = O.launch_standardize(lay, xs, hidden, out=shifted(torch.empty_like(x)))[0]
    assert torch.equal(y, want_y)
    g = O.launch_standardize_backward(lay, shifted(y), rstd, cs, hidden, out=shifted(torch.empty_like(x)))
    assert torch.equal(g, want_g)
    v, m = O.launch_var_mean(lay, xs, hidden)
    assert torch.equal(v.view(torch.uint8), want_v.view(torch.uint8)) and torch.equal(m.view(torch.uint8), want_m.view(torch.uint8))


@pytest.mark.parametrize('row_bytes', (2, 4, 6, 8, 24, 500, 1000))
def test_row_widths(row_bytes):
    lens = lengths(60, 0, 80, 9)
    H = row_bytes // 2
    x = randn((int(lens.sum()), H), BF16, 61, scale=2.0, offset=1.0)
    cot, cv, cm = randn(x.shape, BF16, 62), randn((60, H), BF16, 63), randn((60, H), BF16, 64)
    for kind in 'CP':
        check_all(kind, x, lens, 0, 1e-5, cot, cv, cm, f'{row_bytes}-byte rows {kind}', 'row widths')


def test_sliced_input():
    lens = lengths(30, 1, 40, 10)
    n = int(lens.sum())
    big = randn((n, 24), F32, 71).requires_grad_(True)
    cot = randn((n, 12), F32, 72)
    x = big[:, ::2]
    assert not x.is_contiguous()
    y = ta.segment_standardize(x, lens.to(DEV))
    y.backward(cot)
    want_y, _, want_g = run_std('C', x.detach().contiguous(), lens, 0, 1e-5, cot)
    assert torch.equal(y.detach(), want_y)
    assert torch.equal(big.grad[:, ::2], want_g) and bool((big.grad[:, 1::2] == 0).all())
    big.grad = None
    cv, cm = randn((30, 12), F32, 73), randn((30, 12), F32, 74)
    var, mean = ta.segment_var_mean(x, lens.to(DEV))
    torch.autograd.backward([var, mean], [cv, cm])
    v2, m2, _, g2 = run_vm('C', x.detach().contiguous(), lens, 1, cv, cm)
    def bits(t):                                       # (singletons with correction 1 are NaN: compare the bits)
        return t.detach().contiguous().view(torch.uint8)
    assert torch.equal(bits(var), bits(v2)) and torch.equal(bits(mean), bits(m2)) and torch.equal(bits(big.grad[:, ::2]), bits(g2))
    assert torch.equal(bits(ta.segment_var(x.detach(), lens.to(DEV))), bits(v2))
    assert bool(torch.isnan(var[lens.to(DEV) == 1]).all()) and bool(torch.isfinite(var[lens.to(DEV) > 1]).all())


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_empty_sequences_singletons_and_constant_columns(kind, hidden):
    lens = torch.tensor([0, 0, 5, 0, 1, 0, 0, 40, 3, 1], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F32, 81, offset=4.0)
    off = torch.cumsum(lens, 0) - lens
    x[int(off[7]):int(off[7]) + 40] = 1234.5678              # a constant sequence
    ex = U.Exact(x, lens)
    empty, single = (lens == 0).to(DEV), (lens == 1).to(DEV)
    for c in (0, 1):
        var, mean, _, _ = run_vm(kind, x, lens, c)
        ratio(var, ex.var(c), ex.var_bound(c, F32), f'empties {kind} var c={c}', 'special')
        ratio(mean, ex.mean, ex.mean_bound(F32), f'empties {kind} mean', 'special')
        assert bool(torch.isnan(var[empty]).all()) and bool(torch.isnan(mean[empty]).all())
        assert bool((var[7] == 0).all()) and bool((mean[7] == x[int(off[7])]).all()), 'a constant column: var == 0 exactly'
        assert bool(torch.isnan(var[single]).all()) if c == 1 else bool((var[single] == 0).all())
        y, _, _ = run_std(kind, x, lens, c, 1e-5)
        ratio(y, ex.y(c, 1e-5), ex.y_bound(c, 1e-5, F32), f'empties {kind} y c={c}', 'special')
        rows = torch.repeat_interleave(single, lens.to(DEV))
        assert bool(torch.isnan(y[rows]).all()) if c == 1 else bool((y[rows] == 0).all())
        assert bool((y[int(off[7]):int(off[7]) + 40] == 0).all())


@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_only_empty_sequences_and_no_sequences(hidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        x = torch.empty((0,) + hidden, device=DEV)
        B = lens.numel()
        c = ta.C(x, lens.to(DEV))
        padded = [ta.L(torch.empty((B, 0) + hidden, device=DEV), lens.to(DEV)),
                  ta.R(torch.empty((B, 0) + hidden, device=DEV), lens.to(DEV))] if B else []
        for z in [c] + padded:
            assert z.standardize().data.shape == z.data.shape
            var, mean = z.var_mean()
            assert var.shape == mean.shape == (B,) + hidden and bool(torch.isnan(var).all()) and bool(torch.isnan(mean).all())
            assert z.var().shape == (B,) + hidden
        xg = x.clone().requires_grad_(True)
        ta.segment_standardize(xg, lens.to(DEV)).sum().backward()
        assert xg.grad.shape == x.shape
    pad = torch.full((3, 4) + hidden, float('nan'), device=DEV)          # all padding: all zeros
    z = ta.L(pad, torch.zeros(3, dtype=torch.long, device=DEV))
    assert bool((z.standardize().data == 0).all()) and bool(torch.isnan(z.var_mean()[0]).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (4,), (64,)], ids=str)
def test_nan_and_infinities_stay_in_their_sequence_and_column(kind, hidden):
    inf, nan = float('inf'), float('nan')
    lens = torch.tensor([6, 3, 40, 5, 300, 4, 7], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F32, 91, offset=2.0)
    off = torch.cumsum(lens, 0) - lens
    col = (0,) * len(hidden)
    x[(int(off[0]) + 2,) + col] = nan
    x[(int(off[1]) + 1,) + col] = inf
    x[(int(off[4]) + 17,) + col] = -inf
    x[(int(off[5]),) + col] = inf
    x[(int(off[5]) + 3,) + col] = -inf
    poisoned = torch.zeros((7,) + hidden, dtype=torch.bool, device=DEV)
    for b in (0, 1, 4, 5):
        poisoned[(b,) + col] = True
    clean_x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    ex = U.Exact(clean_x, lens)
    var, mean, _, _ = run_vm(kind, x, lens, 1)
    y, _, _ = run_std(kind, x, lens, 0, 1e-5)
    assert torch.equal(torch.isnan(var), poisoned) and torch.equal(~torch.isfinite(mean), poisoned)
    assert torch.equal(torch.isnan(y), poisoned[ex.ids])
    ok = ~poisoned
    assert bool(((var.double() - ex.var(1)).abs()[ok] <= ex.var_bound(1, F32)[ok]).all())
    assert bool(((mean.double() - ex.mean).abs()[ok] <= ex.mean_bound(F32)[ok]).all())
    rows = ok[ex.ids]
    assert bool(((y.double() - ex.y(0, 1e-5)).abs()[rows] <= ex.y_bound(0, 1e-5, F32)[rows]).all())


def test_integer_payloads_and_bad_arguments_are_refused():
    lens = torch.tensor([2, 3], device=DEV)
    with pytest.raises(ta.RuaError):
        ta.segment_standardize(torch.arange(5, device=DEV), lens)
    with pytest.raises(ta.RuaError):
        ta.C(torch.arange(5, device=DEV, dtype=torch.int32), lens).var_mean()
    x = torch.randn(5, device=DEV)
    with pytest.raises(ta.RuaError):
        ta.segment_standardize(x, lens, eps=-1.0)
    with pytest.raises(ta.RuaError):
        ta.segment_var(x, lens, correction=-1)


# ------------------------------------------------------------------ offsets
@pytest.mark.parametrize('offset,scale', [(10.0, 0.1), (1000.0, 0.1), (1000.0, 1.0)])
def test_offsets(offset, scale):
    """x = offset + scale * randn in fp32: the fused fold stays inside the bounds; the naive E[x^2] - E[x]^2 evaluated in
    fp32 on the same data is outside them at (1000, 0.1) — asserted, so the case is known to discriminate."""
    lens = torch.tensor([5, 33, 513, 2049, 5000], dtype=torch.long)
    x = randn((int(lens.sum()), 4), F32, 141, scale=scale, offset=offset)
    ex = U.Exact(x, lens)
    for kind in 'CP':
        for c in (0, 1):
            var, mean, _, _ = run_vm(kind, x, lens, c)
            ratio(var, ex.var(c), ex.var_bound(c, F32), f'offset {offset} scale {scale} {kind} var', f'offsets ({offset:g}, {scale:g})')
            ratio(mean, ex.mean, ex.mean_bound(F32), f'offset {offset} scale {scale} {kind} mean', f'offsets ({offset:g}, {scale:g})')
            for eps in (1e-5, 0.0):
                y, _, _ = run_std(kind, x, lens, c, eps)
                ratio(y, ex.y(c, eps), ex.y_bound(c, eps, F32), f'offset {offset} scale {scale} {kind} y', f'offsets ({offset:g}, {scale:g})')
    ids, B = ex.ids, 5
    n32 = lens.to(DEV).float()[:, None]
    naive = U.seg_sum(x * x, ids, B) / n32 - (U.seg_sum(x, ids, B) / n32) ** 2          # fp32 throughout
    excess = float(((naive.double() - ex.var(0)).abs() / ex.var_bound(0, F32)).max())
    print(f'naive E[x^2] - E[x]^2 in fp32: {excess:.1f} x the var bound')
    if (offset, scale) == (1000.0, 0.1):
        assert excess > 1.0, 'the naive formula is inside the bound: this case does not discriminate'


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('kind', 'CP')
@pytest.mark.parametrize('hidden', [(), (3,), (20,)], ids=str)
def test_gradcheck_and_gradgradcheck(kind, hidden):
    lens = torch.tensor([3, 1, 0, 5, 2], dtype=torch.long)
    x = randn((int(lens.sum()),) + hidden, F64, 101, offset=1.0)
    z = build(kind, x, lens)
    live = (lens > 0).to(DEV)

    def std(data):
        return rewrap(z, data).standardize(1e-5, 0).data

    def vm(data):                                      # correction 0 (singletons); the empty sequence's NaN row is dropped
        var, mean = rewrap(z, data).var_mean(0)
        return var[live], mean[live]
    for f in (std, vm):
        leaf = z.data.detach().clone().requires_grad_(True)
        assert torch.autograd.gradcheck(f, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-5)
        assert torch.autograd.gradgradcheck(f, (leaf,), eps=1e-6, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize('kind', 'LR')
def test_second_order_with_poisoned_padding(kind):
    lens = torch.tensor([3, 2, 0, 5], dtype=torch.long)
    x = randn((int(lens.sum()), 3), F64, 111)
    z = build(kind, x, lens)
    live = build(kind, torch.ones_like(x), lens).data != 0
    leaf = torch.where(live, z.data, torch.full_like(z.data, 1e9)).requires_grad_(True)
    out = z._replace(data=leaf).standardize().data
    cot = torch.where(live, randn(out.shape, F64, 112), torch.full_like(out, float('inf')))
    g, = torch.autograd.grad(out, leaf, cot, create_graph=True)
    assert bool(torch.isfinite(g).all()) and bool((g[~live] == 0).all())
    gg, = torch.autograd.grad((g * g).sum(), leaf)
    assert bool(torch.isfinite(gg).all()) and bool((gg[~live] == 0).all())
    nonempty = (lens > 0).to(DEV)
    leaf2 = torch.where(live, z.data, torch.full_like(z.data, 1e9)).requires_grad_(True)
    var, mean = z._replace(data=leaf2).var_mean(0)
    g, = torch.autograd.grad((var[nonempty] * var[nonempty]).sum() + mean[nonempty].sum(), leaf2, create_graph=True)
    assert bool(torch.isfinite(g).all()) and bool((g[~live] == 0).all())
    gg, = torch.autograd.grad((g * g).sum(), leaf2)
    assert bool(torch.isfinite(gg).all()) and bool((gg[~live] == 0).all())


def test_autograd_saves_only_the_output_and_rstd():
    lens = lengths(20, 1, 30, 12)
    x = randn((int(lens.sum()), 16), F32, 121).requires_grad_(True)
    y = ta.with_host_sizes(x, lens).standardize().data
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == y.data_ptr() and tuple(saved[1].shape) == (20, 16)
    var, mean = ta.with_host_sizes(x, lens).var_mean()
    saved = var.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == x.data_ptr() and tuple(saved[1].shape) == (20, 16)


# ------------------------------------------------------------------ property, report
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('dtype', (F32, F64))
def test_standardized_sequences_have_mean_zero_and_variance_one(kind, dtype):
    """reduce_mean(y) ~ 0 and, with eps = 0 and correction = 0, reduce_mean(y^2) ~ 1 for sequences of >= 2 tokens.
    Every y carries an error of at most E = (BAR + 4 u rho) (1 + |y|), and its own output rounding u |y|.  The mean of n
    such errors is at most their maximum: |mean y| <= E_max, with no factor of n.  For the second moment,
    |mean(y^2) - 1| <= mean(2 |y| E + E^2) <= E_rel * mean(2 |y| + 2 y^2) + ..., and mean(y^2) = 1, mean |y| <= 1
    (Cauchy-Schwarz), so it is at most 4 E_rel with E_rel = BAR + 4 u rho.  reduce_mean adds its own rounding, of order
    u per term relative to mean |y| <= 1 (pairwise / blocked fold), far below BAR.  The factor is therefore 4 + 1 for
    both properties, whatever the length: 5 (BAR + 4 u rho)."""
    lens = torch.cat([lengths(100, 2, 300, 13), torch.tensor([3000])])
    x = randn((int(lens.sum()), 8), dtype, 131, scale=3.0, offset=6.0)
    z = build(kind, x, lens)
    bar, u = U.bar_u(dtype)
    ex = U.Exact(x, lens)
    tol = 5 * (bar + 4 * u * ex.mean.abs() / torch.sqrt(ex.var(0)))
    y = z.standardize(eps=0.0, correction=0)
    m1 = ta.reduce_mean(y).double().abs()
    m2 = (ta.reduce_mean(rewrap(y, y.data * y.data)).double() - 1).abs()
    note(f'property {dtype} mean / tol', (m1 / tol).max())
    note(f'property {dtype} second moment / tol', (m2 / tol).max())
    assert bool((m1 <= tol).all()) and bool((m2 <= tol).all())
    y5 = z.standardize()
    tol5 = 5 * (bar + 4 * u * ex.mean.abs() / torch.sqrt(ex.var(0) + 1e-5))
    assert bool((ta.reduce_mean(y5).double().abs() <= tol5).all())


def test_zz_report():
    """The worst achieved error / bound of this run, per path and dtype (for the GPU test log and DESIGN 3.2f)."""
    for key in sorted(REPORT):
        print(f'standardize report: {key}: {REPORT[key]:.3f}')
