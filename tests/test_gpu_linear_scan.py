"""Per-sequence gated linear recurrence on the GPU: the reference's stored results (tests/golden/r9_linear_scan.npz) in
all four containers, every kernel form against a float64 per-sequence loop, the bit-for-bit identities (casts commute,
reverse is the mirrored forward scan, cut == uncut, unaligned == aligned, gate 1 == cumsum, gate 0 restarts, scalar ==
filled tensor), an exact test, the ignored gate, NaN containment, padding, aliasing, degenerate shapes, gradients.

The bound is the one of tests/test_linear_scan_surface.py (its docstring counts K): with M_t the recurrence in float64
on (|a|, |x|),
    forward    |got - want64| <= BAR * M_t,   BAR = 231 * 2^-24 = 1.38e-5   (float64 payloads: the same BAR)
    grad_x     the same against the reversed recurrence of (|a|, |cot|)   (Mdx)
    grad_gate  2 * BAR * Mdx_t * Mh_(t-1)
plus one unit in the last place of the payload dtype at the wanted value for bf16 / f16 (the output is rounded once).
The backward's input is the SAVED OUTPUT h, which a bf16 / f16 payload holds rounded to that dtype (the payload is not
saved, so nothing more exact exists).  The wanted grad_gate of those dtypes is therefore the float64 dx times the h
that was saved — the forward's own output, held to its own bound above — not times the unrounded float64 h, which the
backward never sees: against that one the rounding of h alone (up to one ulp of the product) plus the rounding of
grad_gate (half an ulp) measured 1.207 x the bound on mid.h250.bf16.  fp32 / fp64 keep the float64 h: the factor 2
covers the error of h there.
Fixtures are held to the float64 loop AND sit within the bar of the reference's stored fp32 results."""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from test_linear_scan_surface import BAR, grads64, load_cases, scales64, scan64, want64
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT = {'fp32': F32, 'fp64': F64, 'bf16': BF16, 'fp16': F16}
REPORT = {}


# ------------------------------------------------------------------ helpers
def ulp_at(v64, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at the float64 values `v64`."""
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)
    _, e = torch.frexp(v64.abs().clamp_min(2.0 ** -140))            # |v| = m * 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(v64), (e - 1 - bits).clamp_min(lowest))


def check(got, want64_, scale64, what, key, factor=1.0):
    """`got` (payload dtype, any device) against the float64 numpy `want64_` at factor * BAR * scale64 (+ ulp)."""
    got = got.detach().cpu()
    w = torch.from_numpy(np.ascontiguousarray(want64_)).reshape(got.shape)
    if got.numel() == 0:
        return
    bound = factor * BAR * torch.from_numpy(np.ascontiguousarray(scale64)).reshape(got.shape)
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


def run(kind, x, a, lens_host, reverse, cot=None, host_sizes=True, gate_container=False):
    """(y, grad_x, grad_gate), each in cat form (None where not asked for), of the operator applied in layout `kind`;
    `a` a tensor in cat form or a Python float."""
    z = build(kind, x, lens_host, host_sizes)
    tensor_gate = isinstance(a, torch.Tensor)
    za = build(kind, a, lens_host, host_sizes) if tensor_gate else None
    if cot is None:
        gate = (za if gate_container else za.data) if tensor_gate else a
        out = z.linear_scan(gate, reverse=reverse)
        assert type(out) is type(z) and out.data.shape == z.data.shape and out.data.dtype == x.dtype
        return out.cat().data, None, None
    leaf = z.data.detach().clone().requires_grad_(True)
    gleaf = za.data.detach().clone().requires_grad_(True) if tensor_gate else a
    out = rewrap(z, leaf).linear_scan(rewrap(z, gleaf) if tensor_gate and gate_container else gleaf, reverse=reverse)
    out.data.backward(build(kind, cot, lens_host, host_sizes).data)          # the cotangent in the same layout
    ga = rewrap(z, gleaf.grad).cat().data if tensor_gate else None
    return out.cat().data.detach(), rewrap(z, leaf.grad).cat().data, ga


def saved_h64(y, want_h64):
    """The h that grad_gate's reference multiplies with (the module docstring): the saved output for bf16 / f16."""
    return y.detach().cpu().double().numpy().reshape(want_h64.shape) if y.dtype in (BF16, F16) else want_h64


def check_all(x, a, cot, lens, reverse, y, gx, ga, what, key):
    """y, gx, ga (cat form) against the float64 loop at the bound of the docstring."""
    x64 = x.detach().cpu().double().numpy()
    a64 = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else float(a)
    c64 = cot.cpu().double().numpy() if cot is not None else np.zeros_like(x64)
    want = scan64(x64, a64, lens, reverse)
    Mh, Mdx, Mda = scales64(x64, a64, c64, lens, reverse)
    check(y, want, Mh, what + ' fwd', key)
    if gx is not None:
        dx, da = grads64(a64, c64, saved_h64(y, want), lens, reverse)
        check(gx, dx, Mdx, what + ' grad_x', key)
        if ga is not None:
            check(ga, da, Mda, what + ' grad_gate', key, factor=2.0)


def payload(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64 if dtype == F64 else F32).to(dtype).to(DEV)


def gates(shape, dtype, seed):
    """+-exp(0.02 * randn), about a quarter negative: nothing decays, so a lost carry shows at full size."""
    g = torch.Generator().manual_seed(seed)
    work = F64 if dtype == F64 else F32
    mag = torch.exp(0.02 * torch.randn(shape, generator=g, dtype=work))
    sign = torch.where(torch.rand(shape, generator=g, dtype=work) < 0.25, -1.0, 1.0).to(work)
    return (sign * mag).to(dtype).to(DEV)


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


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ fixtures from the reference
CASES = load_cases()


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture(name, kind):
    c = CASES[name]
    dtype, lens = DT[c['dtype']], c['lens']
    x, cot = c['x'].to(dtype).to(DEV), c['cot'].to(dtype).to(DEV)
    a = c['a'].to(dtype).to(DEV) if c['gamma'] is None else c['gamma']
    host = kind in 'CL'                    # device-only lengths for P and R, a host mirror for C and L
    for reverse, ykey, gxkey, gakey in ((False, 'y', 'gx', 'ga'), (True, 'yrev', 'gxrev', 'garev')):
        y, gx, ga = run(kind, x, a, lens, reverse, cot, host_sizes=host, gate_container=True)
        if x.numel() == 0:
            assert y.shape == x.shape and gx.shape == x.shape
            continue
        wy, dx, da, Mh, Mdx, Mda = want64(c, reverse)
        what = f'{name} {kind} rev={int(reverse)}'
        check(y, wy, Mh, what + ' fwd', 'fixtures')
        check(gx, dx, Mdx, what + ' grad_x', 'fixtures')
        if ga is not None:
            if dtype in (BF16, F16):
                da = grads64(c['a'].double().numpy(), c['cot'].double().numpy(), saved_h64(y, wy), lens, reverse)[1]
            check(ga, da, Mda, what + ' grad_gate', 'fixtures', factor=2.0)
        # and against the reference's own stored results: both sit within the bar of float64
        if dtype in (F32, F64):
            check(y, c[ykey].astype(np.float64), Mh, what + ' fwd vs reference', 'fixtures vs reference', factor=1.5)
            check(gx, c[gxkey].astype(np.float64), Mdx, what + ' grad_x vs reference', 'fixtures vs reference', factor=1.5)


# ------------------------------------------------------------------ every kernel form, at the smallest shape that reaches it
RAGGED = LT(0, 1, 31, 32, 33, 129, 2100, 64)
CUT = LT(8193, 8211)
# (id, kind, lens, hidden, dtype, shift the base?, record without rev= / bwd= / gate=)
PATHS = [
    ('lanes_f32_h1', 'C', RAGGED, (1,), F32, False, 'seg_linear_scan_lanes_kernel T=f32 W=4 AL=1 cut=0'),
    ('lanes_f64_h2', 'P', RAGGED, (2,), F64, False, 'seg_linear_scan_lanes_kernel T=f64 W=16 AL=1 kind=2'),
    ('lanes_bf16_h8', 'L', RAGGED, (8,), BF16, False, 'seg_linear_scan_lanes_kernel T=bf16 W=16 AL=1 kind=1'),
    ('lanes_1d', 'R', RAGGED, (), F32, False, 'seg_linear_scan_lanes_kernel T=f32 W=4 AL=1 kind=3'),
    ('lanes_f16_1d', 'C', RAGGED, (), F16, False, 'seg_linear_scan_lanes_kernel T=f16 W=2 AL=1'),
    ('rows_aligned_bf16_h64', 'C', RAGGED, (64,), BF16, False, 'seg_linear_scan_rows_kernel T=bf16 AL=1 cut=0'),
    ('rows_aligned_P', 'P', RAGGED, (64,), F32, False, 'seg_linear_scan_rows_kernel T=f32 AL=1 cut=0 kind=2'),
    ('rows_odd_f32_h5', 'C', RAGGED, (5,), F32, False, 'seg_linear_scan_rows_kernel T=f32 AL=0 cut=0'),
    ('rows_shifted_base', 'C', RAGGED, (64,), F32, True, 'seg_linear_scan_rows_kernel T=f32 AL=0 cut=0'),
    ('cut_partial', 'C', CUT, (8,), F32, False, 'seg_linear_scan_rows_kernel T=f32 AL=1 cut=1 phase=partial'),
    ('cut_finish', 'C', CUT, (8,), F32, False, 'seg_linear_scan_rows_kernel T=f32 AL=1 cut=1 phase=finish'),
]


@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path, reverse):
    pid, kind, lens, hidden, dtype, shift, rec = path
    n = int(lens.sum())
    x, a = payload((n,) + hidden, dtype, 11), gates((n,) + hidden, dtype, 13)
    cot = payload((n,) + hidden, dtype, 12)
    if shift:                                        # (a CattedSequence: the storage IS the payload; forward only:
        x, cot = shifted(x), None                    #  autograd's leaf would be a fresh, aligned copy)
    with dispatch_trace() as tr:
        y, gx, ga = run(kind, x, a, lens, reverse, cot)
    want = f'{rec} rev={int(reverse)} gate=tensor bwd=0'
    assert tr.matching(want), f'{pid}: wanted {want}, got {tr.records}'
    if cot is not None:                              # the backward scans the other way
        want = f'{rec} rev={int(not reverse)} gate=tensor bwd=1'
        assert tr.matching(want), f'{pid}: wanted {want}, got {tr.records}'
    check_all(x, a, cot, lens, reverse, y, gx, ga, f'{pid} rev={int(reverse)}', pid)
    # a scalar gate through the same form
    with dispatch_trace() as tr:
        y, gx, _ = run(kind, x, -0.96875, lens, reverse, cot)
    assert tr.matching(f'{rec} rev={int(reverse)} gate=scalar bwd=0'), tr.records
    check_all(x, -0.96875, cot, lens, reverse, y, gx, None, f'{pid} scalar rev={int(reverse)}', pid)


@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
def test_cut_form_with_and_without_workspace(reverse):
    """B=2, lengths 8 193 and 8 211, fp32 H=8: cut across workgroups with `ws`, one workgroup per unit without — the same
    bits, forward and backward, both within the bound."""
    n = int(CUT.sum())
    x, a, cot = payload((n, 8), F32, 14), gates((n, 8), F32, 15), payload((n, 8), F32, 16)
    lay = describe(ta.with_host_sizes(x, CUT))
    with dispatch_trace() as tr:
        y_cut = O.launch_linear_scan(lay, x, a, reverse, (8,))
        gx_cut, ga_cut = O.launch_linear_scan_backward(lay, cot, a, y_cut, reverse, (8,))
    assert len(tr.matching('seg_linear_scan_rows_kernel cut=1 phase=partial')) == 2, tr.records
    assert len(tr.matching('seg_linear_scan_rows_kernel cut=1 phase=finish')) == 2, tr.records
    with dispatch_trace() as tr:
        y_plain = O.launch_linear_scan(lay, x, a, reverse, (8,), cut=False)
        gx_plain, ga_plain = O.launch_linear_scan_backward(lay, cot, a, y_plain, reverse, (8,), cut=False)
    assert not tr.matching('seg_linear_scan_rows_kernel cut=1') and len(tr.records) == 2, tr.records
    assert same_bits(y_cut, y_plain) and same_bits(gx_cut, gx_plain) and same_bits(ga_cut, ga_plain)
    check_all(x, a, cot, CUT, reverse, y_cut, gx_cut, ga_cut, f'cut rev={int(reverse)}', 'cut')
    ys = O.launch_linear_scan(lay, x, 0.96875, reverse, (8,))
    assert same_bits(ys, O.launch_linear_scan(lay, x, 0.96875, reverse, (8,), cut=False))


# ------------------------------------------------------------------ bit for bit
IDENT = [((), F32), ((8,), BF16), ((64,), F32), ((5,), F32), ((3,), F64), ((24,), F16)]
IDENT_IDS = [f'{h}-{d}'.replace('torch.', '') for h, d in IDENT]
CROSSING = LT(0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 5, 0, 4100)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
def test_casts_commute_bit_for_bit(hidden, dtype, reverse):
    n = int(CROSSING.sum())
    x, a = payload((n,) + hidden, dtype, 21), gates((n,) + hidden, dtype, 26)
    c, ca = ta.with_host_sizes(x, CROSSING), ta.with_host_sizes(a, CROSSING)
    fn = lambda z, g: z.linear_scan(g, reverse=reverse)          # noqa: E731
    yc = fn(c, ca)
    assert same_bits(fn(ta.C(x, CROSSING.to(DEV)), a).data, yc.data), 'C with and without a host mirror of the lengths'
    assert same_bits(fn(c.left(0), ca.left(0)).data, yc.left(0).data), 'C <-> L'
    assert same_bits(fn(c.right(0), ca.right(0)).data, yc.right(0).data), 'C <-> R'
    p, pa = c.pack(), ca.pack()
    assert same_bits(fn(p, pa).data, yc.pack().data), 'C <-> P'
    assert same_bits(fn(p, pa).cat().data, yc.data), 'z.linear_scan(a).cat() == z.cat().linear_scan(a.cat())'
    assert same_bits(fn(c.left(0), ca.left(0)).cat().data, yc.data) and same_bits(fn(c.right(0), ca.right(0)).cat().data, yc.data)
    # a scalar gate: the same in every layout, and equal to a tensor filled with it
    for gamma in (0.5, 0.96875):
        ys = fn(c, gamma)
        assert same_bits(ys.data, fn(c, torch.full_like(x, gamma)).data), 'scalar == filled tensor'
        assert same_bits(fn(p, gamma).cat().data, ys.data) and same_bits(fn(c.left(0), gamma).cat().data, ys.data)
        assert same_bits(fn(c.right(0), gamma).cat().data, ys.data)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('kind', 'CLPR')
def test_reverse_is_the_forward_scan_of_the_reversed_sequences(hidden, dtype, kind):
    n = int(CROSSING.sum())
    z = build(kind, payload((n,) + hidden, dtype, 22), CROSSING)
    a = build(kind, gates((n,) + hidden, dtype, 27), CROSSING)
    assert same_bits(z.rev().linear_scan(a.rev()).rev().data, z.linear_scan(a, reverse=True).data)
    assert same_bits(z.rev().linear_scan(a.rev(), reverse=True).rev().data, z.linear_scan(a).data)
    assert same_bits(z.rev().linear_scan(0.96875).rev().data, z.linear_scan(0.96875, reverse=True).data)


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
def test_unaligned_bases_give_the_same_bits(hidden, dtype):
    n = int(CROSSING.sum())
    x, a = payload((n,) + hidden, dtype, 24), gates((n,) + hidden, dtype, 28)
    lay = describe(ta.with_host_sizes(x, CROSSING))
    for reverse in (False, True):
        want = O.launch_linear_scan(lay, x, a, reverse, hidden)
        assert same_bits(O.launch_linear_scan(lay, shifted(x), a, reverse, hidden), want)
        assert same_bits(O.launch_linear_scan(lay, x, shifted(a), reverse, hidden), want)
        assert same_bits(O.launch_linear_scan(lay, x, a, reverse, hidden, out=shifted(torch.empty_like(x))), want)
        cot = payload((n,) + hidden, dtype, 29)
        gx, ga = O.launch_linear_scan_backward(lay, cot, a, want, reverse, hidden)
        gx2, ga2 = O.launch_linear_scan_backward(lay, shifted(cot), shifted(a), shifted(want), reverse, hidden)
        assert same_bits(gx, gx2) and same_bits(ga, ga2)


LONG = LT(8197, 8192 + 2048, 5)
ALL_DT = [((), F32), ((8,), BF16), ((64,), F32), ((5,), F32), ((3,), F64), ((24,), F16), ((), F64), ((40,), BF16)]


@pytest.mark.parametrize('hidden,dtype', ALL_DT, ids=[f'{h}-{d}'.replace('torch.', '') for h, d in ALL_DT])
def test_a_gate_of_one_is_the_cumsum_bit_for_bit(hidden, dtype):
    lens = torch.cat([CROSSING, LONG])
    n = int(lens.sum())
    x = payload((n,) + hidden, dtype, 30)
    x[5:9] = -0.0
    one = torch.ones_like(x)
    for kind in 'CP':
        z = build(kind, x, lens)
        for reverse in (False, True):
            want = z.cumsum(reverse=reverse).data
            assert same_bits(z.linear_scan(rewrap(z, torch.ones_like(z.data)), reverse=reverse).data, want), 'tensor gate of 1'
            assert same_bits(z.linear_scan(1.0, reverse=reverse).data, want), 'scalar gate of 1'
    lay = describe(ta.with_host_sizes(x, lens))
    assert same_bits(O.launch_linear_scan(lay, x, one, False, hidden, cut=False), O.launch_cumsum(lay, x, False, hidden))


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=IDENT_IDS)
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
def test_a_gate_of_zero_restarts_the_sequence_bit_for_bit(hidden, dtype, reverse):
    """a_t == 0 exactly: h_t == x_t bitwise, while h_(t-1) is finite (0 * h is a zero, and a zero added to x_t is x_t)."""
    lens = torch.cat([CROSSING, LONG])
    n = int(lens.sum())
    x, a = payload((n,) + hidden, dtype, 33), gates((n,) + hidden, dtype, 34)
    zero = torch.rand(a.shape, device=DEV) < 0.1
    a = torch.where(zero, torch.zeros_like(a), a)
    for kind in 'CP':
        z, za, zz = build(kind, x, lens), build(kind, a, lens), build(kind, zero.to(dtype), lens)
        y = z.linear_scan(za, reverse=reverse)
        assert bool(torch.isfinite(y.data.float()).all())
        hit = zz.data != 0
        assert int(hit.sum()) > 100 and torch.equal(bits(y.data)[hit], bits(z.data)[hit])


# ------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden,dtype', [((), F32), ((8,), BF16), ((5,), F32), ((64,), F32), ((2,), F64), ((8,), F32)],
                         ids=['lanes-f32', 'lanes-bf16', 'rows-odd', 'rows-aligned', 'lanes-f64', 'cut-or-rows'])
def test_exact_arithmetic_equals_the_float64_loop_bitwise(kind, hidden, dtype):
    """Gates in {1, -1, 2, 0.5} whose running product walks inside 2^+-3 (2^+-1 for bf16), so the gate product of ANY
    span is a power of two inside 2^+-6 (2^+-2); payloads are small integers.  Every partial value of any association
    order is then an integer multiple of 2^-6 (2^-2), and while it stays below 2^17 (2^6; asserted for the results, and
    the partial sums of a span are of the same size) it has at most 24 (8) significant bits: no product and no sum
    rounds, in fp32 or in the final conversion, so every form must equal the float64 loop bitwise.  The cut form
    ((8,) f32 with two long sequences) and P included."""
    bf = dtype == BF16
    lim = 1 if bf else 3
    lens = torch.cat([LT(0, 1, 9, 33, 129), LT(40, 64) if bf else LT(2049, 8193, 8211)])
    n = int(lens.sum())
    rng = np.random.RandomState(7)
    shape = (n,) + hidden
    # the log2 of the running gate product: a walk kept inside [-lim, lim]; the sign flips freely
    step = rng.randint(-1, 2, shape)
    level = np.zeros(shape, dtype=np.int64)
    run_ = np.zeros(hidden, dtype=np.int64)
    for i in range(n):
        s_ = np.where(np.abs(run_ + step[i]) > lim, 0, step[i])
        run_ = run_ + s_
        level[i] = s_
    sign = np.where(rng.rand(*shape) < 0.25, -1.0, 1.0)
    a = torch.from_numpy(sign * np.exp2(level.astype(np.float64)))
    x = torch.from_numpy(rng.randint(-3, 4, shape).astype(np.float64))
    if bf:                                             # sparse payloads of +-1: |h| stays below 2^6
        x = torch.from_numpy(np.where(rng.rand(*shape) < 0.2, rng.randint(0, 2, shape) * 2.0 - 1.0, 0.0))      # (zeros are +0.0)
    for reverse in (False, True):
        want = scan64(x.numpy(), a.numpy(), lens, reverse)
        assert np.abs(want).max() < (2 ** 6 if bf else 2 ** 17)
        want_t = torch.from_numpy(want).to(dtype)
        assert torch.equal(want_t.double(), torch.from_numpy(want)), 'the float64 result is representable in the payload dtype'
        y, _, _ = run(kind, x.to(dtype).to(DEV), a.to(dtype).to(DEV), lens, reverse)
        assert same_bits(y.cpu(), want_t), f'{kind} {hidden} {dtype} rev={int(reverse)}'


# ------------------------------------------------------------------ the ignored gate, NaN containment
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_the_ignored_gate_changes_nothing_and_gets_a_zero_gradient(kind, hidden):
    lens = LT(6, 1, 40, 0, 2100, 33)
    n = int(lens.sum())
    x, a, cot = payload((n,) + hidden, F32, 41), gates((n,) + hidden, F32, 42), payload((n,) + hidden, F32, 43)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    for reverse in (False, True):
        where = [o + (l - 1 if reverse else 0) for o, l in zip(off, lens.tolist()) if l]
        y0, gx0, ga0 = run(kind, x, a, lens, reverse, cot)
        for junk in (float('nan'), float('inf'), -float('inf')):
            bad = a.clone()
            bad[where] = junk
            y, gx, ga = run(kind, x, bad, lens, reverse, cot)
            assert same_bits(y, y0) and same_bits(gx, gx0) and same_bits(ga, ga0)
            assert bool((ga[where] == 0).all()) and bool(torch.isfinite(ga).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (4,), (64,)], ids=str)
def test_nan_stays_in_its_sequence_and_column_and_zero_gates_do_not_resurrect(kind, hidden):
    nan = float('nan')
    lens = LT(6, 3, 40, 5, 300, 4, 2100)
    n = int(lens.sum())
    x, a = payload((n,) + hidden, F32, 91), gates((n,) + hidden, F32, 92)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    col = (0,) * len(hidden)
    x[(off[0] + 2,) + col] = nan
    a[(off[0] + 4,) + col] = 0.0                       # 0 * NaN stays NaN, as in the float64 loop
    a[(off[1] + 1,) + col] = nan                       # a NaN gate that IS used
    x[(off[4] + 170,) + col] = nan                     # past the first tiles
    a[(off[4] + 200,) + col] = 0.0
    x[(off[6] + 2050,) + col] = nan                    # in the second block
    for reverse in (False, True):
        y, _, _ = run(kind, x, a, lens, reverse)
        want = torch.from_numpy(scan64(x.cpu().double().numpy(), a.cpu().double().numpy(), lens, reverse))
        y = y.cpu()
        assert torch.equal(torch.isnan(y), torch.isnan(want)), 'NaN positions'
        assert int(torch.isnan(want).sum()) > 100
        fin = ~torch.isnan(want)
        Mh = torch.from_numpy(scan64(torch.nan_to_num(x.cpu().double()).abs().numpy(),
                                     torch.nan_to_num(a.cpu().double()).abs().numpy(), lens, reverse))
        assert bool(((y.double() - want).abs()[fin] <= BAR * Mh[fin]).all())
        assert bool(torch.isfinite(y[off[2]:off[3]]).all())          # a sequence that holds nothing special
        if hidden:
            assert bool(torch.isfinite(y[..., 1:]).all())            # the other columns


# ------------------------------------------------------------------ aliasing, padding, shapes, errors
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,), (5,)], ids=str)
def test_in_place(kind, hidden):
    lens = torch.cat([lengths(30, 0, 90, 6), LT(700, 2100)])
    n = int(lens.sum())
    z, za = build(kind, payload((n,) + hidden, F32, 31), lens), build(kind, gates((n,) + hidden, F32, 32), lens)
    lay = lay_of(z)
    for reverse in (False, True):
        for gate in (za.data, 0.5):
            y = O.launch_linear_scan(lay, z.data, gate, reverse, hidden)
            buf = z.data.clone()
            assert O.launch_linear_scan(lay, buf, gate, reverse, hidden, out=buf) is buf and same_bits(buf, y)
    with pytest.raises(ta.RuaError):                                  # the output must not be the gate
        O.launch_linear_scan(lay, z.data, za.data, False, hidden, out=za.data)


def test_in_place_cut():
    n = int(CUT.sum())
    x, a = payload((n, 8), F32, 35), gates((n, 8), F32, 36)
    lay = describe(ta.with_host_sizes(x, CUT))
    y = O.launch_linear_scan(lay, x, a, False, (8,))
    buf = x.clone()
    with dispatch_trace() as tr:
        O.launch_linear_scan(lay, buf, a, False, (8,), out=buf)
    assert tr.matching('seg_linear_scan_rows_kernel cut=1 phase=finish') and same_bits(buf, y)


@pytest.mark.parametrize('kind', 'LR')
@pytest.mark.parametrize('hidden', [(), (8,), (64,)], ids=str)
def test_padding_rows_are_zero_whatever_the_inputs_hold(kind, hidden):
    lens = lengths(40, 0, 50, 7)
    n = int(lens.sum())
    x, a, cot = payload((n,) + hidden, F32, 44), gates((n,) + hidden, F32, 45), payload((n,) + hidden, F32, 46)
    z, za, cz = build(kind, x, lens), build(kind, a, lens), build(kind, cot, lens)
    T = z.data.size(1)
    steps = torch.arange(T, device=DEV)[None, :]
    ld = lens.to(DEV)[:, None]
    live = (steps < ld) if kind == 'L' else (steps >= T - ld)
    live = live.reshape(live.shape + (1,) * len(hidden)).expand_as(z.data)
    junk = torch.tensor([float('nan'), float('inf'), 1e9, float('-inf')], device=DEV)
    noise = junk[torch.arange(z.data.numel(), device=DEV) % 4].reshape(z.data.shape)
    for reverse in (False, True):
        clean_x = z.data.clone().requires_grad_(True)
        clean_a = za.data.clone().requires_grad_(True)
        clean = z._replace(data=clean_x).linear_scan(clean_a, reverse=reverse).data
        clean.backward(cz.data)
        dirty_x = torch.where(live, z.data, noise).requires_grad_(True)
        dirty_a = torch.where(live, za.data, noise).requires_grad_(True)
        out = z._replace(data=dirty_x).linear_scan(dirty_a, reverse=reverse).data
        assert same_bits(out.detach(), clean.detach()) and bool((out.detach()[~live] == 0).all())
        out.backward(torch.where(live, cz.data, noise))
        assert same_bits(dirty_x.grad, clean_x.grad) and bool((dirty_x.grad[~live] == 0).all())
        assert same_bits(dirty_a.grad, clean_a.grad) and bool((dirty_a.grad[~live] == 0).all())


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_empty_sequences(kind, hidden):
    lens = LT(0, 0, 5, 0, 1, 0, 0, 40, 3, 0)
    n = int(lens.sum())
    x, a, cot = payload((n,) + hidden, F32, 81), gates((n,) + hidden, F32, 82), payload((n,) + hidden, F32, 83)
    for reverse in (False, True):
        y, gx, ga = run(kind, x, a, lens, reverse, cot)
        check_all(x, a, cot, lens, reverse, y, gx, ga, f'empties {kind}', 'empties')


@pytest.mark.parametrize('hidden', [(), (64,), (0,)], ids=str)
def test_only_empty_sequences_no_sequences_and_no_columns(hidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        x = torch.empty((0,) + hidden, device=DEV)
        c = ta.C(x, lens.to(DEV))
        padded = [ta.L(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV)),
                  ta.R(torch.empty((lens.numel(), 0) + hidden, device=DEV), lens.to(DEV))] if lens.numel() else []
        for z in [c] + padded:
            assert z.linear_scan(z).data.shape == z.data.shape and z.linear_scan(0.5, reverse=True).data.shape == z.data.shape
        xg, ag = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ta.segment_linear_scan(xg, ag, lens.to(DEV)).sum().backward()
        assert xg.grad.shape == x.shape and ag.grad.shape == x.shape
    lens = LT(3, 0, 2)
    wide = torch.empty((5, 0), device=DEV)                               # H = 0 with tokens
    assert ta.C(wide, lens.to(DEV)).linear_scan(wide).data.shape == (5, 0)
    pad = torch.full((3, 4) + hidden, float('nan'), device=DEV)          # all padding: all zeros
    out = ta.L(pad, torch.zeros(3, dtype=torch.long, device=DEV)).linear_scan(pad).data
    assert out.shape == pad.shape and bool((out == 0).all())


def test_mismatched_gates_and_payloads_are_refused():
    lens = torch.tensor([2, 3], device=DEV)
    x = torch.randn(5, 4, device=DEV)
    c = ta.C(x, lens)
    with dispatch_trace() as tr:
        for bad in (torch.ones(5, device=DEV), torch.ones(5, 1, device=DEV), torch.ones(4, 4, device=DEV),    # shape
                    torch.ones(5, 4, device=DEV, dtype=F64), torch.ones(5, 4, device=DEV, dtype=BF16),       # dtype
                    torch.ones(5, 4),                                                                          # device
                    c.left(0), 'gamma', None, True):
            with pytest.raises(ta.RuaError):
                c.linear_scan(bad)
            with pytest.raises(ta.RuaError):
                ta.segment_linear_scan(x, bad, lens)
        for z in (c.left(0), c.right(0)):
            with pytest.raises(ta.RuaError):
                z.linear_scan(x)                                    # a cat-form gate for a padded payload
        with pytest.raises(ta.RuaError):                            # no integer types
            ta.segment_linear_scan(torch.arange(5, device=DEV), 0.5, lens)
        with pytest.raises(ta.RuaError):
            ta.C(torch.arange(5, device=DEV), lens).linear_scan(torch.ones(5, device=DEV, dtype=torch.int64))
    assert not [r for r in tr.records if r.startswith('seg_linear_scan')], 'refused before any launch'


def test_sliced_inputs():
    lens = lengths(30, 1, 40, 10)
    n = int(lens.sum())
    big = payload((n, 24), F32, 71).requires_grad_(True)
    biga = gates((n, 24), F32, 73).requires_grad_(True)
    cot = payload((n, 12), F32, 72)
    x, a = big[:, ::2], biga[:, ::2]
    assert not x.is_contiguous()
    y = ta.segment_linear_scan(x, a, lens.to(DEV))
    y.backward(cot)
    want_y, want_gx, want_ga = run('C', x.detach().contiguous(), a.detach().contiguous(), lens, False, cot)
    assert same_bits(y.detach(), want_y)
    assert same_bits(big.grad[:, ::2], want_gx) and bool((big.grad[:, 1::2] == 0).all())
    assert same_bits(biga.grad[:, ::2], want_ga) and bool((biga.grad[:, 1::2] == 0).all())


# ------------------------------------------------------------------ gradients
@pytest.mark.parametrize('reverse', (False, True), ids=('fwd', 'rev'))
@pytest.mark.parametrize('kind', 'CLPR')
def test_gradcheck_and_gradgradcheck(kind, reverse):
    lens = LT(0, 1, 4)
    z = build(kind, payload((5, 2), F64, 101), lens)
    za = build(kind, gates((5, 2), F64, 102) * 0.7, lens)

    def f(data, gate):
        return rewrap(z, data).linear_scan(gate, reverse=reverse).data

    def fs(data):
        return rewrap(z, data).linear_scan(-0.75, reverse=reverse).data
    leaf = z.data.detach().clone().requires_grad_(True)
    gleaf = za.data.detach().clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (leaf, gleaf), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradgradcheck(f, (leaf, gleaf), eps=1e-6, atol=1e-6, rtol=1e-4)
    assert torch.autograd.gradcheck(fs, (leaf,), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradgradcheck(fs, (leaf,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_gate_only_gradient_and_no_gradient():
    lens = lengths(12, 0, 40, 3)
    n = int(lens.sum())
    x, cot = payload((n, 16), F32, 111), payload((n, 16), F32, 112)
    a = gates((n, 16), F32, 113).requires_grad_(True)
    y = ta.with_host_sizes(x, lens).linear_scan(a).data
    y.backward(cot)
    _, _, want_ga = run('C', x, a.detach(), lens, False, cot)
    assert same_bits(a.grad, want_ga)
    with torch.no_grad():
        assert not ta.with_host_sizes(x, lens).linear_scan(a).data.requires_grad
    assert not ta.with_host_sizes(x, lens).linear_scan(0.5).data.requires_grad


def test_autograd_saves_gate_and_output_and_launches_no_aten_kernel():
    """The first-order forward and backward are the library's kernels alone: one launch each, no ATen compute kernel
    (allocations aside), and the payload is not saved."""
    lens = lengths(20, 1, 30, 12)
    n = int(lens.sum())
    x = payload((n, 16), F32, 121).requires_grad_(True)
    a = gates((n, 16), F32, 123).requires_grad_(True)
    cot = payload((n, 16), F32, 122)
    lay = describe(ta.with_host_sizes(x, lens))         # (the container's metadata: built before the profile)
    allowed = {'aten::empty', 'aten::detach', 'aten::contiguous', 'aten::view', 'aten::alias', 'aten::empty_like',
               'aten::empty_strided', 'aten::as_strided', 'aten::new_empty'}

    def aten_ops(prof):
        return {e.key for e in prof.key_averages() if e.key.startswith('aten::')} - allowed
    with dispatch_trace() as tr, torch.autograd.profiler.profile() as prof:
        y = O.linear_scan(x, a, lay, False, (16,))
    assert tr.kernels == ['seg_linear_scan_rows_kernel'] and tr.matching('seg_linear_scan_rows_kernel rev=0 bwd=0'), tr.records
    assert not aten_ops(prof), f'ATen operators in the forward: {aten_ops(prof)}'
    saved = [t.data_ptr() for t in y.grad_fn.saved_tensors]
    assert sorted(saved) == sorted([a.data_ptr(), y.data_ptr()]) and x.data_ptr() not in saved
    with dispatch_trace() as tr, torch.autograd.profiler.profile() as prof:
        gx, ga = torch.autograd.grad(y, (x, a), cot)
    assert tr.kernels == ['seg_linear_scan_rows_kernel'] and tr.matching('seg_linear_scan_rows_kernel rev=1 bwd=1'), tr.records
    assert not aten_ops(prof), f'ATen operators in the backward: {aten_ops(prof)}'
    check_all(x, a, cot, lens, False, y, gx, ga, 'profiled run', 'autograd')
    # a scalar gate saves the output alone, and P in reverse runs the forward-direction kernel backward
    x2 = x.detach().clone().requires_grad_(True)
    y2 = ta.with_host_sizes(x2, lens).pack().linear_scan(0.96875, reverse=True).data
    assert len(y2.grad_fn.saved_tensors) == 1
    with dispatch_trace() as tr:
        y2.sum().backward()
    assert tr.matching('seg_linear_scan_rows_kernel rev=0 kind=2 gate=scalar bwd=1'), tr.records


def test_zz_report():
    """The worst achieved error / bound of this run, per group and dtype (for the GPU test log)."""
    for key in sorted(REPORT):
        print(f'linear_scan report: {key}: {REPORT[key]:.3e} of the bound')
