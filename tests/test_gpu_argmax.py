"""Per-sequence argmax / argmin / seq_max / seq_min on the GPU, and the take / put operators behind their autograd.

The yardstick is stock torch on the CPU, per sequence: torch.split + .max(dim=0) / .min(dim=0) (+ its autograd); an empty
sequence is index -1 and the identity.  The operator is exact, so every comparison is torch.equal — no tolerance
anywhere.  (Values that hold NaN are compared as bits-agnostic NaN masks plus torch.equal of the rest.)

Boundaries of the implementation (csrc/rua_argreduce.hip): a lanes-form step is 32 lanes x 8 tokens = 256 tokens, a
rows-form step 32 slots x 4 rows = 128 rows, a block 2 048 tokens (the 32-bit offset is re-based there), the cut form
applies to fewer than 1 024 units whose bound is at least 8 192.
"""
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _lib as K
from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64, I64 = torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int64
DTYPES = (F32, F64, BF16, F16, I64)
DT_IDS = [str(d).replace('torch.', '') for d in DTYPES]
HIDDEN = [(), (1,), (3,), (8,), (64,), (250,), (512,)]
I64_MIN, I64_MAX = torch.iinfo(I64).min, torch.iinfo(I64).max
# 0, 1, 2, the wave / half-wave sizes, both step sizes and the block size, each +-1; a few empty sequences
LENS = torch.tensor([0, 1, 2, 31, 32, 33, 63, 64, 65, 0, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 0, 5],
                    dtype=torch.long)


# ------------------------------------------------------------------ helpers
def LT(*values):
    return torch.tensor(values, dtype=torch.long)


def ident(dtype, op):
    if dtype == I64:
        return I64_MIN if op == 'max' else I64_MAX
    return float('-inf') if op == 'max' else float('inf')


_REF = {}


def ref(x_cpu, lens, op, key=None):
    """(values, indices) [B, *H] of stock torch on the CPU, sequence by sequence; computed once per `key`."""
    if key is not None and (key, op) in _REF:
        return _REF[(key, op)]
    hidden = tuple(x_cpu.shape[1:])
    vals, idxs = [], []
    for piece in torch.split(x_cpu, lens.tolist(), dim=0):
        if piece.size(0) == 0:
            vals.append(torch.full(hidden, ident(x_cpu.dtype, op), dtype=x_cpu.dtype))
            idxs.append(torch.full(hidden, -1, dtype=I64))
        else:
            r = piece.max(dim=0) if op == 'max' else piece.min(dim=0)
            vals.append(r.values)
            idxs.append(r.indices)
    out = (torch.stack(vals) if vals else torch.empty((0,) + hidden, dtype=x_cpu.dtype),
           torch.stack(idxs) if idxs else torch.empty((0,) + hidden, dtype=I64))
    if key is not None:
        _REF[(key, op)] = out
    return out


def same(got, want, what):
    """torch.equal, with NaNs required at the same places (torch.equal calls NaN != NaN)."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}'
    if got.is_floating_point():
        gn, wn = got != got, want != want
        assert torch.equal(gn, wn), f'{what}: NaNs at different places'
        got, want = torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want)
    assert torch.equal(got, want), f'{what}: differs at {(got != want).nonzero()[:4].tolist()}'


def draw(shape, dtype, seed, ties=True):
    g = torch.Generator().manual_seed(seed)
    if ties or dtype == I64:
        return torch.randint(-3, 4, shape, generator=g).to(dtype)
    return torch.randn(shape, generator=g, dtype=F64 if dtype == F64 else F32).to(dtype)


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


def shifted(t):
    """The same values at a base address off 16 bytes (by one element)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def check_all_ops(z, x_cpu, lens, what, key=None):
    for op in ('max', 'min'):
        wv, wi = ref(x_cpu, lens, op, key)
        r = ta.seq_max(z) if op == 'max' else ta.seq_min(z)
        assert r._fields == ('values', 'indices')
        same(r.indices, wi, f'{what} seq_{op}.indices')
        same(r.values, wv, f'{what} seq_{op}.values')
        same(z.argmax() if op == 'max' else z.argmin(), wi, f'{what} arg{op}')
    assert torch.equal(z.max().indices, ta.argmax(z)) and torch.equal(z.min().indices, ta.argmin(z))


# ------------------------------------------------------------------ every form in every layout
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('hidden', HIDDEN, ids=str)
def test_every_form_in_every_layout(hidden, dtype):
    n = int(LENS.sum())
    for ties in ((True,) if dtype == I64 else (True, False)):
        x_cpu = draw((n,) + hidden, dtype, 7 + int(ties), ties)
        x = x_cpu.to(DEV)
        key = (hidden, dtype, ties)
        for kind in 'CLPR':
            for host_sizes in (True, False):
                z = build(kind, x, LENS, host_sizes)
                check_all_ops(z, x_cpu, LENS, f'{kind} {hidden} {dtype} ties={ties} host={host_sizes}', key)
        for op, fn in (('max', ta.segment_argmax), ('min', ta.segment_argmin)):
            same(fn(x, LENS.to(DEV)), ref(x_cpu, LENS, op, key)[1], f'segment_arg{op}')


def test_torch_packed_sequence():
    seqs = [draw((k, 5), F32, 40 + k) for k in (3, 9, 1, 9, 4)]
    p = torch.nn.utils.rnn.pack_sequence([s.to(DEV) for s in seqs], enforce_sorted=False)
    lens = LT(3, 9, 1, 9, 4)
    check_all_ops(p, torch.cat(seqs), lens, 'torch pack_sequence')


@pytest.mark.parametrize('hidden', [(), (64,)], ids=str)
def test_only_empty_sequences_and_no_sequences(hidden):
    for lens in (torch.zeros(3, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        for dtype in (F32, I64):
            x = torch.empty((0,) + hidden, dtype=dtype, device=DEV)
            zs = [ta.C(x, lens.to(DEV))]
            if lens.numel():
                zs += [ta.L(torch.empty((lens.numel(), 0) + hidden, dtype=dtype, device=DEV), lens.to(DEV)),
                       ta.R(torch.empty((lens.numel(), 0) + hidden, dtype=dtype, device=DEV), lens.to(DEV))]
            for z in zs:
                check_all_ops(z, x.cpu(), lens, f'{type(z).__name__} B={lens.numel()} all empty')
            same(ta.segment_argmax(x, lens.to(DEV)), torch.full((lens.numel(),) + hidden, -1, dtype=I64), 'segment, empty')
    # all padding, and the padding holds NaN: never read
    pad = torch.full((3, 4) + hidden, float('nan'), device=DEV)
    r = ta.L(pad, torch.zeros(3, dtype=torch.long, device=DEV)).max()
    assert bool((r.indices == -1).all()) and bool((r.values == float('-inf')).all())


@pytest.mark.parametrize('kind', 'LR')
def test_padding_rows_are_never_read(kind):
    lens = LT(3, 0, 40, 7)
    x_cpu = draw((int(lens.sum()), 24), F32, 5)
    z = build(kind, x_cpu.to(DEV), lens)
    live = ta.with_host_sizes(torch.ones(int(lens.sum()), device=DEV), lens)
    mask = (live.left(0) if kind == 'L' else live.right(0)).data.bool()
    poisoned = torch.where(mask[..., None], z.data, torch.full_like(z.data, float('nan')))
    check_all_ops(rewrap(z, poisoned), x_cpu, lens, f'{kind} NaN padding')


# ------------------------------------------------------------------ the cut form
@pytest.mark.parametrize('dtype', (F32, BF16), ids=('float32', 'bfloat16'))
@pytest.mark.parametrize('where', ('first', 'last', 'tied'))
def test_cut_form(where, dtype):
    lens = LT(9000, 8200)
    H = 64
    x_cpu = draw((int(lens.sum()), H), dtype, 3)
    # the maximum (9) and the minimum (-9) of every column of both sequences, placed by hand
    for b, (off, n) in enumerate(((0, 9000), (9000, 8200))):
        spots = {'first': (5,), 'last': (n - 3,), 'tied': (2048 * 2 + 7, 2048 * 3 + 1)}[where]
        for s in spots:
            x_cpu[off + s, : H // 2] = 9
            x_cpu[off + s, H // 2:] = -9
    x = x_cpu.to(DEV)
    for kind in 'CLPR':
        z = build(kind, x, lens)
        lay, hid = lay_of(z), hidden_of(z)
        for op, code in (('max', K.MAX), ('min', K.MIN)):
            wv, wi = ref(x_cpu, lens, op, (where, dtype))
            with dispatch_trace() as tr:
                v1, i1 = O.launch_argreduce(lay, z.data, code, hid)
            assert tr.matching('seg_argreduce_rows_kernel cut=1 phase=partial') and \
                tr.matching('seg_argreduce_rows_kernel cut=1 phase=finish'), tr.records
            with dispatch_trace() as tr:
                v0, i0 = O.launch_argreduce(lay, z.data, code, hid, cut=False)
            assert tr.matching('seg_argreduce_rows_kernel cut=0') and len(tr.records) == 1, tr.records
            same(i1, wi, f'cut {kind} {op} index')
            same(v1, wv, f'cut {kind} {op} values')
            assert torch.equal(i1, i0) and torch.equal(v1, v0), f'cut != uncut, {kind} {op}'
            _, only = O.launch_argreduce(lay, z.data, code, hid, want_values=False)
            assert torch.equal(only, i1)
    assert int(ref(x_cpu, lens, 'max', (where, dtype))[1][0, 0]) == {'first': 5, 'last': 8997, 'tied': 4103}[where]


# ------------------------------------------------------------------ dispatch is what the tests think
RAGGED = LT(0, 1, 31, 32, 33, 129, 300, 64)
PATHS = [
    ('lanes_2B', 'C', (), BF16, False, 'seg_argreduce_lanes_kernel T=bf16 W=2'),
    ('lanes_4B_P', 'P', (), F32, False, 'seg_argreduce_lanes_kernel T=f32 W=4 kind=2'),
    ('lanes_8B_L', 'L', (), I64, False, 'seg_argreduce_lanes_kernel T=i64 W=8 kind=1'),
    ('lanes_6B', 'C', (3,), F16, False, 'seg_argreduce_lanes_kernel T=f16 W=2 H=3'),
    ('lanes_16B', 'C', (8,), BF16, False, 'seg_argreduce_lanes_kernel T=bf16 W=16'),
    ('lanes_16B_shifted', 'C', (8,), BF16, True, 'seg_argreduce_lanes_kernel T=bf16 W=2'),
    ('rows_aligned', 'C', (64,), F32, False, 'seg_argreduce_rows_kernel T=f32 AL=1 cut=0 chunks=2'),
    ('rows_aligned_R', 'R', (64,), F64, False, 'seg_argreduce_rows_kernel T=f64 AL=1 cut=0 kind=3'),
    ('rows_odd_width', 'C', (125,), F32, False, 'seg_argreduce_rows_kernel T=f32 AL=0 cut=0'),
    ('rows_shifted_base', 'C', (64,), F32, True, 'seg_argreduce_rows_kernel T=f32 AL=0 cut=0'),
    ('rows_P_f16', 'P', (24,), F16, False, 'seg_argreduce_rows_kernel T=f16 AL=1 cut=0 kind=2'),
]


@pytest.mark.parametrize('path', PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_path(path):
    pid, kind, hidden, dtype, shift, rec = path
    x_cpu = draw((int(RAGGED.sum()),) + hidden, dtype, 11)
    x = shifted(x_cpu.to(DEV)) if shift else x_cpu.to(DEV)
    z = build(kind, x, RAGGED)
    if shift:
        assert z.data.data_ptr() == x.data_ptr()
    for op in ('max', 'min'):
        with dispatch_trace() as tr:
            r = z.max() if op == 'max' else z.min()
        assert tr.matching(f'{rec} op={op} values=1') and len(tr.records) == 1, f'{pid}: wanted {rec}, got {tr.records}'
        with dispatch_trace() as tr:
            i = z.argmax() if op == 'max' else z.argmin()
        assert tr.matching(f'{rec} op={op} values=0') and len(tr.records) == 1, f'{pid}: wanted {rec}, got {tr.records}'
        wv, wi = ref(x_cpu, RAGGED, op)
        same(r.indices, wi, f'{pid} {op}')
        same(r.values, wv, f'{pid} {op}')
        same(i, wi, f'{pid} arg{op}')


def test_take_and_put_are_the_kernels_of_the_gradient():
    x = draw((int(RAGGED.sum()), 64), F32, 13, ties=False).to(DEV).requires_grad_(True)
    z = build('C', x, RAGGED)
    with dispatch_trace() as tr:
        v = z.max().values
        g, = torch.autograd.grad(v.sum(), x, create_graph=True)
        cot = torch.ones_like(v, requires_grad=True)
        g2, = torch.autograd.grad(v, x, cot, create_graph=True)
        g2.sum().backward()
    names = tr.kernels
    assert names.count('seg_put_kernel') == 2 and names.count('seg_take_kernel') == 1, tr.records
    assert set(names) == {'seg_argreduce_rows_kernel', 'seg_put_kernel', 'seg_take_kernel'}, tr.records


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (4,), (64,)], ids=str)
def test_special_values(kind, hidden):
    inf, nan = float('inf'), float('nan')
    lens = LT(6, 3, 40, 5, 300, 4, 2100, 7)
    x_cpu = draw((int(lens.sum()),) + hidden, F32, 91, ties=False)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    col = (0,) * len(hidden)
    x_cpu[(off[0] + 2,) + col] = nan                            # one NaN
    x_cpu[(off[1] + 2,) + col] = nan                            # two NaNs: the first wins
    x_cpu[(off[1] + 1,) + col] = nan
    x_cpu[(off[2] + 30,) + col] = nan                           # NaN together with +inf, the infinity first
    x_cpu[(off[2] + 3,) + col] = inf
    x_cpu[off[3]:off[3] + 5] = -inf                             # all -inf
    x_cpu[(off[4] + 290,) + col] = nan                          # (a NaN late in a sequence of several steps)
    x_cpu[off[5]:off[5] + 4] = torch.tensor([0.0, -0.0, -0.0, 0.0]).reshape((4,) + (1,) * len(hidden))
    x_cpu[(off[6] + 2099,) + col] = -inf                        # -inf and +inf in the last block of a long one
    x_cpu[(off[6] + 2050,) + col] = inf
    x_cpu[off[7]:off[7] + 7] = inf                              # all +inf
    z = build(kind, x_cpu.to(DEV), lens)
    check_all_ops(z, x_cpu, lens, f'special {kind} {hidden}')
    r, s = z.max(), z.min()
    at = lambda t, b: int(t[(b,) + col])
    assert at(r.indices, 0) == 2 and at(s.indices, 0) == 2
    assert at(r.indices, 1) == 1 and at(s.indices, 1) == 1
    assert at(r.indices, 2) == 30 and at(s.indices, 2) == 30
    assert at(r.indices, 3) == 0 and at(s.indices, 3) == 0
    assert at(r.indices, 5) == 0 and at(s.indices, 5) == 0
    assert at(r.indices, 6) == 2050 and at(s.indices, 6) == 2099
    assert at(r.indices, 7) == 0 and at(s.indices, 7) == 0
    # a NaN does not leak: the neighbours of the poisoned sequences hold none
    assert not bool(torch.isnan(r.values[3]).any()) and not bool(torch.isnan(r.values[5]).any())
    if hidden:
        assert not bool(torch.isnan(r.values[0][1:]).any())     # ... nor the other columns of its own sequence

    # +0.0 / -0.0 in the other order
    y_cpu = torch.tensor([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]).reshape((6,) + (1,) * len(hidden)).expand((6,) + hidden).contiguous()
    w = build(kind, y_cpu.to(DEV), LT(4, 2))
    check_all_ops(w, y_cpu, LT(4, 2), f'zeros {kind} {hidden}')
    assert at(w.argmax(), 0) == 0 and at(w.argmin(), 0) == 0


@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden', [(), (3,), (20,)], ids=str)
def test_int64_extremes(kind, hidden):
    lens = LT(5, 0, 300, 3)
    x_cpu = draw((int(lens.sum()),) + hidden, I64, 17)
    x_cpu[1] = I64_MAX
    x_cpu[3] = I64_MAX
    x_cpu[2] = I64_MIN
    x_cpu[4] = I64_MIN
    x_cpu[5 + 200] = I64_MAX - 1
    x_cpu[5 + 100] = I64_MIN + 1
    x_cpu[305:308] = I64_MIN                                     # equal to the identity of max: position 0, not -1
    z = build(kind, x_cpu.to(DEV), lens)
    check_all_ops(z, x_cpu, lens, f'int64 extremes {kind} {hidden}')
    r = z.max()
    assert bool((r.indices[3] == 0).all()) and bool((r.indices[1] == -1).all()) and bool((r.values[1] == I64_MIN).all())
    assert bool((z.min().values[1] == I64_MAX).all())


# ------------------------------------------------------------------ identities, bit for bit
IDENT = [((), F32), ((8,), BF16), ((64,), F32), ((125,), F16), ((3,), F64), ((), I64), ((40,), I64)]


@pytest.mark.parametrize('hidden,dtype', IDENT, ids=[f'{h}-{d}'.replace('torch.', '') for h, d in IDENT])
def test_identities(hidden, dtype):
    lens = LT(0, 1, 33, 64, 129, 2049, 5, 0, 300)
    x_cpu = draw((int(lens.sum()),) + hidden, dtype, 23)
    x = x_cpu.to(DEV)
    c = build('C', x, lens)
    base = c.max()
    for kind in 'LPR':                                           # the same result from the four layouts
        z = build(kind, x, lens)
        r, s = z.max(), z.min()
        assert torch.equal(r.indices, base.indices) and torch.equal(r.values, base.values), kind
        assert torch.equal(s.indices, c.min().indices) and torch.equal(s.values, c.min().values), kind
        # take at the argmax is the selected value wherever the sequence is not empty
        t = O.launch_take(lay_of(z), z.data, z.argmax(), hidden_of(z))
        live = (lens > 0).to(DEV)
        assert torch.equal(t[live], r.values[live]), kind
        assert bool((t[~live] == 0).all())
    # a base off 16 bytes by one element
    u = ta.with_host_sizes(shifted(x), lens)
    r = u.max()
    assert torch.equal(r.indices, base.indices) and torch.equal(r.values, base.values)
    assert torch.equal(u.argmin(), c.argmin())
    if dtype != I64:                                             # finite inputs, no empty sequence: reduce_max's values
        keep = lens > 0
        xs = torch.cat([p for p, k in zip(torch.split(x, lens.tolist()), keep.tolist()) if k])
        d = ta.with_host_sizes(xs, lens[keep])
        for kind in 'CLPR':
            z = {'C': lambda: d, 'L': lambda: d.left(0), 'R': lambda: d.right(0), 'P': d.pack}[kind]()
            assert torch.equal(z.max().values, ta.reduce_max(z)), kind
            assert torch.equal(z.min().values, ta.reduce_min(z)), kind


# ------------------------------------------------------------------ gradients
def cpu_grads(x_cpu, lens, cot_cpu, w_cpu, op):
    """torch on the CPU, per sequence: d<values, cot>/dx, and the second-order d<that, w>/dcot."""
    x = x_cpu.clone().requires_grad_(True)
    cot = cot_cpu.clone().requires_grad_(True)
    vals = []
    for b, piece in enumerate(torch.split(x, lens.tolist(), dim=0)):
        if piece.size(0):
            vals.append(((piece.max(dim=0) if op == 'max' else piece.min(dim=0)).values * cot[b]).sum())
    total = torch.stack(vals).sum()
    g, = torch.autograd.grad(total, x, create_graph=True)
    gg, = torch.autograd.grad((g * w_cpu).sum(), cot, allow_unused=True)
    return g.detach(), torch.zeros_like(cot_cpu) if gg is None else gg


@pytest.mark.parametrize('dtype', (F32, F64, BF16), ids=('float32', 'float64', 'bfloat16'))
@pytest.mark.parametrize('hidden', [(), (3,), (8,), (64,), (250,)], ids=str)
def test_gradients(hidden, dtype):
    lens = LT(0, 1, 33, 64, 129, 0, 300, 5)
    n, B = int(lens.sum()), lens.numel()
    x_cpu = draw((n,) + hidden, dtype, 31)                       # ties in every column: the chosen token takes it all
    cot_cpu = draw((B,) + hidden, dtype, 32, ties=False)
    w_cpu = draw((n,) + hidden, dtype, 33, ties=False)
    for op in ('max', 'min'):
        want_g, want_gg = cpu_grads(x_cpu, lens, cot_cpu, w_cpu, op)
        for kind in 'CLPR':
            z = build(kind, x_cpu.to(DEV), lens)
            leaf = z.data.detach().clone().requires_grad_(True)
            cot = cot_cpu.to(DEV).requires_grad_(True)
            zz = rewrap(z, leaf)
            r = zz.max() if op == 'max' else zz.min()
            assert not r.indices.requires_grad and r.values.requires_grad
            g, = torch.autograd.grad(r.values, leaf, cot, create_graph=True)
            same(rewrap(z, g.detach()).cat().data, want_g, f'grad {kind} {op} {hidden}')
            if kind in 'LR':                                     # padding rows of the gradient: zeros
                assert int((g.detach() != 0).sum()) == int((want_g != 0).sum())
                assert not bool(torch.isnan(g.detach()).any())
            w = build(kind, w_cpu.to(DEV), lens).data
            gg, = torch.autograd.grad((g * w).sum(), cot)
            same(gg, want_gg, f'second order {kind} {op} {hidden}')
            # plain backward, no graph
            leaf2 = z.data.detach().clone().requires_grad_(True)
            r2 = rewrap(z, leaf2).max() if op == 'max' else rewrap(z, leaf2).min()
            r2.values.backward(cot_cpu.to(DEV))
            assert torch.equal(leaf2.grad, g.detach())


# ------------------------------------------------------------------ put / take directly
@pytest.mark.parametrize('kind', 'CLPR')
@pytest.mark.parametrize('hidden,dtype', [((), F32), ((3,), BF16), ((8,), F16), ((64,), F32), ((125,), F64), ((40,), I64)],
                         ids=str)
def test_put_and_take(kind, hidden, dtype):
    lens = LT(4, 0, 33, 300, 1)
    B, n = lens.numel(), int(lens.sum())
    x_cpu = draw((n,) + hidden, dtype, 51)
    z = build(kind, x_cpu.to(DEV), lens)
    lay, hid = lay_of(z), hidden_of(z)
    g = torch.Generator().manual_seed(52)
    index = torch.stack([torch.randint(0, max(int(k), 1), hidden, generator=g) for k in lens.tolist()])
    index[0] = -1                                               # no token
    index[2] = 33                                               # == len: no token
    index[1] = 0                                                # an empty sequence has no token 0
    flat = index.reshape(B, -1)
    flat[3, ::2] = 299                                          # the last token
    flat[4, :] = 0
    src_cpu = draw((B,) + hidden, dtype, 53) + 5                # (never zero)
    # wanted, in cat form
    want_put = torch.zeros_like(x_cpu)
    want_take = torch.zeros((B,) + hidden, dtype=dtype)
    off = (torch.cumsum(lens, 0) - lens).tolist()
    xs, wp, wt = x_cpu.reshape(n, -1), want_put.reshape(n, -1), want_take.reshape(B, -1)
    ss = src_cpu.reshape(B, -1)
    for b in range(B):
        for h in range(flat.size(1)):
            t = int(flat[b, h])
            if 0 <= t < int(lens[b]):
                wp[off[b] + t, h] = ss[b, h]
                wt[b, h] = xs[off[b] + t, h]
    with dispatch_trace() as tr:
        took = O.launch_take(lay, z.data, index.to(DEV), hid)
    assert tr.kernels == ['seg_take_kernel'], tr.records
    same(took, want_take, f'take {kind}')
    # put into a buffer pre-filled with NaN (int64: with ones): every element is written
    out = torch.full(z.data.shape, float('nan') if dtype != I64 else 1, dtype=dtype, device=DEV)
    with dispatch_trace() as tr:
        O.launch_put(lay, src_cpu.to(DEV), index.to(DEV), hid, z.data.shape, out=out)
    assert tr.kernels == ['seg_put_kernel'], tr.records
    if dtype != I64:
        assert not bool(torch.isnan(out).any()), 'put left an element unwritten'
    same(rewrap(z, out).cat().data, want_put, f'put {kind}')
    assert int((out != 0).sum()) == int((want_put != 0).sum())   # padding rows of L / R: zeros
    # adjoint: <put(s), y> == <s, take(y)> exactly on small integers
    if dtype != I64:
        lhs = (out.double() * z.data.double()).sum()
        rhs = (src_cpu.to(DEV).double() * took.double()).sum()
        assert float(lhs) == float(rhs)


def test_put_cuts_long_sequences_into_blocks():
    lens = LT(9000, 8200)
    x = torch.zeros(int(lens.sum()), 64, device=DEV)
    for kind in 'CLPR':
        z = build(kind, x, lens)
        index = torch.stack([torch.full((64,), 8999, dtype=I64), torch.arange(64) * 128]).to(DEV)
        src = torch.arange(1, 129, dtype=F32, device=DEV).reshape(2, 64)
        out = torch.full(z.data.shape, float('nan'), device=DEV)
        with dispatch_trace() as tr:
            O.launch_put(lay_of(z), src, index, (64,), z.data.shape, out=out)
        assert tr.matching('seg_put_kernel AL=1 blocks=5' if kind != 'C' else 'seg_put_kernel AL=1'), tr.records
        got = rewrap(z, out).cat().data.cpu()
        want = torch.zeros(int(lens.sum()), 64)
        want[8999] = src[0].cpu()
        want[9000 + torch.arange(64) * 128, torch.arange(64)] = src[1].cpu()
        assert torch.equal(got, want), kind
        assert torch.equal(O.launch_take(lay_of(z), out, index, (64,)), src)


def test_unsupported_dtype_raises():
    x = torch.zeros(4, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ta.RuaError):
        ta.segment_argmax(x, LT(4).to(DEV))
    with pytest.raises(ta.RuaError):
        ta.C(x, LT(4).to(DEV)).max()
