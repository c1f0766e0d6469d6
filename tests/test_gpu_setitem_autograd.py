"""An in-place `__setitem__` that autograd sees runs on the library's kernels: the row mover in scatter mode in the
forward (`_ops._ScatterRows`), the fused gather-and-zero kernel (rua_setitem_backward) in the backward.  Bit-exact against
the reference's CPU autograd (tests/golden/r6_setitem_grad.npz: integer-valued floats, so every sum is exact in any
order) and against stock torch on the same device."""
import contextlib

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import torchrua_amd as ta
from torchrua_amd import _ops as O
from torchrua_amd import core
from helpers import to_np, to_torch
from gpu_util import DEV, KINDS, dispatch_trace
from test_setitem_grad_fixtures import CASES

pytestmark = pytest.mark.gpu

ATEN_INDEXING = ('index_put', 'index_add', 'index_select', 'index.Tensor', 'gather')


# ------------------------------------------------------------------ plumbing
def container(kind: str, data: torch.Tensor, f):
    if kind == 'P':
        return ta.P(data, torch.from_numpy(f['batch_sizes'].copy()), to_torch(f['sorted_indices'], DEV),
                    to_torch(f['unsorted_indices'], DEV))
    return KINDS[kind](data, to_torch(f['lens'], DEV))


def key_of(f):
    form = str(f['form'])
    if form in ('pair', 'pair2d'):
        return to_torch(f['bp'], DEV), to_torch(f['tp'], DEV)
    idx = to_torch(f['idx'], DEV)
    if form in ('zkey', 'tensorZ'):
        return ta.C(idx, to_torch(f['key_lens'], DEV))
    if form == 'zkeyL':
        return ta.L(idx, to_torch(f['key_lens'], DEV))
    return idx


@contextlib.contextmanager
def patched(on: bool):
    if on:
        ta.patch_tensor_indexing()
    try:
        yield
    finally:
        if on:
            ta.unpatch_tensor_indexing()


def write(f, base_grad=True, value_grad=True):
    """Replay a fixture case on the GPU: (written storage, base leaf, value leaf)."""
    bf = str(f['dtype']) == 'bf16'
    kind, form = str(f['kind']), str(f['form'])
    s = to_torch(f['base'], DEV, bf16=bf).requires_grad_(base_grad)
    v = to_torch(f['value'], DEV, bf16=bf).requires_grad_(value_grad)
    z = container(kind, s * 2.0, f)
    key = key_of(f)
    with patched(form == 'tensorZ'):
        if form == 'tensorZ':
            z.raw()[key] = v
        else:
            z[key] = v
    return z.data, s, v


class OpNames(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


@contextlib.contextmanager
def kernel_names():
    seen = []
    prev = O._kernel_hook
    O.set_kernel_hook(lambda name, start: seen.append(name) if start else None)
    try:
        yield seen
    finally:
        O.set_kernel_hook(prev)


# ------------------------------------------------------------------ the reference's results, bit for bit
@pytest.mark.parametrize('case', sorted(CASES))
def test_fixture_case_is_bit_exact(case):
    f = CASES[case]
    bf = str(f['dtype']) == 'bf16'
    out, s, v = write(f)
    assert out.grad_fn is not None
    cot = to_torch(f['cot'], DEV, bf16=bf)
    g_base, g_value = torch.autograd.grad(out, [s, v], cot)
    assert g_value.shape == v.shape and g_value.dtype == v.dtype
    assert to_np(g_value).tobytes() == f['grad_value'].tobytes(), 'gradient w.r.t. the value'
    assert np.array_equal(to_np(g_base), f['grad_base']), 'gradient w.r.t. the base'
    if int(f['unique']):
        assert np.array_equal(to_np(out), f['out']), 'written storage'


# ------------------------------------------------------------------ no ATen indexing kernel, forward or backward
FORMS = sorted({(str(f['kind']), str(f['form'])) for f in CASES.values()})


@pytest.mark.parametrize('kind,form', FORMS)
def test_no_aten_indexing_kernel_runs(kind, form):
    name = next(c for c in sorted(CASES) if str(CASES[c]['kind']) == kind and str(CASES[c]['form']) == form)
    f = CASES[name]
    cot = to_torch(f['cot'], DEV, bf16=str(f['dtype']) == 'bf16')
    with kernel_names() as seen, OpNames() as ops:
        out, s, v = write(f)
        torch.autograd.grad(out, [s, v], cot)
        torch.cuda.synchronize()
    bad = [n for n in ops.names if any(w in n for w in ATEN_INDEXING)]
    assert not bad, f'{name}: ATen indexing ops ran: {sorted(set(bad))}'
    plan = 'setitem' if form in ('pair', 'pair2d') else 'scatter_flat'
    assert plan in seen, f'{name}: the scatter plan did not run ({seen})'
    assert plan + '_bwd' in seen, f'{name}: the fused backward did not run ({seen})'
    assert 'flat_rows' not in seen, f'{name}: the flat rows were computed although nothing consumes them'


@pytest.mark.parametrize('kind', list('CLPR'))
def test_the_copy_runs_only_when_the_storage_gradient_is_wanted(kind):
    f = CASES[f'{kind}.pair.full.h5.fp32.u']
    cot = to_torch(f['cot'], DEV)
    with dispatch_trace() as t:
        out, s, v = write(f, base_grad=False)                 # only `value` requires grad: the common case
        g_value, = torch.autograd.grad(out, [v], cot)
    assert to_np(g_value).tobytes() == f['grad_value'].tobytes()
    assert 'setitem_backward_kernel' in t.kernels and 'setitem_backward_copy' not in t.kernels
    assert t.matching('setitem_backward_kernel value=1 raw=0')
    with dispatch_trace() as t:
        out, s, v = write(f, value_grad=False)                # only the storage: copy and zero
        g_base, = torch.autograd.grad(out, [s], cot)
    assert np.array_equal(to_np(g_base), f['grad_base'])
    assert t.kernels.count('setitem_backward_copy') == 1 and t.matching('setitem_backward_kernel value=0 raw=1')
    with dispatch_trace() as t:
        out, s, v = write(f)
        torch.autograd.grad(out, [s, v], cot)
    assert t.kernels.count('setitem_backward_copy') == 1 and t.matching('setitem_backward_kernel value=1 raw=1')


# ------------------------------------------------------------------ against stock torch at a realistic size
@pytest.mark.parametrize('H,dtype', [(512, torch.bfloat16), (125, torch.float32)])
def test_against_stock_torch_at_a_realistic_size(H, dtype):
    B, T, M = 4096, 256, 300_000
    N = B * T                                                                 # ~1 M storage rows
    g = torch.Generator(device=DEV).manual_seed(H)
    base = torch.randn(N, H, generator=g, device=DEV, dtype=torch.float32).to(dtype)
    value = torch.randn(M, H, generator=g, device=DEV, dtype=torch.float32).to(dtype)
    cot = torch.randn(N, H, generator=g, device=DEV, dtype=torch.float32).to(dtype)
    lens = torch.full((B,), T, dtype=torch.long, device=DEV)
    for unique in (False, True):
        if unique:
            rows = torch.randperm(N, generator=g, device=DEV)[:M]
        else:
            rows = torch.randint(0, N, (M,), generator=g, device=DEV)
        bp, tp = rows // T, rows % T
        s, v = base.clone().requires_grad_(True), value.clone().requires_grad_(True)
        c = ta.C(s * 2.0, lens)
        c[bp, tp] = v
        gs, gv = torch.autograd.grad(c.data, [s, v], cot)
        rs, rv = base.clone().requires_grad_(True), value.clone().requires_grad_(True)
        ref = rs * 2.0
        ref[rows] = rv
        es, ev = torch.autograd.grad(ref, [rs, rv], cot)
        assert torch.equal(gv, ev), 'gradient w.r.t. the value'
        assert torch.equal(gs, es), 'gradient w.r.t. the base'
        if unique:
            assert torch.equal(c.data.detach(), ref.detach()), 'written storage'
        del s, v, c, gs, gv, rs, rv, ref, es, ev


# ------------------------------------------------------------------ second order
@pytest.mark.parametrize('kind', list('CLPR'))
@pytest.mark.parametrize('vshape', ['full', 'H'])
def test_second_order_equals_stock_torch(kind, vshape):
    """grad(..., create_graph=True) through the write, then a second grad.  Small integers in fp32: every product and sum
    is exact, so the order in which repeats are accumulated does not show.  The loss is quadratic in the written storage, so
    its gradients depend on WHICH write of a repeated row won — undefined in torch too: the full value gets unique keys,
    the broadcast row (the same bytes whoever wins) keeps the repeats — and two pairs that name no token, which the
    composed backward must gather as zeros (its flat rows put them past the storage's end)."""
    g = torch.Generator().manual_seed(17)
    lens = torch.tensor([3, 5, 1, 4, 2])
    H = 6
    c0 = ta.with_host_sizes(torch.randint(-3, 4, (int(lens.sum()), H), generator=g).float().to(DEV), lens)
    z0 = {'C': c0, 'L': c0.left(), 'P': c0.pack(), 'R': c0.right()}[kind]
    bp_all, tp_all = c0.ptr()
    pick = torch.tensor([0, 7, 12, 3, 14, 9, 5, 11] if vshape == 'full' else [0, 7, 7, 3, 14, 9, 0, 11], device=DEV)
    bp, tp = bp_all[pick], tp_all[pick]
    rows = core._flat_rows(z0, (bp, tp))
    if vshape == 'H':                                   # sequence 2 has one token; there is no sequence 9
        bp = torch.cat([bp[:3], torch.tensor([2, 9], device=DEV), bp[3:]])
        tp = torch.cat([tp[:3], torch.tensor([3, 0], device=DEV), tp[3:]])
    value = torch.randint(-3, 4, (8, H) if vshape == 'full' else (H,), generator=g).float().to(DEV)
    w = torch.randint(-2, 3, z0.data.shape, generator=g).float().to(DEV)

    def both(write_fn):
        s = z0.data.detach().clone().requires_grad_(True)
        v = value.clone().requires_grad_(True)
        data = s * 2.0
        out = write_fn(data, v)
        loss = (out * out * w).sum()
        first = torch.autograd.grad(loss, [s, v], create_graph=True)
        second = torch.autograd.grad(sum((x * x).sum() for x in first), [s, v])
        return [out.detach()] + [x.detach() for x in first] + list(second)

    def mine(data, v):
        z = z0._replace(data=data)
        z[bp, tp] = v
        return z.data

    def stock(data, v):
        raw = data.flatten(0, 1) if kind in 'LR' else data
        raw[rows] = v
        return data

    got, exp = both(mine), both(stock)
    for name, a, b in zip(('out', 'd/ds', 'd/dv', 'd2/ds', 'd2/dv'), got, exp):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ values broadcast along the rows of a 2-D / 3-D key
@pytest.mark.parametrize('lead,vshape', [
    ((4, 3), (1, 3, 5)), ((4, 3), (3, 5)),        # a leading run of row dims: the reducer, one sequence per kept row
    ((4, 3), (4, 1, 5)), ((4, 3), (4, 1, 1)),     # a trailing run: one sequence per leading row (+ inside the row)
    ((2, 3, 2), (2, 1, 2, 5)),                    # row dims broadcast in the middle: sum_to_size
    ((2, 3, 2), (1, 1, 2, 5)), ((2, 3, 2), (2, 1, 1, 5)), ((2, 3, 2), (5,)), ((2, 3, 2), ()),
])
@pytest.mark.parametrize('order', [1, 2])
def test_value_broadcast_along_row_dims_equals_stock_torch(lead, vshape, order):
    """`z[index] = v` with a 2-D / 3-D row index and a value that is broadcast along some of the index's dims, against
    stock torch's own setitem: small integers in fp32, so every sum is exact in any order.  Unique rows (the loss of the
    second-order leg is quadratic in the written storage)."""
    g = torch.Generator().manual_seed(len(lead) * 100 + len(vshape))
    n, H = 40, 5
    m = int(np.prod(lead))
    index = torch.randperm(n, generator=g)[:m].reshape(lead).to(DEV)
    base = torch.randint(-3, 4, (n, H), generator=g).float().to(DEV)
    value = torch.randint(-3, 4, vshape, generator=g).float().to(DEV)
    w = torch.randint(-2, 3, (n, H), generator=g).float().to(DEV)
    lens = torch.tensor([n], device=DEV)

    def run(mine):
        s, v = base.clone().requires_grad_(True), value.clone().requires_grad_(True)
        data = s * 2.0
        if mine:
            ta.C(data, lens)[index] = v
        else:
            data[index] = v
        if order == 1:
            return [data.detach()] + list(torch.autograd.grad(data, [s, v], w))
        first = torch.autograd.grad((data * data * w).sum(), [s, v], create_graph=True)
        return [data.detach()] + [x.detach() for x in first] + list(torch.autograd.grad(sum((x * x).sum() for x in first), [s, v]))

    with kernel_names() as seen:
        got = run(True)
    assert 'scatter_flat' in seen
    for a, b in zip(got, run(False)):
        assert a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------ 1-byte lanes
@pytest.mark.parametrize('hidden', [(), (3,), (7,)])
@pytest.mark.parametrize('dtype', [torch.int8, torch.uint8])
def test_rows_of_an_odd_number_of_bytes(hidden, dtype):
    """Rows of 1, 3 and 7 bytes reach rua_setitem_backward's 1-byte lanes (no autograd: integer payloads carry no
    gradient, the entry point moves bytes)."""
    g = torch.Generator().manual_seed(11)
    n = 333
    grad = torch.randint(1, 120, (n,) + hidden, generator=g).to(dtype).to(DEV)
    rows = torch.randint(-n, n, (500,), generator=g).to(DEV)                      # repeats, negative rows
    from torchrua_amd import _lib as K
    from torchrua_amd import _meta as M
    plan = O.MovePlan(M.lay_list(None, rows), M.lay_flat(n), grad.shape, flags=K.MOVE_SCATTER, name='scatter_flat')
    with dispatch_trace() as t:
        g_value, g_raw = O.setitem_backward(plan, grad, hidden, True, True)
    assert t.matching('setitem_backward_kernel VEC=1')
    assert torch.equal(g_value, grad[rows])
    exp = grad.clone()
    exp[rows] = 0
    assert torch.equal(g_raw, exp)


# ------------------------------------------------------------------ nothing keeps the written storage alive
@pytest.mark.parametrize('kind', list('CLPR'))
@pytest.mark.parametrize('form', ['pair', 'flat'])
@pytest.mark.parametrize('backward', [False, True])
def test_the_written_storage_is_freed_by_reference_counting(kind, form, backward):
    """The autograd node of the write must not reference the written storage (a closure over the container would: storage
    -> grad_fn -> ctx -> closure -> container -> storage).  With the cyclic collector OFF, dropping the last references
    frees the storage at once, as after torch's own setitem."""
    import gc
    import weakref
    z0 = _small(kind, H=64)
    value = torch.ones(2, 64, device=DEV, requires_grad=True)
    bp, tp = torch.tensor([2, 0], device=DEV), torch.tensor([1, 2], device=DEV)
    rows = torch.tensor([3, 1], device=DEV)

    def once():
        s = z0.data.clone().requires_grad_(True)
        z = z0._replace(data=s * 2.0)
        if form == 'pair':
            z[bp, tp] = value
        else:
            z[rows] = value
        alive = weakref.ref(z.data)
        if backward:
            gs, gv = torch.autograd.grad(z.data, [s, value], torch.ones_like(z.data))
            del gs, gv
        del z, s
        return alive

    once()                                              # (whatever is memoised on the lengths is allocated now)
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        level = torch.cuda.memory_allocated()
        alive = once()
        torch.cuda.synchronize()
        assert alive() is None, 'the written storage is still referenced (a cycle through its autograd node)'
        assert torch.cuda.memory_allocated() == level
    finally:
        gc.enable()


# ------------------------------------------------------------------ edges
def _small(kind='C', H=5, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor([3, 1, 4, 2])
    c = ta.with_host_sizes(torch.randint(-4, 5, (10, H), generator=g).to(dtype).to(DEV), lens)
    return {'C': c, 'L': c.left(), 'P': c.pack(), 'R': c.right()}[kind]


def test_a_leaf_that_requires_grad_raises_and_is_not_written():
    z = _small()
    leaf = z.data.clone().requires_grad_(True)
    before = leaf.detach().clone()
    bp, tp = torch.tensor([2], device=DEV), torch.tensor([1], device=DEV)
    with pytest.raises(RuntimeError):
        z._replace(data=leaf)[bp, tp] = torch.ones(1, 5, device=DEV)
    with pytest.raises(RuntimeError):
        z._replace(data=leaf)[torch.tensor([4], device=DEV)] = torch.ones(1, 5, device=DEV)
    lz = _small('L')
    lleaf = lz.data.clone().requires_grad_(True)
    with pytest.raises(RuntimeError):                            # L.raw() is a view of the leaf
        lz._replace(data=lleaf)[torch.tensor([1], device=DEV)] = torch.ones(1, 5, device=DEV)
    assert torch.equal(leaf.detach(), before)


@pytest.mark.parametrize('kind', list('CLPR'))
def test_version_moves_by_torchs_amount(kind):
    z = _small(kind)
    bp, tp = torch.tensor([2, 0], device=DEV), torch.tensor([1, 2], device=DEV)
    v = torch.ones(2, 5, device=DEV, requires_grad=True)
    data = z.data.clone()
    v0 = data._version
    z._replace(data=data)[bp, tp] = v
    ref = z.data.clone()
    r0 = ref._version
    (ref.flatten(0, 1) if kind in 'LR' else ref)[torch.tensor([0, 1], device=DEV)] = v.detach().clone().requires_grad_(True)
    assert data._version - v0 == ref._version - r0 == 1
    assert data.grad_fn is not None
    data2 = z.data.clone()
    v0 = data2._version
    z._replace(data=data2)[torch.tensor([3, 1], device=DEV)] = v           # the flat-key path (through raw(): a view for L / R)
    assert data2._version - v0 == 1 and data2.grad_fn is not None


def test_a_write_under_no_grad_takes_the_old_path():
    z = _small()
    v = torch.ones(1, 5, device=DEV, requires_grad=True)
    data = z.data.clone()
    v0 = data._version
    with kernel_names() as seen, torch.no_grad():
        z._replace(data=data)[torch.tensor([2], device=DEV), torch.tensor([3], device=DEV)] = v
    assert seen == ['setitem'] and data.grad_fn is None and not data.requires_grad and data._version > v0
    assert bool((data[7] == 1).all())


def test_a_value_of_another_dtype_gets_a_gradient_of_its_own_dtype():
    z = _small(dtype=torch.bfloat16)
    s = z.data.clone().requires_grad_(True)
    v = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0]], device=DEV, requires_grad=True)            # fp32 into bf16
    c = ta.C(s * 2.0, z.token_sizes)
    c[torch.tensor([1], device=DEV), torch.tensor([0], device=DEV)] = v
    assert c.data.dtype == torch.bfloat16 and torch.equal(c.data[3].float(), v.detach()[0])
    cot = torch.arange(50, device=DEV).reshape(10, 5).to(torch.bfloat16)
    gs, gv = torch.autograd.grad(c.data, [s, v], cot)
    assert gv.dtype == torch.float32 and gs.dtype == torch.bfloat16
    assert torch.equal(gv, cot[3:4].float())
    exp = cot * 2
    exp[3] = 0
    assert torch.equal(gs, exp)


@pytest.mark.parametrize('kind', list('CLPR'))
def test_no_keys_at_all(kind):
    z = _small(kind)
    s = z.data.clone().requires_grad_(True)
    v = torch.zeros(0, 5, device=DEV, requires_grad=True)
    zz = z._replace(data=s * 2.0)
    empty = torch.zeros(0, dtype=torch.long, device=DEV)
    zz[empty, empty] = v
    assert torch.equal(zz.data.detach(), z.data * 2.0)
    cot = torch.ones_like(z.data)
    gs, gv = torch.autograd.grad(zz.data, [s, v], cot)
    assert gv.shape == (0, 5) and torch.equal(gs, cot * 2.0)


@pytest.mark.parametrize('kind', list('CLPR'))
def test_a_pair_that_names_no_token_is_skipped(kind):
    z = _small(kind)                                                            # lengths 3, 1, 4, 2
    bp = torch.tensor([0, 1, 2, 9, -1, 3], device=DEV)
    tp = torch.tensor([2, 1, 3, 0, 0, 5], device=DEV)                           # entries 1, 3, 4, 5 name no token
    plain = z._replace(data=z.data.clone() * 2.0)
    value = torch.arange(30, device=DEV).reshape(6, 5).float()
    plain[bp, tp] = value                                                       # the no-grad path
    s = z.data.clone().requires_grad_(True)
    v = value.clone().requires_grad_(True)
    zz = z._replace(data=s * 2.0)
    zz[bp, tp] = v
    assert torch.equal(zz.data.detach(), plain.data)
    cot = torch.randint(1, 5, z.data.shape, device=DEV).float()
    gs, gv = torch.autograd.grad(zz.data, [s, v], cot)
    rows = core._flat_rows(z, (bp[[0, 2]], tp[[0, 2]]))
    flat_cot = cot.reshape(-1, 5)
    assert torch.equal(gv[[0, 2]], flat_cot[rows]) and not gv[[1, 3, 4, 5]].any()
    exp = (cot * 2.0).reshape(-1, 5).clone()
    exp[rows] = 0
    assert torch.equal(gs.reshape(-1, 5), exp)


@pytest.mark.parametrize('row_bytes', [32, 1024, 24, 40, 1000, 20])
@pytest.mark.parametrize('off_bytes', [4, 8])
def test_misaligned_storage_and_cotangent_give_the_same_bits(row_bytes, off_bytes):
    """A payload view that starts 4 or 8 bytes into an allocation is contiguous and reaches the kernels as it is: the
    narrower-lane forms of the forward scatter and of the gather-and-zero backward give the bits of the aligned run."""
    H = row_bytes // 4
    g = torch.Generator().manual_seed(row_bytes + off_bytes)
    lens = torch.tensor([3, 1, 7, 2, 5, 0, 4, 9, 1, 6, 2, 8, 70])
    N, off = int(lens.sum()), off_bytes // 4
    base = torch.randint(-9, 10, (N, H), generator=g).float().to(DEV)
    cot = torch.randint(-9, 10, (N, H), generator=g).float().to(DEV)
    pick = torch.randint(0, N, (100,), generator=g)
    bp = torch.repeat_interleave(torch.arange(lens.numel()), lens)[pick].to(DEV)
    tp = torch.cat([torch.arange(int(k)) for k in lens])[pick].to(DEV)
    value = torch.randint(-9, 10, (100, H), generator=g).float().to(DEV)
    dl = lens.to(DEV)

    def run(shift):
        def at(t):
            flat = torch.empty(t.numel() + shift + 16, device=DEV)
            view = flat[shift:shift + t.numel()].view(t.shape)
            view.copy_(t)
            return view
        store, c = at(base), at(cot)
        assert store.is_contiguous() and store.data_ptr() % 16 == 4 * shift % 16
        v = value.clone().requires_grad_(True)
        # value only: the write goes into the misaligned storage itself
        z = ta.C(store, dl)
        z[bp, tp] = v
        gv, = torch.autograd.grad(z.data, [v], c)
        # value and storage: a non-leaf that requires grad (aligned: autograd made it), the cotangent misaligned
        s2 = base.clone().requires_grad_(True)
        z2 = ta.C(s2 * 2.0, dl)
        z2[bp, tp] = v
        gs2, gv2 = torch.autograd.grad(z2.data, [s2, v], c)
        return store.clone(), gv, gs2, gv2

    aligned, shifted = run(0), run(off)
    for name, a, b in zip(('storage', 'd/dv (value only)', 'd/ds', 'd/dv'), aligned, shifted):
        if name == 'storage':
            continue                                              # (repeats among the keys: the winner is undefined)
        assert torch.equal(a, b), name
    rows = core._flat_rows(ta.C(base, dl), (bp, tp))
    assert torch.equal(aligned[1], cot[rows]) and torch.equal(aligned[3], cot[rows])
    exp = cot * 2.0
    exp[rows] = 0
    assert torch.equal(aligned[2], exp)


def test_a_write_on_a_non_default_stream():
    f = CASES['P.pair.full.h125.fp32.u']
    cot = to_torch(f['cot'], DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        out, s, v = write(f)
        g_base, g_value = torch.autograd.grad(out, [s, v], cot)
    side.synchronize()
    assert np.array_equal(to_np(out), f['out'])
    assert np.array_equal(to_np(g_base), f['grad_base']) and np.array_equal(to_np(g_value), f['grad_value'])
