"""Per-sequence stable sort / argsort / reorder / topk on the GPU.  The reference is torch.sort(seq.cpu(), dim=0,
stable=True, descending=d) of every sequence on its own; values are compared as BITS and indices exactly, padding rows
of L / R results included (zeros).  Every container is compared with the same reference cast through the library's own
row movers, which is the commutation identity across C / L / P / R."""
import zlib

import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _lib

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64, I64, I8, BOOL = (torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64,
                                      torch.int8, torch.bool)
KINDS = 'CLPR'
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def block_len() -> int:
    return int(_lib.load().rua_sort_block_len())


def batches():
    """name -> lengths.  The forms go by the longest sequence: <= 64 lanes, <= block the LDS network, longer the merge;
    at most two long sequences per case, a non-power-of-two block count among them (an odd run at a merge level)."""
    k = block_len()
    return {
        'lanes': [0, 1, 2, 3, 31, 32, 33, 63, 64],
        'lanes8': [5, 0, 8, 7, 1],
        'block': [65, 127, 129, 0, 64, 3],
        'edge-': [k - 1, 2, k],
        'edge+': [k + 1, 0, 2 * k + 1],
        'five': [33, 5 * k + 3],
        'empty': [0, 0, 0],
        'one': [129],
    }


# (name, dtype, hidden, data)
CONFIGS = [
    ('f32-1d-ties', F32, (), 'ties'),
    ('f32-1d-special', F32, (), 'special'),
    ('f32-h1', F32, (1,), 'special'),
    ('f32-h3', F32, (3,), 'ties'),
    ('f16-h8', F16, (8,), 'special'),
    ('f32-h33', F32, (33,), 'ties'),
    ('bf16-2x5', BF16, (2, 5), 'special'),
    ('f64-h2', F64, (2,), 'special'),
    ('i64-1d', I64, (), 'extremes'),
    ('i64-1d-ties', I64, (), 'ties'),
]


def LT(values):
    return torch.tensor(list(values), dtype=torch.long)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_BITS[t.element_size()]) if t.dtype != BOOL else t.view(torch.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def split(x, lens):
    return list(x.split(lens.tolist()))


def draw(n, dtype, hidden, data, lens, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + tuple(hidden)
    if data == 'ties':
        return torch.randint(0, 4, shape, generator=g).to(dtype)
    if data == 'extremes':
        x = torch.randint(-2 ** 62, 2 ** 62, shape, generator=g)
        flat = x.view(-1)
        flat[torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 7)]] = torch.iinfo(I64).min
        flat[torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 7)]] = torch.iinfo(I64).max
        return x
    x = torch.randn(shape, generator=g).to(dtype)
    flat = x.view(-1)
    for value in (float('nan'), float('inf'), float('-inf'), 0.0, -0.0, 1.0):
        if flat.numel():
            flat[torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 9)]] = value
    # NaNs with distinct payload bits, and one sequence that is all NaN
    ib = x.view(_BITS[x.element_size()]).view(-1)
    nan_at = torch.isnan(flat).nonzero().view(-1)
    if nan_at.numel():
        ib[nan_at] = ib[nan_at] | (torch.arange(nan_at.numel()) % 5 + 1).to(ib.dtype)
        ib[nan_at[::2]] = ib[nan_at[::2]] | torch.iinfo(ib.dtype).min            # some negative NaNs
    off = [0] + torch.cumsum(lens, 0).tolist()
    for b, length in enumerate(lens.tolist()):
        if 2 <= length <= 200:
            x[off[b]:off[b + 1]] = float('nan')
            break
    assert torch.isnan(x).sum() == torch.isnan(flat).sum()
    return x


def ref_sort(x, lens, descending):
    """(values, indices) in cat order: stock torch.sort of every sequence on the CPU."""
    vs, ix = [], []
    for s in split(x, lens):
        if s.shape[0] == 0:
            vs.append(s)
            ix.append(torch.zeros(s.shape, dtype=I64))
            continue
        v, i = torch.sort(s, dim=0, stable=True, descending=descending)
        vs.append(v)
        ix.append(i)
    return torch.cat(vs), torch.cat(ix)


def build(kind, x, lens, fill=0):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.with_host_sizes(x.to(DEV), lens)
    return {'C': lambda: c, 'L': lambda: c.left(fill), 'R': lambda: c.right(fill), 'P': c.pack}[kind]()


def pad_fill(dtype):
    return float('nan') if dtype.is_floating_point else 7


_REF = {}


def case(cfg, batch, descending):
    """(x, lens, reference values, reference indices), computed once and shared."""
    key = (cfg, batch, descending)
    if key not in _REF:
        name, dtype, hidden, data = next(c for c in CONFIGS if c[0] == cfg)
        lens = LT(batches()[batch])
        x = draw(int(lens.sum()), dtype, hidden, data, lens, seed=zlib.crc32(repr(key).encode()))
        _REF[key] = (x, lens) + ref_sort(x, lens, descending)
    return _REF[key]


def check_sort(cfg, batch, descending, kinds=KINDS):
    x, lens, want_v, want_i = case(cfg, batch, descending)
    for kind in kinds:
        z = build(kind, x, lens, pad_fill(x.dtype))
        before = z.data.clone()
        out = z.sort(descending=descending)
        what = f'{cfg} {batch} desc={descending} {kind}'
        assert isinstance(out, ta.SeqSort) and type(out.values) is type(z) and type(out.indices) is type(z), what
        assert out.values.data.dtype == x.dtype and out.indices.data.dtype == I64, what
        assert out.values.data.shape == z.data.shape == out.indices.data.shape, what
        if kind == 'P':
            assert out.values.batch_sizes is z.batch_sizes and out.indices.sorted_indices is z.sorted_indices, what
        else:
            assert out.values.token_sizes is z.token_sizes and out.indices.token_sizes is z.token_sizes, what
        assert same_bits(z.data, before), f'{what}: the input changed'
        # the same reference, cast by the library's row movers with zero padding: values, indices, padding rows at once
        assert same_bits(out.values.data, build(kind, want_v, lens, 0).data), f'{what}: values'
        assert torch.equal(out.indices.data, build(kind, want_i, lens, 0).data), f'{what}: indices'
        assert torch.equal(z.argsort(descending=descending).data, out.indices.data), f'{what}: argsort'
        again = z.reorder(out.indices, inverse=False)               # per element: the indices have the storage shape
        assert same_bits(again.data, out.values.data), f'{what}: reorder(argsort) is not sort().values'
        if kind == 'C':
            sv, si = ta.segment_sort(z.data, z.token_sizes, descending=descending)
            assert same_bits(sv, out.values.data) and torch.equal(si, out.indices.data), what
            assert torch.equal(ta.segment_argsort(z.data, z.token_sizes, descending=descending), si), what


@pytest.mark.parametrize('descending', [False, True])
@pytest.mark.parametrize('cfg', [c[0] for c in CONFIGS])
def test_short_and_medium_sequences_match_torch_sort(cfg, descending):
    for batch in ('lanes', 'lanes8', 'block', 'empty', 'one'):
        check_sort(cfg, batch, descending)


@pytest.mark.parametrize('descending', [False, True])
@pytest.mark.parametrize('batch', ['edge-', 'edge+', 'five'])
@pytest.mark.parametrize('cfg', ['f32-1d-ties', 'f32-h3', 'f16-h8', 'i64-1d', 'bf16-2x5'])
def test_block_boundaries_and_merge_passes_match_torch_sort(cfg, batch, descending):
    check_sort(cfg, batch, descending)


@pytest.mark.parametrize('cfg', ['f32-1d-special', 'f32-h33', 'f64-h2', 'i64-1d-ties'])
def test_merge_passes_other_widths(cfg):
    check_sort(cfg, 'edge+', False, kinds='CP')
    check_sort(cfg, 'five', True, kinds='LR')


def test_a_payload_whose_base_is_only_8_byte_aligned():
    for batch in ('lanes', 'block', 'edge+'):
        x, lens, want_v, want_i = case('f32-1d-ties', batch, False)
        buf = torch.empty(x.numel() + 2, dtype=F32, device=DEV)
        data = buf[2:]
        data.copy_(x)
        assert data.data_ptr() % 16 == 8
        c = ta.with_host_sizes(data, lens)
        out = c.sort()
        assert same_bits(out.values.data, want_v) and torch.equal(out.indices.data.cpu(), want_i), batch
        rows = c.reorder(c.argsort())                               # 1-D payload: whole rows of 4 bytes
        assert same_bits(rows.data, want_v), batch


def test_device_only_lengths_take_the_same_bits():
    """A CattedSequence whose lengths the host never saw is planned by its row count: other forms, the same result."""
    for batch in ('lanes', 'edge+'):
        x, lens, want_v, want_i = case('f32-h3', batch, True)
        out = ta.C(x.to(DEV), lens.to(DEV)).sort(descending=True)
        assert same_bits(out.values.data, want_v) and torch.equal(out.indices.data.cpu(), want_i), batch


def test_every_form_is_reached():
    k = block_len()
    assert k == 2048
    x, lens, _, _ = case('f32-1d-ties', 'lanes', False)
    with dispatch_trace() as t:
        build('C', x, lens).sort()
    assert len(t.matching('seg_sort_lanes_kernel G=64')) == 1 and not t.matching('seg_sort_merge_kernel'), t.records
    x, lens, _, _ = case('f32-1d-ties', 'lanes8', False)
    with dispatch_trace() as t:
        build('P', x, lens).argsort()
    assert len(t.matching('seg_sort_lanes_kernel G=8 values=0')) == 1, t.records
    x, lens, _, _ = case('f32-1d-ties', 'edge-', False)
    with dispatch_trace() as t:
        build('L', x, lens).sort()
    assert len(t.matching('seg_sort_block_kernel passes=0')) == 1 and not t.matching('seg_sort_merge_kernel'), t.records
    x, lens, _, _ = case('f32-1d-ties', 'five', False)
    with dispatch_trace() as t:
        build('R', x, lens).sort()
    assert len(t.matching('seg_sort_block_kernel passes=3')) == 1 and len(t.matching('seg_sort_merge_kernel')) == 3, t.records


# ------------------------------------------------------------------ reorder
def perm_indices(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(n, generator=g) for n in lens.tolist()] + [torch.zeros(0, dtype=I64)])


def gather_ref(x, idx, lens):
    return torch.cat([s[i] for s, i in zip(split(x, lens), split(idx, lens))] + [x[:0]])


@pytest.mark.parametrize('dtype,hidden', [(I8, (7,)), (BF16, (512,)), (BOOL, ()), (F16, ()), (F32, ()), (I64, ()),
                                          (I8, ()), (F64, (3,)), (F32, (4,))])
def test_reorder_rows_and_its_inverse(dtype, hidden):
    lens = LT([0, 5, 1, 64, 130, 0, 33])
    n = int(lens.sum())
    g = torch.Generator().manual_seed(3)
    if dtype == BOOL:
        x = torch.rand((n,) + hidden, generator=g) < 0.5
    elif dtype.is_floating_point:
        x = torch.randn((n,) + hidden, generator=g).to(dtype)
    else:
        x = torch.randint(-100, 100, (n,) + hidden, generator=g).to(dtype)
    idx = perm_indices(lens, 5)
    want = gather_ref(x, idx, lens)
    for kind in KINDS:
        z = build(kind, x, lens, 1)
        zi = build(kind, idx, lens, -3)                             # padding rows of the index hold garbage: never read
        out = z.reorder(zi)
        assert type(out) is type(z) and same_bits(out.data, build(kind, want, lens, 0).data), (kind, dtype)
        assert same_bits(z.reorder(zi.data).data, out.data), kind   # the index as a plain tensor
        back = out.reorder(zi, inverse=True)
        assert same_bits(back.data, build(kind, x, lens, 0).data), (kind, dtype, 'inverse')
        fwd = z.reorder(zi, inverse=True)                           # the scatter on its own: out[idx[t]] = z[t]
        inv = torch.cat([torch.argsort(i) for i in split(idx, lens)] + [idx[:0]])
        assert same_bits(fwd.data, build(kind, gather_ref(x, inv, lens), lens, 0).data), (kind, dtype, 'scatter')


def test_reorder_per_element_and_its_inverse():
    lens = LT([3, 0, 70, 9])
    n, H = int(lens.sum()), 5
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, H, generator=g)
    idx = torch.stack([perm_indices(lens, 20 + h) for h in range(H)], dim=1)
    want = torch.cat([torch.take_along_dim(s, i, dim=0) for s, i in zip(split(x, lens), split(idx, lens))])
    for kind in KINDS:
        z, zi = build(kind, x, lens, float('nan')), build(kind, idx, lens, 99)
        out = z.reorder(zi)
        assert same_bits(out.data, build(kind, want, lens, 0).data), kind
        assert same_bits(out.reorder(zi, inverse=True).data, build(kind, x, lens, 0).data), kind


def test_out_of_range_positions_give_zeros():
    """Positions one past the end of sequences that are neither the last nor the longest (inside every allocation even
    for a wrong kernel) and -1 in a sequence that is not the first: zeros in the gather, dropped by the scatter."""
    lens = LT([4, 6, 3, 7])
    n, off = 20, [0, 4, 10, 13]
    x = torch.arange(1, n + 1, dtype=F32)
    idx = perm_indices(lens, 2)
    idx[1] = 4                                                      # sequence 0: len
    idx[6] = -1                                                     # sequence 1
    idx[11] = 3                                                     # sequence 2: len
    bad = torch.zeros(n, dtype=torch.bool)
    bad[[1, 6, 11]] = True
    safe = torch.where(bad, torch.zeros_like(idx), idx)
    want = torch.where(bad, torch.zeros(n), gather_ref(x, safe, lens))
    for kind in KINDS:
        z, zi = build(kind, x, lens, 5.0), build(kind, idx, lens, 0)
        assert same_bits(z.reorder(zi).data, build(kind, want, lens, 0).data), kind
        wide = build(kind, torch.stack([x, -x], dim=1), lens, 5.0)
        want2 = torch.stack([want, torch.where(bad, torch.zeros(n), -gather_ref(x, safe, lens))], dim=1)   # +0.0, not -0.0
        assert same_bits(wide.reorder(zi).data, build(kind, want2, lens, 0).data), kind
        scattered = z.reorder(zi, inverse=True).cat().data.cpu()
        exp = torch.zeros(n)
        for b, (s, i) in enumerate(zip(split(x, lens), split(idx, lens))):
            for t, p in enumerate(i.tolist()):
                if 0 <= p < s.shape[0]:
                    exp[off[b] + p] = s[t]
        assert torch.equal(scattered, exp), kind
    torch.cuda.synchronize()


# ------------------------------------------------------------------ topk
@pytest.mark.parametrize('largest', [True, False])
@pytest.mark.parametrize('k', [0, 1, 3, 100])
def test_topk_matches_torch_topk(k, largest):
    lens = LT([0, 1, 2, 5, 64, 130])
    n = int(lens.sum())
    g = torch.Generator().manual_seed(9)
    x = torch.stack([torch.randperm(n, generator=g).float(), -torch.randperm(n, generator=g).float()], dim=1)   # distinct
    want = [torch.topk(s, min(k, s.shape[0]), dim=0, largest=largest) for s in split(x, lens)]
    new_lens = LT(min(k, v) for v in lens.tolist())
    wv, wi = torch.cat([w.values for w in want]), torch.cat([w.indices for w in want])
    for kind in KINDS:
        out = build(kind, x, lens, float('nan')).topk(k, largest=largest)
        assert isinstance(out, ta.SeqSort), kind
        for got, exp in ((out.values, wv), (out.indices, wi)):
            c = got.cat()
            assert c.token_sizes.cpu().tolist() == new_lens.tolist(), (kind, k)
            assert same_bits(c.data, exp), (kind, k)
            assert same_bits(got.data, build(kind, exp, new_lens, 0).data), (kind, k)


# ------------------------------------------------------------------ gradients
def with_leaf(z):
    leaf = z.data.detach().clone().requires_grad_(True)
    if isinstance(z, ta.P):
        return leaf, ta.P(leaf, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return leaf, z._replace(data=leaf)


@pytest.mark.parametrize('batch', ['block', 'edge+'])
def test_sort_gradient_is_exact(batch):
    x, lens, _, _ = case('f32-h3', batch, True)
    g = torch.Generator().manual_seed(4)
    w = torch.randn(x.shape, generator=g)
    xc = x.clone().requires_grad_(True)
    ref = torch.cat([torch.sort(s, dim=0, stable=True, descending=True)[0] for s in split(xc, lens)])
    (ref * w).sum().backward()
    for kind in KINDS:
        leaf, z = with_leaf(build(kind, x, lens, float('nan')))
        out = z.sort(descending=True)
        assert out.values.data.requires_grad and not out.indices.data.requires_grad, kind
        out.values.data.backward(build(kind, w, lens, float('nan')).data)       # NaN cotangents in the padding rows
        assert same_bits(leaf.grad, build(kind, xc.grad, lens, 0).data), kind   # exact, padding rows exact zeros


def test_reorder_gradient_is_exact_and_goes_to_the_payload_only():
    lens = LT([3, 0, 70, 9])
    n = int(lens.sum())
    g = torch.Generator().manual_seed(12)
    x, w = torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g)
    rows = perm_indices(lens, 31)
    elems = torch.stack([perm_indices(lens, 40 + h) for h in range(4)], dim=1)
    for idx in (rows, elems):
        for inverse in (False, True):
            xc = x.clone().requires_grad_(True)
            parts = []
            for s, i in zip(split(xc, lens), split(idx, lens)):
                i2 = i if i.dim() == 2 else i[:, None].expand(-1, 4)
                parts.append(torch.zeros_like(s).scatter(0, i2, s) if inverse else torch.take_along_dim(s, i2, dim=0))
            (torch.cat(parts) * w).sum().backward()
            for kind in KINDS:
                leaf, z = with_leaf(build(kind, x, lens, float('nan')))
                zi = build(kind, idx, lens, 0)
                out = z.reorder(zi, inverse=inverse)
                assert same_bits(out.data.detach(), build(kind, torch.cat(parts).detach(), lens, 0).data), (kind, inverse)
                out.data.backward(build(kind, w, lens, float('nan')).data)
                assert same_bits(leaf.grad, build(kind, xc.grad, lens, 0).data), (kind, inverse, idx.dim())
                assert zi.data.grad is None


def test_second_order_on_float64():
    lens = LT([3, 0, 4])
    g = torch.Generator().manual_seed(6)
    x = torch.randperm(14, generator=g).double().view(7, 2) / 3          # distinct: the sort is differentiable there
    for kind in 'CLP':
        z = build(kind, x, lens, 100.0)
        leaf, _ = with_leaf(z)

        def values(t, z=z):
            zz = ta.P(t, z.batch_sizes, z.sorted_indices, z.unsorted_indices) if kind == 'P' else z._replace(data=t)
            return zz.sort(descending=True).values.data

        def moved(t, z=z):
            zz = ta.P(t, z.batch_sizes, z.sorted_indices, z.unsorted_indices) if kind == 'P' else z._replace(data=t)
            idx = zz.argsort()
            return zz.reorder(idx).data * zz.reorder(idx, inverse=True).data

        assert torch.autograd.gradcheck(values, (leaf,), eps=1e-6, atol=1e-7)
        assert torch.autograd.gradgradcheck(values, (leaf,), eps=1e-6, atol=1e-7)
        assert torch.autograd.gradcheck(moved, (leaf,), eps=1e-6, atol=1e-7)
        assert torch.autograd.gradgradcheck(moved, (leaf,), eps=1e-6, atol=1e-7)


def test_int64_passes_through_without_a_graph():
    x, lens, want_v, _ = case('i64-1d', 'block', False)
    out = build('C', x, lens).sort()
    assert not out.values.data.requires_grad and out.values.data.grad_fn is None and same_bits(out.values.data, want_v)
