"""Per-sequence compress on the GPU, bit for bit: every container against the yardstick of tests/compress_util.py (plain
torch on the CPU), the two commutation identities field by field (PackedSequence metadata included), wave and block
boundaries, the cut form against the uncut one, every row width class, padding, device-only lengths, strided inputs,
autograd of every order, and the dispatch trace for every kernel form.  No tolerance anywhere: rows move as bits and
floats are compared through an integer view."""
import pytest
import torch

import torchrua_amd as ta
from compress_util import bits, compress_cat, compress_grad_cat, keep, padded, same_bits, split
from gpu_util import DEV, dispatch_trace

pytestmark = pytest.mark.gpu

BLOCK = 2048                                   # SEG_BLOCK_TOK of csrc/rua_seg_plan.h
WAVE_LENS = [0, 1, 7, 63, 64, 65, 129]         # around the wave boundaries (bound 129: the plan's rows form)
SHORT_LENS = [64, 0, 1, 7, 63, 33, 32, 2, 64]  # bound 64: the plan's lanes form (more than one workgroup's 8 sequences)
BF16, F32, F64, I64, BOOL = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.bool
# (dtype, hidden, row bytes)
WIDTHS = [(BOOL, (), 1), (BF16, (1,), 2), (I64, (), 8), (F32, (4,), 16), (F32, (5,), 20), (F32, (32,), 128),
          (F32, (33,), 132), (BF16, (512,), 1024), (F32, (2, 3), 24)]
MASKS = ('all', 'none', 'first', 'last', 'bernoulli')


# ------------------------------------------------------------------ helpers
def LT(values):
    return torch.tensor(list(values), dtype=torch.long)


def draw(shape, dtype, seed):
    """Random payload on the CPU; floats carry a few NaNs and infinities (rows are bits: they must survive)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == BOOL:
        return torch.rand(shape, generator=g) < 0.5
    if dtype == I64:
        return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g)
    x = torch.randn(shape, generator=g).to(dtype)
    flat = x.view(-1)
    if flat.numel() >= 8:
        flat[1], flat[flat.numel() // 2], flat[-2] = float('nan'), float('inf'), float('-inf')
    return x


def draw_mask(kind, lens, seed):
    n = int(lens.sum())
    if kind == 'all':
        return torch.ones(n, dtype=BOOL)
    m = torch.zeros(n, dtype=BOOL)
    if kind == 'bernoulli':
        return torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.5
    off = 0
    for length in lens.tolist():
        if length and kind == 'first':
            m[off] = True
        if length and kind == 'last':
            m[off + length - 1] = True
        off += length
    return m


def build(kind, x, lens, fill=0, device_lens=False):
    """The container of `kind` over C(x, lens), through the library's own casts (they only move rows)."""
    c = ta.C(x.to(DEV), lens.to(DEV)) if device_lens else ta.with_host_sizes(x.to(DEV), lens)
    return {'C': lambda: c, 'L': lambda: c.left(fill), 'R': lambda: c.right(fill), 'P': c.pack}[kind]()


def mask_like(kind, mask, lens, device_lens=False):
    """The mask cast the same way as the data; padding rows of an L / R hold True (they must be ignored)."""
    return build(kind, mask, lens, fill=True, device_lens=device_lens).data


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def same_fields(a, b, what):
    assert type(a) is type(b), what
    assert same_bits(a.data, b.data), f'{what}: data {tuple(a.data.shape)} vs {tuple(b.data.shape)}'
    if isinstance(a, ta.P):
        assert a.batch_sizes.dtype == b.batch_sizes.dtype and torch.equal(a.batch_sizes.cpu(), b.batch_sizes.cpu()), what
        assert torch.equal(a.sorted_indices, b.sorted_indices) and torch.equal(a.unsorted_indices, b.unsorted_indices), what
    else:
        assert a.token_sizes.dtype == b.token_sizes.dtype == I64 and torch.equal(a.token_sizes, b.token_sizes), what


def check(kind, x, mask, lens, what, device_lens=False):
    """z.compress(m) against the yardstick and both commutation identities; returns the result."""
    z, m = build(kind, x, lens, device_lens=device_lens), mask_like(kind, mask, lens, device_lens)
    x_before, m_before = z.data.clone(), m.clone()
    out = z.compress(m)
    what = f'{what} {kind}'
    assert type(out) is type(z) and out.data.dtype == x.dtype, what
    assert same_bits(z.data, x_before) and torch.equal(m, m_before), f'{what}: an input changed'
    assert out.data.untyped_storage().data_ptr() != z.data.untyped_storage().data_ptr() or out.data.numel() == 0, what
    want, want_lens = compress_cat(x, mask, lens)
    kept = keep(split(x, lens), split(mask, lens))
    # the yardstick, in cat form and in the container's own storage (T' = the longest new sequence, zero padding)
    got = out.cat()
    assert same_bits(got.data, want), f'{what}: payload'
    assert got.token_sizes.dtype == I64 and got.token_sizes.cpu().tolist() == want_lens.tolist(), f'{what}: lengths'
    if kind in 'LR':
        assert same_bits(out.data, padded(kept, x, right=kind == 'R')), f'{what}: padded storage'
    # z.compress(m) == z.cat().compress(m_as_cat).X(), and z.compress(m).cat() == z.cat().compress(m_as_cat)
    zc = z.cat()
    mc = mask.to(DEV) if kind == 'C' else rewrap(z, m).cat().data
    ref = zc.compress(mc)
    same_fields(out, {'C': lambda: ref, 'L': ref.left, 'R': ref.right, 'P': ref.pack}[kind](), f'{what}: X(compress(cat))')
    same_fields(got, ref, f'{what}: cat(compress)')
    return out


# ------------------------------------------------------------------ every width, mask and layout at the wave boundaries
@pytest.mark.parametrize('dtype,hidden,row_bytes', WIDTHS, ids=[f'{rb}B' for _, _, rb in WIDTHS])
def test_widths_masks_layouts(dtype, hidden, row_bytes):
    lens = LT(WAVE_LENS)
    x = draw((int(lens.sum()),) + hidden, dtype, seed=row_bytes)
    assert x[0].numel() * x.element_size() == row_bytes
    for i, mk in enumerate(MASKS):
        mask = draw_mask(mk, lens, seed=10 + i)
        for kind in 'CLPR':
            out = check(kind, x, mask, lens, f'{row_bytes}B {mk}')
            if mk == 'all':                                       # the identity, metadata included
                same_fields(out, build(kind, x, lens), f'{row_bytes}B all-true {kind}')
            if mk == 'none':                                      # everything empty: the containers still construct
                assert out.data.shape[0] == (0 if kind in 'CP' else len(WAVE_LENS)) and out.data.numel() == 0
                assert out.cat().token_sizes.cpu().tolist() == [0] * len(WAVE_LENS)
                if kind == 'P':
                    assert out.batch_sizes.numel() == 0 and out.sorted_indices.numel() == len(WAVE_LENS)


def test_segment_compress_is_the_cat_form():
    lens = LT(WAVE_LENS)
    x, mask = draw((int(lens.sum()), 5), F32, 3), draw_mask('bernoulli', lens, 4)
    data, sizes = ta.segment_compress(x.to(DEV), mask.to(DEV), lens.to(DEV))
    want, want_lens = compress_cat(x, mask, lens)
    assert same_bits(data, want) and sizes.dtype == I64 and sizes.cpu().tolist() == want_lens.tolist()


def test_the_new_lengths_carry_their_host_copy():
    """The operator reads the lengths back once and attaches the copy: the next pack() / left() reads nothing back."""
    from torchrua_amd import _meta as M
    lens = LT(WAVE_LENS)
    x, mask = draw((int(lens.sum()), 5), F32, 5), draw_mask('bernoulli', lens, 6)
    out = build('C', x, lens).compress(mask.to(DEV))
    host = M._memo_get(out.token_sizes, 'host')
    assert host is not None and not host.is_cuda and host.tolist() == compress_cat(x, mask, lens)[1].tolist()


# ------------------------------------------------------------------ the plan's forms: lanes, rows, long, cut
def test_short_sequences_take_the_lanes_plan():
    lens = LT(SHORT_LENS)
    x, mask = draw((int(lens.sum()), 5), F32, 7), draw_mask('bernoulli', lens, 8)
    for kind in 'CLPR':
        with dispatch_trace() as tr:
            check(kind, x, mask, lens, 'short')
        assert tr.matching('seg_compress_plan_kernel form=lanes G=32'), tr.records
    with dispatch_trace() as tr:
        check('C', x, mask, LT([0, 1, 7, 63, 64, 65, 66]), 'bound 66')       # the same 266 rows, other lengths
    assert tr.matching('seg_compress_plan_kernel form=rows G=64') and not tr.matching('seg_compress_plan_kernel form=lanes')


def test_sequences_across_blocks_take_the_long_plan():
    lens = LT([3, BLOCK + 1, 0, 2 * BLOCK + 1, 65])
    for dtype, hidden in ((F32, (5,)), (BF16, ())):
        x = draw((int(lens.sum()),) + hidden, dtype, 9)
        for mk in ('bernoulli', 'last', 'all'):
            mask = draw_mask(mk, lens, 11)
            for kind in 'CLPR':
                with dispatch_trace() as tr:
                    check(kind, x, mask, lens, f'long {mk}')
                assert tr.matching('seg_compress_plan_kernel form=long G=256 cut=0'), tr.records
                assert not tr.matching('seg_compress_plan_kernel form=cut')


def test_device_only_lengths():
    """C(data, token_sizes_on_device): the host never saw the lengths, the bound is the row count (the long plan)."""
    lens = LT(WAVE_LENS + [BLOCK + 5])
    x, mask = draw((int(lens.sum()), 5), F32, 12), draw_mask('bernoulli', lens, 13)
    for kind in 'CLPR':
        check(kind, x, mask, lens, 'device lengths', device_lens=True)
    with dispatch_trace() as tr:
        ta.C(x.to(DEV), lens.to(DEV)).compress(mask.to(DEV))
    assert tr.matching('seg_compress_plan_kernel form=long'), tr.records


def test_cut_equals_uncut():
    """B = 2 long sequences are cut across workgroups (two plan launches, a cut move); the same two among 1 024 short
    ones are not.  The two long sequences' results must be the same bits."""
    long_lens = [4 * BLOCK + 3, 8 * BLOCK]
    n_long = sum(long_lens)
    extra = 1024
    for dtype, hidden in ((F32, (8,)), (I64, ()), (F32, (33,))):
        x = draw((n_long + extra,) + hidden, dtype, 14)
        for mk in ('bernoulli', 'last'):
            mask_long = draw_mask(mk, LT(long_lens), 15)
            mask = torch.cat([mask_long, draw_mask('bernoulli', LT([1] * extra), 16)])
            want, want_lens = compress_cat(x[:n_long], mask_long, LT(long_lens))
            for kind in 'CLPR':
                with dispatch_trace() as tr:
                    cut = check(kind, x[:n_long], mask_long, LT(long_lens), f'cut {mk}')
                assert tr.matching('seg_compress_plan_kernel form=cut phase=count blocks=8'), tr.records
                assert tr.matching('seg_compress_plan_kernel form=cut phase=finish blocks=8'), tr.records
                if hidden:
                    assert tr.matching('seg_compress_move_rows_kernel expand=0 cut=1'), tr.records
                if kind in 'LR':
                    continue                                     # (1 026 padded rows of 16 384 tokens: gigabytes)
                with dispatch_trace() as tr:
                    whole = build(kind, x, LT(long_lens + [1] * extra)).compress(
                        mask_like(kind, mask, LT(long_lens + [1] * extra)))
                assert not tr.matching('seg_compress_plan_kernel form=cut') and tr.matching('seg_compress_plan_kernel form=long')
                assert not tr.matching('seg_compress_move_rows_kernel cut=1'), tr.records
                wc = whole.cat()
                n_kept = int(want_lens.sum())
                assert wc.token_sizes[:2].cpu().tolist() == want_lens.tolist()
                assert same_bits(wc.data[:n_kept], want) and same_bits(cut.cat().data, want), f'{kind} {mk}'


# ------------------------------------------------------------------ padding, strides
def test_padded_storage_wider_than_the_longest_sequence():
    """An L / R with T_phys above the longest sequence and an all-true [B, T] mask: the identity on the tokens; padding
    rows of the input (NaN here) are never kept, padding rows of the result are zero bits."""
    lens = LT([3, 0, 9, 5])
    B, T, T_phys = 4, 9, 12
    for dtype, hidden in ((F32, (5,)), (BF16, ())):
        x = draw((int(lens.sum()),) + hidden, dtype, 17)
        seqs = split(x, lens)
        for right in (False, True):
            data = torch.full((B, T_phys) + hidden, float('nan'), dtype=dtype)
            for b, s in enumerate(seqs):
                n = s.shape[0]
                data[b, (T - n if right else 0):(T if right else n)] = s
            z = (ta.R if right else ta.L)(data.to(DEV), lens.to(DEV))
            out = z.compress(torch.ones(B, T_phys, dtype=BOOL, device=DEV))
            assert same_bits(out.data, padded(seqs, x, right=right)) and out.token_sizes.cpu().tolist() == lens.tolist()
            m = torch.rand(B, T_phys, generator=torch.Generator().manual_seed(18)) < 0.5
            out = z.compress(m.to(DEV))
            kept = [s[m[b, (T - s.shape[0] if right else 0):(T if right else s.shape[0])]] for b, s in enumerate(seqs)]
            assert same_bits(out.data, padded(kept, x, right=right)), ('R' if right else 'L', dtype)


def test_non_contiguous_payload_and_mask():
    lens = LT(WAVE_LENS)
    n = int(lens.sum())
    wide, pair = draw((n, 10), F32, 19).to(DEV), torch.stack([draw_mask('bernoulli', lens, 20)] * 2, dim=1).to(DEV)
    x, mask = wide[:, ::2], pair[:, 1]
    assert not x.is_contiguous() and not mask.is_contiguous()
    out = ta.C(x, lens.to(DEV)).compress(mask)
    want, want_lens = compress_cat(x.cpu(), mask.cpu(), lens)
    assert same_bits(out.data, want) and out.token_sizes.cpu().tolist() == want_lens.tolist()
    l = ta.C(x, lens.to(DEV)).left()
    ml = ta.C(mask, lens.to(DEV)).left()
    out = ta.L(l.data.transpose(0, 1).contiguous().transpose(0, 1), l.token_sizes).compress(
        ml.data.transpose(0, 1).contiguous().transpose(0, 1))
    assert same_bits(out.cat().data, want)


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_gradient_is_the_yardsticks_bit_for_bit(dtype):
    """d (z.compress(m).data * w).sum() / d z.data: w at the kept tokens, exact zeros at dropped tokens — NaN and inf
    planted there — and at padding rows.  Rows of 2 / 4 bytes take the lanes move, 18 / 36 bytes the rows move."""
    lens = LT(WAVE_LENS)
    for hidden in ((), (9,)):
        form = 'lanes' if not hidden else 'rows'
        x = torch.randn((int(lens.sum()),) + hidden, generator=torch.Generator().manual_seed(21)).to(dtype)
        mask = draw_mask('bernoulli', lens, 22)
        dropped = (~mask).nonzero().reshape(-1)
        x[dropped[0::2]], x[dropped[1::2]] = float('nan'), float('inf')
        for kind in 'CLPR':
            z, m = build(kind, x, lens, fill=float('nan')), mask_like(kind, mask, lens)
            leaf = z.data.clone().requires_grad_(True)
            with dispatch_trace() as tr:
                out = rewrap(z, leaf).compress(m)
                w = torch.randn(out.data.shape, generator=torch.Generator().manual_seed(23)).to(dtype).to(DEV)
                (out.data * w).sum().backward()
            assert tr.matching(f'seg_compress_move_{form}_kernel expand=0') and tr.matching(f'seg_compress_move_{form}_kernel expand=1'), tr.records
            assert len(tr.matching('seg_compress_plan_kernel')) == 1, 'the backward counts nothing again'
            w_kept = rewrap(out, w).cat().data.cpu()
            want = compress_grad_cat(mask, w_kept, lens, x)
            assert leaf.grad.dtype == dtype and same_bits(leaf.grad, build(kind, want, lens).data), (kind, hidden)
            assert same_bits(rewrap(z, leaf.grad).cat().data[~mask.to(DEV)], torch.zeros_like(x[~mask])), 'dropped: true zeros'


def test_gradcheck_and_double_backward():
    lens = LT([3, 0, 5])
    mask = torch.tensor([True, False, True, False, True, True, False, True])
    x = torch.randn(8, 2, dtype=F64, generator=torch.Generator().manual_seed(24))
    for kind in 'CLPR':
        z, m = build(kind, x, lens), mask_like(kind, mask, lens)
        leaf = z.data.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda d: rewrap(z, d).compress(m).data, (leaf,), nondet_tol=0.0)
        assert torch.autograd.gradgradcheck(lambda d: rewrap(z, d).compress(m).data, (leaf,), nondet_tol=0.0)
        # create_graph: the gradient is expand(cotangent), and the double backward of a cotangent is compress of it
        out = rewrap(z, leaf).compress(m)
        cot = torch.randn(out.data.shape, dtype=F64, device=DEV).requires_grad_(True)
        g, = torch.autograd.grad(out.data, leaf, cot, create_graph=True)
        assert g.requires_grad and g.shape == leaf.shape
        v = torch.randn(leaf.shape, dtype=F64, device=DEV)
        gg, = torch.autograd.grad(g, cot, v)
        assert same_bits(gg, rewrap(z, v).compress(m).data), kind


def test_integer_and_bool_payloads_carry_no_graph():
    lens = LT(WAVE_LENS)
    mask = draw_mask('bernoulli', lens, 25)
    for dtype in (I64, BOOL):
        x = draw((int(lens.sum()),), dtype, 26)
        with torch.enable_grad():
            out = build('P', x, lens).compress(mask_like('P', mask, lens))
        assert not out.data.requires_grad and out.data.grad_fn is None and out.data.dtype == dtype
        assert same_bits(out.cat().data, compress_cat(x, mask, lens)[0])


def test_one_read_back_of_the_new_lengths(monkeypatch):
    """Device-only lengths [2, 0, 3], hidden (2,): compress on a C, an L and a P, and segment_compress, each read back
    exactly once — the [3] new lengths — and leave the host copy, the kept counts, on the result's lengths."""
    from torchrua_amd import _meta
    lens, mask = LT([2, 0, 3]), torch.tensor([True, False, True, True, False])
    x = draw((5, 2), F32, 27)
    packed = build('P', x, lens)
    cases = {                                                    # containers from their fields: no cast has read the lengths
        'C': (ta.C(x.to(DEV), lens.to(DEV)), mask.to(DEV)),
        'L': (ta.L(build('L', x, lens).data, lens.to(DEV)), mask_like('L', mask, lens)),
        'P': (ta.P(packed.data, packed.batch_sizes.clone(), packed.sorted_indices, packed.unsorted_indices),
              mask_like('P', mask, lens)),
    }
    torch.cuda.synchronize()
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    for kind, (z, m) in cases.items():
        del calls[:]
        out = z.compress(m)
        assert calls == [(3,)], (kind, calls)
        new = _meta.pack_lens(out) if kind == 'P' else out.token_sizes
        host = _meta._memo_get(new, 'host')
        assert host is not None and not host.is_cuda and host.tolist() == [1, 0, 2], (kind, host)
        assert calls == [(3,)], (kind, calls)
        assert same_bits(out.cat().data, x[mask]), kind
    del calls[:]
    data, new = ta.segment_compress(x.to(DEV), mask.to(DEV), lens.to(DEV))
    assert calls == [(3,)], calls
    host = _meta._memo_get(new, 'host')
    assert host is not None and not host.is_cuda and host.tolist() == [1, 0, 2]
    assert same_bits(data, x[mask])
