"""pack(keep_sums=...) keeps the per-sequence sums of its one pass and reduce_sum(p) reuses them: the PackedSequence is
the plain pack()'s bit for bit, the sums are the two-op path's (pack(keep_sums=False) then reduce_sum), the memo dies
with an in-place write or a re-built PackedSequence, autograd goes through native kernels, and the bench hooks fire.

Shapes sit at the dispatch edges: just below / at reduce.FUSED_MIN_UNITS units, rows of 128 B .. 4 160 B (one lane group
per row, several rows per wave instruction, four column chunks per wave, two units per row), rows off 16 bytes (the
mover packs, no sums), lengths from 1, one sequence beyond the split threshold among 16 384 short ones, sources C / L / R.

Bounds.  The kept sums are the fp32 accumulators, so the fp64 bound of the issue (1e-5 * sum|x|) is asserted on THEM;
what reduce_sum returns must be those accumulators rounded once to the payload dtype (asserted exactly), which for
bf16 / f16 is all a rounded output can promise (half an ulp of the sum is far above 1e-5 * sum|x|).  Against the two-op
path: rtol 2**-7, atol 1e-2 (bench.py's own allclose), and bit-equal whenever the two-op reduce gave every sequence to
one wave walking it whole (its trace says seg_reduce_kernel without a split, and the fused pass did not split either):
then both fold the same rows in the same order."""
import numpy as np
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _ops as O
from torchrua_amd import reduce as R
from gpu_util import DEV, dispatch_trace
from helpers import orc

pytestmark = pytest.mark.gpu

#        name              B      H     dtype            kind  long  keep   fused?
CASES = {
    'below_units':      (16383,   64, torch.bfloat16, 'C',    0, None, False),
    'at_units':         (16384,   64, torch.bfloat16, 'C',    0, None, True),
    'forced_small':     (  300,   64, torch.bfloat16, 'C',    0, True, True),
    'h72':              (16384,   72, torch.bfloat16, 'C',    0, None, True),
    'h68_off_16_bytes': (16384,   68, torch.bfloat16, 'C',    0, None, False),
    'h520_f16':         (16384,  520, torch.float16,  'C',    0, None, True),
    'h1024_f32':        (16384, 1024, torch.float32,  'C',    0, None, True),
    'two_chunks_below': ( 8191, 1040, torch.float32,  'C',    0, None, False),
    'two_chunks':       ( 8192, 1040, torch.float32,  'C',    0, None, True),
    'one_long':         (16384,   64, torch.bfloat16, 'C', 6000, None, True),
    'one_long_f32':     (16384,   64, torch.float32,  'C', 6000, None, True),
    'left':             (16384,   64, torch.float32,  'L',    0, None, True),
    'right':            (16384,   64, torch.float16,  'R',    0, None, True),
}
_made = {}


def _inputs(B, H, dtype, long):
    """(payload [N, H] on the device, host lengths) — made once per shape, never written."""
    key = (B, H, dtype, long)
    if key not in _made:
        g = torch.Generator().manual_seed(B * 7 + H)
        lens = torch.randint(1, 5, (B,), generator=g)
        if long:
            lens[B // 3] = long
        x = torch.randn((int(lens.sum()), H), generator=g).to(dtype)
        _made[key] = (x.to(DEV), lens)
    return _made[key]


def _source(kind, x, lens):
    c = ta.with_host_sizes(x, lens)
    return c if kind == 'C' else (c.left() if kind == 'L' else c.right())


def _same_meta(p, q):
    return (torch.equal(p.batch_sizes, q.batch_sizes) and torch.equal(p.sorted_indices, q.sorted_indices)
            and torch.equal(p.unsorted_indices, q.unsorted_indices))


@pytest.mark.parametrize('case', sorted(CASES))
def test_pack_and_sums_match_the_two_op_path(case):
    B, H, dtype, kind, long, keep, fused = CASES[case]
    x, lens = _inputs(B, H, dtype, long)
    z_plain, z = _source(kind, x, lens), _source(kind, x, lens)           # (the casts to L / R stay out of the traces)
    with dispatch_trace() as two:
        plain = z_plain.pack(keep_sums=False)
        want = ta.reduce_sum(plain)
    assert O.kept_sums(plain) is None
    with dispatch_trace() as one:
        p = z.pack(keep_sums=keep)
        kept = O.kept_sums(p)
        got = ta.reduce_sum(p)
    assert (kept is not None) == fused, one.records
    assert torch.equal(p.data, plain.data) and _same_meta(p, plain)
    assert got.dtype == dtype and got.shape == want.shape == (B, H)
    if fused:
        assert 'seg_reduce_kernel' in one.kernels and all('COPY=1' in r for r in one.records), one.records
        assert ('seg_reduce_tail_kernel' in one.kernels) == bool(long), one.records          # the split is armed when it must
        assert kept.dtype == torch.float32 and torch.equal(got, kept.to(dtype))              # rounded once
    x64 = x.double().cpu().numpy()
    ref = orc.segment_sum(x64, lens.numpy())
    scale = orc.segment_sum(np.abs(x64), lens.numpy())
    acc = (kept if fused else got.float() if dtype == torch.float32 else None)
    if acc is not None:
        err = np.abs(acc.double().cpu().numpy() - ref)
        print(case, 'max |sums - fp64| / sum|x| =', float((err / np.maximum(scale, 1e-300)).max()))
        assert (err <= 1e-5 * scale).all()
    print(case, 'max |fused - two-op| =', float((got.float() - want.float()).abs().max()))
    assert torch.allclose(got.float(), want.float(), rtol=2 ** -7, atol=1e-2)
    whole = [r for r in two.records if r.startswith('seg_reduce')]
    if fused and len(whole) == 1 and whole[0].startswith('seg_reduce_kernel ') and not long:
        assert torch.equal(got, want), 'one wave per sequence on both paths: the same fold, bit for bit'


def _fused(dtype=torch.bfloat16, B=16384, H=64):
    x, lens = _inputs(B, H, dtype, 0)
    return x, lens, ta.with_host_sizes(x, lens).pack()


def test_an_in_place_write_drops_the_kept_sums():
    x, lens, p = _fused(torch.float32)
    assert O.kept_sums(p) is not None
    before = ta.reduce_sum(p)
    p.data.mul_(2)
    assert O.kept_sums(p) is None
    after = ta.reduce_sum(p)
    fresh = ta.reduce_sum(ta.P(p.data.clone(), p.batch_sizes, p.sorted_indices, p.unsorted_indices))
    assert torch.equal(after, fresh)                      # the payload was walked again: the fresh sums of what it holds now
    assert torch.allclose(after, before * 2, rtol=2 ** -7, atol=1e-2) and not torch.equal(after, before)


def test_rebuilt_sequences_take_the_unchanged_path_and_agree():
    x, lens, p = _fused()
    want = ta.reduce_sum(ta.with_host_sizes(x, lens).pack(keep_sums=False))
    rewrapped = ta.P(p.data, p.batch_sizes, p.sorted_indices, p.unsorted_indices)
    cloned = ta.P(p.data.clone(), p.batch_sizes, p.sorted_indices, p.unsorted_indices)
    other_meta = ta.P(p.data, p.batch_sizes.clone(), p.sorted_indices, p.unsorted_indices)
    assert O.kept_sums(cloned) is None and O.kept_sums(other_meta) is None
    for q in (rewrapped, cloned, other_meta):
        assert torch.equal(ta.reduce_sum(q), want)
    assert torch.equal(ta.reduce_mean(p), ta.reduce_mean(cloned)) and torch.equal(ta.reduce_max(p), ta.reduce_max(cloned))


def test_every_call_returns_its_own_tensor():
    x, lens, p = _fused()
    a, b = ta.reduce_sum(p), ta.reduce_sum(p)
    kept = O.kept_sums(p)
    assert a.data_ptr() != b.data_ptr() and a.data_ptr() != kept.data_ptr() and torch.equal(a, b)
    a.zero_()
    assert torch.equal(ta.reduce_sum(p), b)


def _ulps(a, b):
    def ordered(t):
        bits = t.view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7fff), bits)
    return int((ordered(a) - ordered(b)).abs().max())


def _grads(dtype, keep, terms, kind='C', create_graph=False, long=0):
    B, H = 16384, 64
    x, lens = _inputs(B, H, dtype, long)
    g = torch.Generator().manual_seed(11)
    w = torch.randn((B, H), generator=g).to(dtype).to(DEV).requires_grad_(create_graph)
    v = torch.randn((x.size(0), H), generator=g).to(dtype).to(DEV)
    leaf = x.clone().requires_grad_(True)
    p = _source(kind, leaf, lens).pack(keep_sums=keep)
    assert (O.kept_sums(p) is not None) == (keep is not False)
    loss = 0
    if 'sums' in terms:
        loss = loss + (ta.reduce_sum(p) * w).sum()
    if 'data' in terms:
        loss = loss + (p.data * v).sum()
    gx = torch.autograd.grad(loss, leaf, create_graph=create_graph)[0]
    if create_graph:             # ... and once more: d/dw of a function of the first gradient
        return gx, torch.autograd.grad((gx * gx).sum(), w)[0]
    return gx


@pytest.mark.parametrize('kind', ['C', 'L'])
@pytest.mark.parametrize('terms', [('sums', 'data'), ('sums',), ('data',)], ids=['both', 'sums_only', 'data_only'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_backward_matches_the_two_op_path(dtype, terms, kind):
    want = _grads(dtype, False, terms, kind)
    with dispatch_trace() as t:
        got = _grads(dtype, None, terms, kind)
    assert ('pack_sums_backward_kernel' in t.kernels) == (len(terms) == 2), t.records      # both cotangents: ONE kernel
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        assert _ulps(got, want) <= 1


@pytest.mark.parametrize('terms', [('sums', 'data'), ('sums',)], ids=['both', 'sums_only'])
def test_backward_with_one_long_sequence(terms):
    """One sequence of 6 000 rows among 16 384 short ones: the forward splits it, the adjoint of both cotangents walks it
    with one wave (correct at any length; DESIGN 4.0b states the rate), the sums' alone goes one storage row at a time."""
    want = _grads(torch.bfloat16, False, terms, long=6000)
    got = _grads(torch.bfloat16, None, terms, long=6000)
    assert _ulps(got, want) <= 1


def test_create_graph_falls_back_to_the_two_op_pieces():
    want, want_w = _grads(torch.float32, False, ('sums', 'data'), create_graph=True)
    with dispatch_trace() as t:
        got, got_w = _grads(torch.float32, None, ('sums', 'data'), create_graph=True)
    assert 'pack_sums_backward_kernel' not in t.kernels
    assert got.requires_grad and torch.equal(got, want) and torch.equal(got_w, want_w)


def test_one_step_fires_each_hook_once():
    x, lens = _inputs(16384, 64, torch.bfloat16, 0)
    calls = []
    O.set_kernel_hook(lambda name, begin: calls.append((name, begin)))
    try:
        ta.reduce_sum(ta.with_host_sizes(x, lens).pack())
    finally:
        O.set_kernel_hook(None)
    assert calls == [('to_pack', True), ('to_pack', False), ('reduce', True), ('reduce', False)]


def test_threshold_is_the_reducers():
    assert R.fused_units(16384, 128) == R.FUSED_MIN_UNITS and R.fused_units(8192, 4160) == R.FUSED_MIN_UNITS
