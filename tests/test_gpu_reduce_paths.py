"""Every dispatch path of the segmented reduce, each against a float64 restatement of the reference.

`PATHS` holds one row per path: the container and shape that reach it, and the records the dispatch trace
(rua_debug_trace) must show, so that a threshold change that moves a case to another kernel fails here instead of
leaving a kernel untested.  tests/test_reduce_path_table.py checks that every reduce kernel template appears in
some row.

The reference is the reference's own formula (torchrua/reduce.py:34-61) restated in plain torch on the exactly upcast
input: torch.segment_reduce with the global `initial` (tensor.min() / tensor.max()) for max / min, and the max / exp /
sum / log composition with `eps` for logsumexp.  Gradients come from float64 autograd through the same restatement.

Data whose answer does not depend on the order of summation make a dropped, doubled or misassigned row fail at any
length: small integers for sum / mean / max / min (values in {0, 1, 2} half the time, so ties are common), and factors
from {+-1, +-0.5, +-2} for prod.  Sum, max, min and prod must then be bit-equal to the exact value rounded once."""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

import torchrua_amd as ta
from gpu_util import DEV, dispatch_trace
from torchrua_amd import _meta as M

pytestmark = pytest.mark.gpu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
FULL = {F32: 4, BF16: 8, F16: 8, F64: 2}          # elements per 16-byte lane
HALF = {F32: 2, BF16: 4, F16: 4, F64: 1}
HALF_ULP = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11, F64: 2.0 ** -53}   # half an ulp, relative
ACC_ULP = {F32: 2.0 ** -23, BF16: 2.0 ** -23, F16: 2.0 ** -23, F64: 2.0 ** -52}
OPS = ('sum', 'mean', 'max', 'min', 'prod', 'logsumexp')


@dataclasses.dataclass
class Case:
    id: str
    kind: str                 # C (host sizes) | Cdev (lengths on the device only) | seg (segment_*) | L | R | P | fused
    B: int
    lo: int
    hi: int
    row_bytes: int = 0        # hidden = (row_bytes // itemsize,) unless `hidden` is given
    hidden: Optional[Tuple[int, ...]] = None
    fwd: Tuple[str, ...] = ()                 # trace records the forward must show (max / min / logsumexp included)
    bwd: Tuple[str, ...] = ()                 # ... and the backward of sum / max / logsumexp
    dtypes: Tuple[torch.dtype, ...] = (F32, BF16)
    ops: Tuple[str, ...] = OPS
    outlier: int = 0          # one more sequence of this many rows
    empties: bool = True      # a few empty sequences (not for P)
    split: int = 0            # force the long-sequence split (M.reduce_split_rows) to parts of this many rows
    misaligned: bool = False  # the payload starts one element into a flat buffer: contiguous, not 8-byte aligned
    bwd_prod: Tuple[str, ...] = ()            # the records of prod's backward

    def hid(self, dtype):
        return self.hidden if self.hidden is not None else (self.row_bytes // torch.empty(0, dtype=dtype).element_size(),)


PATHS = [
    # adjacent ranks of a sorted PackedSequence share a wave (short form: T <= 128)
    Case('ranks_P_short', 'P', 16400, 1, 10, 256,
         fwd=('seg_reduce_ranks_kernel EPL=FULL glog=0 check=0 split=0',),
         bwd=('seg_backward_ranks_kernel EPL=FULL TV=0', 'seg_backward_ranks_kernel EPL=FULL TV=2'),
         dtypes=(F32, BF16, F16, F64)),
    # (24-byte rows: the forward's 16-byte lanes overlap the row's last half vector; the backward takes 8-byte lanes)
    Case('ranks_P_half', 'P', 70000, 1, 40, 24,
         fwd=('seg_reduce_ranks_kernel EPL=FULL',), bwd=('seg_backward_ranks_kernel EPL=HALF',), dtypes=(F32, BF16)),
    Case('ranks_P_half_8B', 'P', 40000, 1, 10, 8, fwd=('seg_reduce_ranks_kernel EPL=HALF',), dtypes=(F32, BF16)),
    Case('ranks_P_scalar_1d', 'P', 70000, 1, 40, hidden=(),
         fwd=('seg_reduce_ranks_kernel EPL=1',), bwd=('seg_backward_walk_kernel EPL=1',)),
    # ... long form (T > 128): at least 4 096 waves of ranks
    Case('ranks_P_long', 'P', 8200, 1, 20, 512, outlier=200, fwd=('seg_reduce_ranks_kernel EPL=FULL glog=0',)),
    # every row slot of a wave its own sequence of a CattedSequence: the caller's word (SHORT_SEQS) or checked
    Case('ranks_C_hint', 'C', 100000, 1, 8, 16, fwd=('seg_reduce_ranks_kernel EPL=FULL glog=0 check=0 split=0',),
         bwd=('seg_backward_walk_kernel EPL=FULL',)),
    Case('ranks_C_outlier', 'C', 100000, 1, 8, 16, outlier=5000,
         fwd=('seg_reduce_ranks_kernel EPL=FULL glog=0 check=1 split=0',)),
    Case('ranks_C_device_lens', 'Cdev', 100000, 1, 8, 16, fwd=('seg_reduce_ranks_kernel EPL=FULL glog=0 check=1',)),
    # four sequences per wave (rows of <= 32 bytes)
    Case('ranks_C_four_32B', 'C', 16400, 66, 130, 32, fwd=('seg_reduce_ranks_kernel EPL=FULL glog=3 split=0',),
         dtypes=(F32, BF16, F16, F64)),
    Case('ranks_C_four_small_batch', 'C', 20000, 1, 8, 16, fwd=('seg_reduce_ranks_kernel EPL=FULL glog=4',)),
    # ... with the long-sequence split: forced, and armed by itself (device-only lengths, long on average)
    Case('ranks_split_forced', 'Cdev', 100000, 1, 8, 16, outlier=5000, split=256,
         fwd=('seg_reduce_ranks_kernel check=1 split=1', 'seg_reduce_tail_kernel split=1',
              'seg_reduce_combine_kernel split=1')),
    Case('ranks_split_natural', 'seg', 16400, 256, 300, 16,
         fwd=('seg_reduce_ranks_kernel glog=4 split=1', 'seg_reduce_tail_kernel', 'seg_reduce_combine_kernel'),
         ops=('sum', 'max', 'logsumexp')),
    # few long units: a team of waves per sequence
    Case('team', 'C', 37, 512, 1024, 256, fwd=('seg_reduce_team_kernel EPL=FULL team=4',),
         bwd=('seg_backward_rows_kernel chunks=0 span=0',), bwd_prod=('seg_backward_kernel OP=prod split=0',),
         dtypes=(F32, BF16, F16, F64)),
    Case('team_L', 'L', 37, 512, 1024, 256, fwd=('seg_reduce_team_kernel team=4',),
         bwd=('seg_backward_rows_kernel chunks=0',)),
    Case('team_P', 'P', 37, 512, 1024, 256, fwd=('seg_reduce_team_kernel team=4',),
         bwd=('seg_backward_kernel split=1', 'seg_backward_tail_kernel split=1')),   # (the backward has no teams)
    # (at most 512 rows: longer sequences of 1000-byte rows arm the long-sequence split instead)
    Case('team_tail_overlap', 'C', 37, 256, 512, 1000, fwd=('seg_reduce_team_kernel EPL=FULL team=4',)),
    # one wave per (sequence, column chunk)
    Case('seq_cpw1_wpb2', 'C', 1500, 1, 100, 512,
         fwd=('seg_reduce_kernel EPL=FULL CPW=1 WPB=2 split=0',), bwd=('seg_backward_rows_kernel chunks=0 span=1',),
         bwd_prod=('seg_backward_kernel OP=prod',), dtypes=(F32, BF16, F16, F64)),
    Case('seq_cpw1_wpb2_R', 'R', 1500, 1, 100, 512, fwd=('seg_reduce_kernel CPW=1 WPB=2',),
         bwd=('seg_backward_rows_kernel',), bwd_prod=('seg_backward_kernel OP=prod pad_memset=1',)),
    Case('seq_cpw1_wpb1_C', 'C', 1000, 20, 100, 256, fwd=('seg_reduce_kernel EPL=FULL CPW=1 WPB=1',)),
    Case('seq_cpw1_P', 'P', 1000, 1, 100, 768, fwd=('seg_reduce_kernel EPL=FULL CPW=1 WPB=1',),
         bwd=('seg_backward_walk_kernel EPL=FULL chunks=0',), bwd_prod=('seg_backward_kernel OP=prod',)),
    Case('seq_tail_overlap', 'C', 1500, 1, 100, 1000, fwd=('seg_reduce_kernel EPL=FULL CPW=1 WPB=2',)),
    # rows wider than 1 KiB: four column chunks per wave
    Case('seq_cpw4', 'C', 300, 1, 100, 2048, fwd=('seg_reduce_kernel EPL=FULL CPW=4',),
         bwd=('seg_backward_rows_kernel chunks=1',), dtypes=(F32, BF16, F16, F64)),
    Case('seq_cpw4_P', 'P', 300, 1, 100, 2048, fwd=('seg_reduce_kernel EPL=FULL CPW=4',),
         bwd=('seg_backward_walk_kernel EPL=FULL chunks=1',), dtypes=(F32, BF16, F16, F64)),
    Case('seq_cpw4_half_P', 'P', 300, 1, 100, 2008, fwd=('seg_reduce_kernel EPL=HALF CPW=4',),
         bwd=('seg_backward_walk_kernel EPL=HALF',)),
    # scalar lanes: odd widths, and an aligned width whose payload pointer is not
    Case('scalar_H13', 'C', 3000, 20, 60, hidden=(13,), fwd=('seg_reduce_kernel EPL=1 CPW=1',),
         bwd=('seg_backward_walk_kernel EPL=1',), bwd_prod=('seg_backward_kernel EPL=1 OP=prod',)),
    Case('scalar_misaligned', 'C', 3000, 20, 60, 64, misaligned=True, fwd=('seg_reduce_kernel EPL=1',),
         bwd=('seg_backward_walk_kernel EPL=1',)),
    Case('multi_dim_hidden', 'C', 3000, 1, 100, hidden=(4, 8), fwd=('seg_reduce_kernel EPL=FULL',)),
    # one giant sequence among short ones: split + tail + combine (backward: over P, whose walk has no rows kernel)
    Case('seq_split', 'C', 2000, 1, 50, 256, outlier=60000,
         fwd=('seg_reduce_kernel split=1', 'seg_reduce_tail_kernel split=1', 'seg_reduce_combine_kernel split=1'),
         ops=('sum', 'mean', 'max', 'logsumexp')),
    Case('seq_split_P', 'P', 2000, 1, 50, 256, outlier=60000,
         fwd=('seg_reduce_kernel split=1', 'seg_reduce_tail_kernel', 'seg_reduce_combine_kernel'),
         bwd=('seg_backward_kernel split=1', 'seg_backward_tail_kernel split=1'), ops=('sum', 'max', 'logsumexp')),
    Case('seq_split_forced', 'Cdev', 300, 200, 3000, 64, split=128,
         fwd=('seg_reduce_kernel split=1', 'seg_reduce_tail_kernel', 'seg_reduce_combine_kernel')),
    # fused pack + reduce
    Case('fused_cpw1', 'fused', 3000, 1, 40, 256, fwd=('seg_reduce_kernel COPY=1 CPW=1',), dtypes=(F32, BF16, F16)),
    Case('fused_cpw4', 'fused', 2000, 1, 10, 2048, fwd=('seg_reduce_kernel COPY=1 CPW=4',)),
    # fill_empty: narrow rows, the ballot form over 16-byte pieces and over elements; NO_EMPTY proved by the host
    Case('fill_narrow', 'seg', 3000, 1, 100, 64, fwd=('fill_empty_kernel form=narrow',), ops=('max', 'min', 'logsumexp')),
    Case('fill_ballot', 'seg', 500, 1, 100, 1024, fwd=('fill_empty_kernel form=ballot',), ops=('max', 'min', 'logsumexp')),
    Case('fill_scalar', 'seg', 3000, 1, 100, hidden=(13,), fwd=('fill_empty_kernel form=ballot_scalar',),
         ops=('max', 'min', 'logsumexp')),
    Case('no_empty_host', 'C', 1000, 1, 100, 256, empties=False, fwd=('seg_reduce_kernel no_empty=1',),
         ops=('max', 'min', 'logsumexp')),
    Case('no_empty_device', 'Cdev', 1000, 1, 100, 256, empties=False, fwd=('seg_reduce_kernel no_empty=0',),
         ops=('max', 'min', 'logsumexp')),
]


# ------------------------------------------------------------------ the reference, restated (reduce.py:34-61)
def ref_reduce(name, x, lens):
    if name in ('max', 'min'):
        init = (x.min() if name == 'max' else x.max()).detach().item()
        return torch.segment_reduce(x, name, lengths=lens, unsafe=True, initial=init)
    if name == 'logsumexp':
        m = ref_reduce('max', x, lens).detach()
        t = (x - torch.repeat_interleave(m, dim=0, repeats=lens)).exp()
        eps = (lens == 0).to(dtype=t.dtype).view((-1, *[1 for _ in t.size()[1:]]))
        return (ref_reduce('sum', t, lens) + eps).log() + m
    initial = 1 if name == 'prod' else 0
    return torch.segment_reduce(x, name, lengths=lens, unsafe=True, initial=initial)


# ------------------------------------------------------------------ inputs
def make_lens(case, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(case.lo, case.hi + 1, (case.B,), generator=g)
    if case.outlier:
        lens = torch.cat([lens, torch.tensor([case.outlier])])[torch.randperm(case.B + 1, generator=g)]
    if case.empties and case.kind not in ('P', 'fused'):
        lens[torch.randperm(lens.numel(), generator=g)[:max(1, lens.numel() // 50)]] = 0
    return lens


def make_data(name, n, hidden, dtype, lens, seed):
    """Integer data for sum / mean / max / min (exact in any order); factors from {+-1, +-0.5, +-2} for prod, at most
    ~100 non-unit ones per sequence (~12 in f16); randn for logsumexp."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + tuple(hidden)
    if name == 'logsumexp':
        return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
    if name == 'prod':
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
        cap = 6 if dtype == F16 else 100
        per_row = cap / max(1, int(lens.max()) if lens.numel() else 1)
        nonunit = torch.rand(shape, generator=g) < min(0.5, per_row)
        mag = torch.where(torch.rand(shape, generator=g) < 0.5, 0.5, 2.0).double()
        return (sign * torch.where(nonunit, mag, torch.ones_like(mag))).to(dtype)
    hi = 2 if dtype == F16 else 8
    wide = torch.randint(-hi, hi + 1, shape, generator=g)
    narrow = torch.randint(0, 3, shape, generator=g)                  # ties
    pick = torch.rand(shape[:1] + (1,) * len(hidden), generator=g) < 0.5
    return torch.where(pick, narrow, wide).double().to(dtype)


def storage_rows(kind, lens, T=None, sorted_indices=None):
    """Row of the container's storage (first dims flattened) of every token, in CattedSequence order."""
    lens_np = lens.numpy()
    b = np.repeat(np.arange(lens_np.size), lens_np)
    off = np.concatenate([[0], np.cumsum(lens_np)[:-1]]) if lens_np.size else np.zeros(0, np.int64)
    t = np.arange(lens_np.sum()) - np.repeat(off, lens_np)
    if kind == 'L':
        return torch.from_numpy(b * T + t)
    if kind == 'R':
        return torch.from_numpy(b * T + (T - lens_np[b]) + t)
    if kind == 'P':
        srt = sorted_indices.cpu().numpy()
        rank = np.empty_like(srt)
        rank[srt] = np.arange(srt.size)
        bsz = np.array([(lens_np > s).sum() for s in range(int(lens_np.max()))])
        boff = np.concatenate([[0], np.cumsum(bsz)[:-1]])
        return torch.from_numpy(boff[t] + rank[b])
    return torch.from_numpy(np.arange(lens_np.sum()))


def build(case, x, lens, pad=0.0):
    """(container or payload, storage tensor, storage rows of the tokens) on the device; the storage is a leaf."""
    xd = x.to(DEV)
    if case.misaligned:
        flat = torch.empty(xd.numel() + 1, dtype=x.dtype, device=DEV)
        flat[1:] = xd.reshape(-1)
        xd = flat[1:].view(xd.shape)
    if case.kind in ('C', 'Cdev', 'seg', 'fused'):
        return xd, storage_rows('C', lens)
    c = ta.with_host_sizes(xd, lens)
    if case.kind == 'P':
        p = c.pack()
        return p, storage_rows('P', lens, sorted_indices=p.sorted_indices)
    z = c.left(pad) if case.kind == 'L' else c.right(pad)
    return z, storage_rows(case.kind, lens, int(z.data.size(1)))


def run(case, name, base, lens, leaf):
    """The reduction under test over the storage tensor `leaf`."""
    if case.kind == 'C':
        return getattr(ta, f'reduce_{name}')(ta.with_host_sizes(leaf, lens))
    if case.kind == 'Cdev':
        return getattr(ta, f'reduce_{name}')(ta.C(leaf, lens.to(DEV)))
    if case.kind == 'seg':
        return getattr(ta, f'segment_{name}')(leaf, lens.to(DEV))
    if case.kind == 'P':
        return getattr(ta, f'reduce_{name}')(ta.P(leaf, base.batch_sizes, base.sorted_indices, base.unsorted_indices))
    cls = ta.L if case.kind == 'L' else ta.R
    return getattr(ta, f'reduce_{name}')(cls(leaf, base.token_sizes))


def flat_rows(t, case):
    return t.reshape((-1,) + tuple(t.shape[2:])) if case.kind in ('L', 'R') else t


# ------------------------------------------------------------------ comparisons
def check_forward(name, got, exact, dtype, what):
    got = got.cpu()
    if name in ('sum', 'max', 'min', 'prod'):
        want = exact.to(dtype)
        same = (got == want) | (torch.isnan(got) & torch.isnan(want))
        assert bool(same.all()), f'{what}: {int((~same).sum())} elements not bit-equal to the exact result'
        return
    g64 = got.double()
    if name == 'mean':
        bound = (ACC_ULP[dtype] + HALF_ULP[dtype]) * exact.abs()
    else:
        bound = (1e-5 + 2 * HALF_ULP[dtype]) * exact.abs().clamp_min(1.0)
    ok = ((g64 - exact).abs() <= bound) | (torch.isnan(g64) & torch.isnan(exact)) | (g64 == exact)
    assert bool(ok.all()), f'{what}: {int((~ok).sum())} elements outside the bound'


def check_grad(name, got, exact, w_rows, dtype, what, out_rows=None):
    got = got.double().cpu()
    if name == 'sum':
        bound = torch.zeros_like(exact)
    elif name == 'logsumexp':
        # g * exp(x - out) with `out` as the forward returned it, rounded to the payload dtype: exp carries that
        # rounding (|out| * half an ulp) into the gradient
        bound = (1e-5 + HALF_ULP[dtype] * (2 + 2 * out_rows.abs())) * torch.maximum(exact.abs(), w_rows.abs())
    else:
        bound = (ACC_ULP[dtype] + HALF_ULP[dtype]) * exact.abs()
    ok = ((got - exact).abs() <= bound) | (torch.isnan(got) & torch.isnan(exact)) | (got == exact)
    assert bool(ok.all()), f'{what}: {int((~ok).sum())} gradient elements outside the bound'


def resolve(want, dtype):
    return want.replace('EPL=FULL', f'EPL={FULL[dtype]}').replace('EPL=HALF', f'EPL={HALF[dtype]}')


def assert_reached(t, wants, dtype, what):
    for w in wants:
        w = resolve(w, dtype)
        assert t.matching(w), f'{what}: no launch matched "{w}"; the dispatchers launched:\n  ' + '\n  '.join(t.records)


# ------------------------------------------------------------------ the table, row by row
def _ids(case_dtype):
    case, dtype = case_dtype
    return f'{case.id}-{str(dtype).replace("torch.", "")}'


ROWS = [(c, d) for c in PATHS for d in c.dtypes]


@pytest.mark.parametrize('case,dtype', ROWS, ids=[_ids(r) for r in ROWS])
def test_path(case, dtype, monkeypatch):
    if case.split:
        monkeypatch.setattr(M, 'reduce_split_rows', lambda lay, *a, **k: case.split)
    seed = sum(map(ord, case.id)) + FULL[dtype]
    lens = make_lens(case, seed)
    hidden = case.hid(dtype)
    n = int(lens.sum())
    fwd_seen, bwd_seen = [], []
    for k, name in enumerate(case.ops):
        x = make_data(name, n, hidden, dtype, lens, seed + k)
        what = f'{case.id} {name} {dtype}'
        x64 = x.double().requires_grad_(True)
        exact = ref_reduce(name, x64, lens)
        base, rows = build(case, x, lens)
        if case.kind == 'fused':
            with dispatch_trace() as t:
                p, got = ta.pack_reduce(ta.with_host_sizes(base, lens), name, fused=True)
            assert torch.equal(p.data, ta.with_host_sizes(base, lens).pack().data), f'{what}: packed payload'
            check_forward(name, got, exact.detach(), dtype, what)
            fwd_seen.append(t)
            continue
        store = base if isinstance(base, torch.Tensor) else base.data
        want_grad = bool(case.bwd or case.bwd_prod) and (name in ('sum', 'max', 'logsumexp', 'prod'))
        leaf = store.clone().requires_grad_(True) if want_grad and not case.misaligned else store
        if want_grad and case.misaligned:
            leaf = store.requires_grad_(True)
        with dispatch_trace() as t:
            got = run(case, name, base, lens, leaf)
        fwd_seen.append(t)
        assert got.dtype == dtype and tuple(got.shape) == (lens.numel(),) + tuple(hidden)
        check_forward(name, got, exact.detach(), dtype, what)
        if not want_grad:
            continue
        g = torch.Generator().manual_seed(seed + 100 + k)
        w = torch.randint(-2, 3, got.shape, generator=g).double()
        (gx,) = torch.autograd.grad(exact, x64, w)
        with dispatch_trace() as tb:
            (gs,) = torch.autograd.grad(got, leaf, w.to(dtype).to(DEV))
        if name == 'prod':
            assert_reached(tb, case.bwd_prod, dtype, what + ' backward')
        else:
            bwd_seen.append(tb)
        flat = flat_rows(gs, case)
        w_rows = torch.repeat_interleave(w, lens, dim=0)
        out_rows = torch.repeat_interleave(exact.detach(), lens, dim=0)
        check_grad(name, flat[rows.to(DEV)], gx, w_rows, dtype, what + ' gradient', out_rows)
        live = torch.zeros(flat.size(0), dtype=torch.bool)
        live[rows] = True
        assert bool((flat[(~live).to(DEV)] == 0).all()), f'{what}: padding rows got a gradient'
    for want in case.fwd:
        w = resolve(want, dtype)
        assert any(t.matching(w) for t in fwd_seen), \
            f'{case.id} {dtype}: no forward launch matched "{w}":\n  ' + '\n  '.join(r for t in fwd_seen for r in t.records)
    for want in case.bwd:
        w = resolve(want, dtype)
        assert any(t.matching(w) for t in bwd_seen), \
            f'{case.id} {dtype}: no backward launch matched "{w}":\n  ' + '\n  '.join(r for t in bwd_seen for r in t.records)


# ------------------------------------------------------------------ edge rows on every path that tracks `initial`
EDGE_ROWS = [(c, d) for c in PATHS if c.kind != 'fused' and set(c.ops) & {'max', 'min', 'logsumexp'}
             for d in (F32,)]


def edge_data(variant, name, n, hidden, lens, seed):
    x = make_data('sum', n, hidden, F64, lens, seed)
    g = torch.Generator().manual_seed(seed)
    if variant == 'inf':                      # +-inf elements, and a column that is all -inf
        flat = x.view(n, -1)
        hit = torch.rand(flat.shape, generator=g) < 0.01
        inf = torch.full(flat.shape, np.inf, dtype=torch.float64)
        flat[hit] = torch.where(torch.rand(flat.shape, generator=g) < 0.5, -inf, inf)[hit]
        if flat.size(1) > 1:
            flat[:, 0] = -np.inf
    elif variant == 'nan':                    # one NaN: poisons `initial`, hence every empty sequence
        x.view(-1)[int(torch.randint(0, x.numel(), (1,), generator=g))] = np.nan
    elif variant == 'allinf':                 # all +inf (max / logsumexp) or all -inf (min): the global initial itself
        x.fill_(-np.inf if name == 'min' else np.inf)
    return x


@pytest.mark.parametrize('variant', ['inf', 'nan', 'allinf'])
@pytest.mark.parametrize('case,dtype', EDGE_ROWS, ids=[_ids(r) for r in EDGE_ROWS])
def test_path_edges(case, dtype, variant, monkeypatch):
    """Empty sequences next to infinities and NaN, and data that are nothing but an infinity, on every forward path
    that tracks the reference's global `initial`; padding rows of L / R holding inf / NaN / 1e9 get an exactly zero
    gradient; where the reference's gradient is finite the gradient matches it."""
    if case.split:
        monkeypatch.setattr(M, 'reduce_split_rows', lambda lay, *a, **k: case.split)
    seed = sum(map(ord, case.id)) + 7
    lens = make_lens(case, seed)
    hidden = case.hid(dtype)
    n = int(lens.sum())
    pad = {'inf': np.inf, 'nan': np.nan, 'allinf': 1e9}[variant]
    for k, name in enumerate(o for o in case.ops if o in ('max', 'min', 'logsumexp')):
        x = edge_data(variant, name, n, hidden, lens, seed + k).to(dtype)
        what = f'{case.id} {name} {dtype} {variant}'
        x64 = x.double().requires_grad_(True)
        exact = ref_reduce(name, x64, lens)
        base, rows = build(case, x, lens, pad=pad)
        store = base if isinstance(base, torch.Tensor) else base.data
        leaf = store.requires_grad_(True) if case.misaligned else store.clone().requires_grad_(True)
        got = run(case, name, base, lens, leaf)
        check_forward(name, got, exact.detach(), dtype, what)
        w = torch.randint(-2, 3, got.shape, generator=torch.Generator().manual_seed(seed)).double()
        (gx,) = torch.autograd.grad(exact, x64, w)
        (gs,) = torch.autograd.grad(got, leaf, w.to(dtype).to(DEV))
        flat = flat_rows(gs, case)
        live = torch.zeros(flat.size(0), dtype=torch.bool)
        live[rows] = True
        assert bool((flat[(~live).to(DEV)] == 0).all()), f'{what}: padding rows got a nonzero gradient'
        tok = flat[rows.to(DEV)].double().cpu()
        fin = torch.isfinite(gx)
        w_rows = torch.repeat_interleave(w, lens, dim=0).expand_as(gx)
        out_rows = torch.repeat_interleave(exact.detach(), lens, dim=0).expand_as(gx)
        check_grad(name, tok[fin], gx[fin], w_rows[fin], dtype, what + ' gradient', out_rows[fin])


# ------------------------------------------------------------------ state that outlives a call
# The max / min / logsumexp scratch persists per (device, stream) and fill_empty_kernel's ticket hands it back zeroed: a
# stale slot would leak one call's global extreme into the next call's empty sequences.
def _alternating_calls(seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 12, (500,), generator=g)
    lens[::7] = 0
    n = int(lens.sum())
    calls = []
    for k, (name, dtype, sign) in enumerate([('max', F32, 1), ('min', F32, -1), ('logsumexp', BF16, 1),
                                             ('max', BF16, -1), ('min', F64, 1), ('logsumexp', F32, -1),
                                             ('max', F16, 1), ('min', BF16, -1)]):
        # shifted integers: the global extreme (the fill of every empty sequence) changes sign and size call by call
        x = (torch.randint(0, 5, (n, 24), generator=g) + 3 * (k + 1)).double() * sign
        calls.append((name, x.to(dtype), lens))
    return calls


def _check_call(name, x, lens, what):
    got = getattr(ta, f'segment_{name}')(x.to(DEV), lens.to(DEV))
    check_forward(name, got, ref_reduce(name, x.double(), lens), x.dtype, what)


def test_scratch_back_to_back_alternating_op_dtype_sign():
    for i, (name, x, lens) in enumerate(_alternating_calls(1) * 2):
        _check_call(name, x, lens, f'call {i}: {name} {x.dtype}')


def test_scratch_on_a_second_stream():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    calls = _alternating_calls(2)
    with torch.cuda.stream(side):
        for i, (name, x, lens) in enumerate(calls):
            _check_call(name, x, lens, f'side stream call {i}: {name}')
    for i, (name, x, lens) in enumerate(calls[::-1]):        # and back on the default stream, which kept its own
        _check_call(name, x, lens, f'default stream call {i}: {name}')


def test_scratch_after_a_refused_launch(monkeypatch):
    """A launch the library refuses (here: fill_empty reported as refused) makes the caller forget the scratch; the next
    calls start from a fresh one and still match the reference."""
    from torchrua_amd import _lib
    real = _lib.check
    fired = []

    def refuse_once(code, what):
        if what == 'rua_fill_empty' and not fired:
            fired.append(what)
            real(code, what)
            raise _lib.RuaError('rua_fill_empty: refused (test)')
        return real(code, what)

    calls = _alternating_calls(3)
    _check_call(*calls[0], 'before')
    monkeypatch.setattr(_lib, 'check', refuse_once)
    name, x, lens = calls[1]
    with pytest.raises(_lib.RuaError):
        getattr(ta, f'segment_{name}')(x.to(DEV), lens.to(DEV))
    monkeypatch.setattr(_lib, 'check', real)
    assert fired
    for i, (name, x, lens) in enumerate(calls[2:] + calls[:2]):
        _check_call(name, x, lens, f'after the refusal, call {i}: {name}')


@pytest.mark.parametrize('name', ['max', 'min', 'logsumexp'])
def test_graph_replay_with_empty_sequences(name):
    """A captured reduce over a batch WITH empty sequences tracks the global `initial` on every replay: payloads whose
    global minimum / maximum changes between replays (single-stream capture, as test_ops_replay_inside_a_hip_graph)."""
    g = torch.Generator().manual_seed(21)
    lens = torch.randint(0, 20, (300,), generator=g)
    lens[::5] = 0
    n = int(lens.sum())
    static = torch.zeros(n, 32, device=DEV)
    c = ta.with_host_sizes(static, lens)
    red = getattr(ta, f'reduce_{name}')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            red(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = red(c)
    for k, shift in enumerate((5.0, -40.0, 300.0, -2.0)):
        x = torch.randint(-4, 5, (n, 32), generator=g).double() + shift
        static.copy_(x.float().to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        check_forward(name, out, ref_reduce(name, x, lens), F32, f'replay {k} (shift {shift})')
