"""The dispatch-trace records of the fold operators (softmax, log_softmax, cumsum, argmax / argmin, linear_scan,
var_mean, standardize, softmax_pool, causal_conv), byte for byte: which kernel form a call takes, with which template
arguments, in which order, and what each record says (field order, spelling, AL= as each operator computes it).

tests/golden/seg_trace_records.json was recorded by running `battery()` below on the commit BEFORE the host launchers
moved onto csrc/rua_seg_launch.h (the parent of the commit that added this file), never from the tree under test:
`json.dump(battery(), f, indent=0, sort_keys=True)` on an MI355X, with librua_hip.so built from that commit.  A
launcher refactor must leave it as it is; an intended change of a record re-records it the same way, from a tree that
has nothing else in flight.

The battery: every entry, forward and backward, float32 and bfloat16 (int64 where the operator takes it), over
C / L / P / R with lengths (0, 5, 70), at H = 2 (rows of one vector: the lanes form), H = 40 in bfloat16 and H = 64 (the
rows form, AL=1: 80 bytes are five whole vectors, so that shape is as aligned as the 64-column one) and H = 36 in
bfloat16 (the rows form, 72-byte rows: AL=0, the elementwise arm of every launcher); and once per operator that has a
cut form the smallest shape that cuts — one sequence of 8 192 tokens, H = 8 float32 (one unit, below 1 024, at the
8 192 bound; AL=1) and H = 9 float32 (36-byte rows: the cut records with AL=0), as an L and as a C whose length bound
the host knows."""
import json
import os

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib as K
from torchrua_amd.layout import lay_hidden, rewrap

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seg_trace_records.json')
LENS = (0, 5, 70)
CUT_LEN, CUT_HS = 8192, (8, 9)
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
SHAPES = [(F32, 2), (BF16, 2), (BF16, 36), (BF16, 40), (F32, 64), (BF16, 64), (I64, 2), (I64, 64)]


def _payload(n, H, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == I64:
        return torch.randint(-50, 50, (n, H), generator=g).cuda()
    return torch.randn(n, H, generator=g).to(dtype).cuda()


def _build(kind, x, lens):
    c = ta.with_host_sizes(x, torch.tensor(lens, dtype=torch.long))
    z = {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()
    lay_hidden(z)                                  # whatever describing the layout launches happens before the trace
    return z


def _leaf(z):
    return z.data.detach().clone().requires_grad_(True)


def _back(out):
    out.float().sum().backward()


def _unary(name, **kw):
    def run(z, floating):
        if not floating:
            getattr(z, name)(**kw)
            return
        _back(getattr(rewrap(z, _leaf(z)), name)(**kw).data)
    return run


def _arg(z, floating):
    z.argmax()
    z.argmin()
    if not floating:
        z.max()
        return
    _back(rewrap(z, _leaf(z)).max().values)
    _back(rewrap(z, _leaf(z)).min().values)


def _linear_scan(z, floating):
    gate = torch.full_like(z.data, 0.5).requires_grad_(True)
    _back(rewrap(z, _leaf(z)).linear_scan(gate).data)
    _back(rewrap(z, _leaf(z)).linear_scan(gate.detach(), reverse=True).data)
    _back(rewrap(z, _leaf(z)).linear_scan(0.9).data)


def _var_mean(z, floating):
    var, mean = rewrap(z, _leaf(z)).var_mean()
    _back(var + mean)


def _pool(z, floating):
    lead = 1 if isinstance(z, (ta.C, ta.P)) else 2
    for shape in (z.data.shape[:lead], z.data.shape):          # one score column, and one per hidden column
        scores = torch.zeros(shape, dtype=z.data.dtype, device=z.data.device).requires_grad_(True)
        _back(rewrap(z, _leaf(z)).softmax_pool(scores))


def _conv(z, floating):
    H = z.data.shape[-1]
    for reverse in (False, True):
        w = torch.ones(3, H, dtype=z.data.dtype, device=z.data.device).requires_grad_(True)
        b = torch.zeros(H, dtype=z.data.dtype, device=z.data.device).requires_grad_(True)
        _back(rewrap(z, _leaf(z)).causal_conv(w, b, reverse=reverse).data)
    z.causal_conv(w.detach())                                   # no bias, no gradient


# operator -> (runner, takes int64, has a cut form, the entry point of its workspace)
OPS = {
    'softmax': (_unary('softmax'), False, True, 'rua_softmax_ws_bytes'),
    'log_softmax': (_unary('log_softmax'), False, True, 'rua_softmax_ws_bytes'),
    'cumsum': (_unary('cumsum'), True, True, 'rua_cumsum_ws_bytes'),
    'cumsum_reverse': (_unary('cumsum', reverse=True), True, True, 'rua_cumsum_ws_bytes'),
    'argreduce': (_arg, True, True, 'rua_argreduce_ws_bytes'),
    'linear_scan': (_linear_scan, False, True, 'rua_linear_scan_ws_bytes'),
    'var_mean': (_var_mean, False, True, 'rua_norm_ws_bytes'),
    'standardize': (_unary('standardize'), False, True, 'rua_norm_ws_bytes'),
    'softmax_pool': (_pool, False, False, None),
    'causal_conv': (_conv, False, True, None),                  # (cuts by the family's rule; its workspace is the backward's)
}


def battery():
    """{'<operator> <dtype> H=<H> <kind>': [records]} of the whole battery."""
    from gpu_util import dispatch_trace
    got = {}

    def one(key, run, z, floating):
        with dispatch_trace() as tr:
            run(z, floating)
        got[key] = tr.records

    for name, (run, takes_i64, cuts, _) in OPS.items():
        for dtype, H in SHAPES:
            if dtype == I64 and not takes_i64:
                continue
            x = _payload(sum(LENS), H, dtype, 7)
            for kind in 'CLPR':
                one(f'{name} {dtype} H={H} {kind}'.replace('torch.', ''), run, _build(kind, x, LENS), dtype != I64)
        for H in CUT_HS if cuts else ():
            x = _payload(CUT_LEN, H, F32, 8)
            for kind in 'LC':
                one(f'{name} cut H={H} {kind}', run, _build(kind, x, (CUT_LEN,)), True)
    return got


def test_the_cut_shape_has_a_workspace():
    """No GPU: the smallest shape that cuts does cut, by every operator's own `*_ws_bytes`."""
    lib = K.load()
    lays = (K.RuaLayout(kind=K.LEFT, n_rows=CUT_LEN, B=1, T_phys=CUT_LEN, T_log=CUT_LEN),
            K.RuaLayout(kind=K.CAT, n_rows=CUT_LEN, B=1, len_add=1, T_log=CUT_LEN))
    for symbol in sorted({ws for _, _, cuts, ws in OPS.values() if cuts and ws}):
        for lay in lays:
            for H in CUT_HS:
                assert getattr(lib, symbol)(lay, H, K.F32) > 0, (symbol, H)
            assert getattr(lib, symbol)(lay, 4, K.F32) == 0, symbol               # (a row of one vector never cuts)
    assert lib.rua_causal_conv_ws_bytes(lays[0], CUT_HS[0], 3, K.F32) > 0


@pytest.mark.gpu
def test_trace_records_are_the_recorded_ones():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = battery()
    for name, (_, _, cuts, _) in OPS.items():
        for kind in 'CLPR':
            recs = got[f'{name} bfloat16 H=36 {kind}']
            assert any(' AL=0 ' in r and '_lanes_' not in r for r in recs), (name, kind, recs)
        for H in CUT_HS if cuts else ():
            for kind in 'LC':
                recs = got[f'{name} cut H={H} {kind}']
                assert any(f'AL={int(H % 4 == 0)} ' in r and 'cut=1' in r for r in recs), (name, H, kind, recs)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
