"""Per-sequence softmax-weighted sum (softmax_pool): what can be checked without a GPU — the public surface, the C ABI
and its device-free argument checks, and the fixture file itself (tests/golden/r10_softmax_pool.npz, written by
scripts/gen_golden_pool.py from the reference).

The GPU tests hold the kernels to the bounds of tests/pool_util.py against a float64 evaluation; the stored reference
results are re-checked HERE against that evaluation at half those bounds."""
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from pool_util import DTYPES, GOLDEN, exact, load_cases, ratio
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ('segment_softmax_pool', 'softmax_pool')
ENTRY_POINTS = ('rua_segment_softmax_pool', 'rua_segment_softmax_pool_backward', 'rua_softmax_pool_ws_bytes')


def test_public_names_exist():
    import importlib
    mod = importlib.import_module('torchrua_amd.pool')
    for name in FUNCTIONS:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.softmax_pool is ta.softmax_pool, cls


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import softmax_pool, segment_softmax_pool; '
            'from torchrua.pool import segment_softmax_pool as s2; '
            'assert softmax_pool is ta.softmax_pool and s2 is ta.segment_softmax_pool; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    v, s, sizes = torch.randn(7, 3), torch.randn(7), torch.tensor([3, 4])
    with pytest.raises(ta.RuaError):
        ta.segment_softmax_pool(v, s, sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    ps = torch.nn.utils.rnn.pack_sequence([torch.randn(3), torch.randn(2)])
    pairs = ((ta.C(v, sizes), s), (ta.L(torch.randn(2, 4, 3), sizes), torch.randn(2, 4)),
             (ta.R(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4), sizes)), (p, ps))
    for z, sc in pairs:
        with pytest.raises(ta.RuaError):
            z.softmax_pool(sc)
        with pytest.raises(ta.RuaError):
            ta.softmax_pool(z, sc)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    for word in ('seg_pool_lanes_kernel', 'seg_pool_rows_kernel', 'seg_pool_backward_kernel'):
        assert word in header, f'the header comment does not name the trace record {word}'


def test_argument_checks_need_no_device():
    lib = _lib.load()
    EINVAL = -1
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    fwd, bwd = lib.rua_segment_softmax_pool, lib.rua_segment_softmax_pool_backward
    # (pointers are never dereferenced before the checks: small integers stand in for distinct buffers)
    V, S, O, LSE, GO, GV, GS = 64, 128, 192, 256, 320, 384, 448
    assert fwd(None, V, S, O, LSE, 8, 8, _lib.F32, None, None) == EINVAL              # a null layout
    assert bwd(None, GO, V, S, O, LSE, GV, GS, 8, 8, _lib.F32, None, None) == EINVAL
    for code in (_lib.I64, _lib.I32, _lib.U8):                                         # an integer dtype
        assert fwd(lay, V, S, O, LSE, 8, 8, code, None, None) == EINVAL
        assert bwd(lay, GO, V, S, O, LSE, GV, GS, 8, 8, code, None, None) == EINVAL
    assert fwd(lay, V, S, O, LSE, 8, 3, _lib.F32, None, None) == EINVAL               # H % D != 0
    assert fwd(lay, V, S, O, LSE, 8, 0, _lib.F32, None, None) == EINVAL
    assert bwd(lay, GO, V, S, O, LSE, GV, GS, 8, 3, _lib.F32, None, None) == EINVAL
    assert fwd(lay, V, S, V, LSE, 8, 8, _lib.F32, None, None) == EINVAL               # an output aliasing an input
    assert fwd(lay, V, S, S, LSE, 8, 8, _lib.F32, None, None) == EINVAL
    assert fwd(lay, V, S, O, V, 8, 8, _lib.F32, None, None) == EINVAL
    assert fwd(lay, V, S, O, O, 8, 8, _lib.F32, None, None) == EINVAL
    for alias in (GO, V, S, O, LSE):
        assert bwd(lay, GO, V, S, O, LSE, alias, GS, 8, 8, _lib.F32, None, None) == EINVAL
        assert bwd(lay, GO, V, S, O, LSE, GV, alias, 8, 8, _lib.F32, None, None) == EINVAL
    assert bwd(lay, GO, V, S, O, LSE, GV, GV, 8, 8, _lib.F32, None, None) == EINVAL
    # nothing to do: 0 without a launch
    for empty in (_lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0), _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=3)):
        assert fwd(empty, V, S, O, LSE, 8, 8, _lib.F32, None, None) == 0
        assert bwd(empty, GO, V, S, O, LSE, GV, GS, 8, 8, _lib.F32, None, None) == 0
    assert fwd(lay, V, S, O, LSE, 0, 1, _lib.F32, None, None) == 0                    # H == 0
    assert bwd(lay, GO, V, S, O, LSE, GV, GS, 0, 1, _lib.F32, None, None) == 0
    assert bwd(lay, GO, V, S, O, LSE, None, None, 8, 8, _lib.F32, None, None) == 0    # no gradient asked for
    assert lib.rua_softmax_pool_ws_bytes(lay, 8, 8, _lib.F32) == 0


SHAPES = {((), ()), ((3,), ()), ((8,), ()), ((64,), ()), ((4, 16), (4,)), ((3, 5), (3,)), ((64,), (64,)), ((250,), ()),
          ((512,), ())}


def test_fixture_file_loads():
    assert os.path.getsize(GOLDEN) < 1_000_000
    cases = load_cases()
    assert len(cases) >= 30
    assert SHAPES <= {(c['hidden'], c['shidden']) for c in cases.values()}
    assert {c['dtype'] for c in cases.values()} == set(DTYPES)
    lens = [c['lens'] for c in cases.values()]
    assert any(int(x[0]) == 0 for x in lens) and any(int(x[-1]) == 0 for x in lens)
    assert any(bool(((x[1:] == 0) & (x[:-1] == 0)).any()) for x in lens)
    assert any(bool((x == 1).all()) for x in lens)
    assert any(int(x.max()) > 512 for x in lens)
    for name, c in cases.items():
        assert c['scale'] <= 3.0
        B = c['lens'].numel()
        assert c['out'].shape == (B,) + c['hidden'] and c['gv'].shape == c['v'].shape and c['gs'].shape == c['s'].shape
        for k in ('out', 'gv', 'gs'):
            assert bool(torch.isfinite(c[k]).all()), (name, k)


def test_reference_results_are_within_half_the_bar_of_float64():
    worst = {'out': 0.0, 'gv': 0.0, 'gs': 0.0}
    for name, c in load_cases().items():
        e = exact(c['v'], c['s'], c['cot'], c['lens'])
        for k, b in (('out', 'b_out'), ('gv', 'b_gv'), ('gs', 'b_gs')):
            r = ratio(c[k], e[k], e[b])
            assert r <= 0.5, f'{name}: the reference\'s {k} is at {r:.3f} of the bar'
            worst[k] = max(worst[k], r)
    print(f'reference vs float64, share of the bar: {worst}')
