"""cummax / cummin / logcumsumexp: what can be checked without a GPU — the public surface, the C ABI, the refusals
before any launch, and the yardsticks themselves (tests/cumext_util.py): torch's tie / NaN rule that the kernels
reproduce, and fp32 torch.logcumsumexp against the float64 one on the GPU tests' own inputs."""
import importlib
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib
import cumext_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_segment_cumextreme', 'rua_cumextreme_ws_bytes', 'rua_segment_cumextreme_backward',
                'rua_segment_logcumsumexp', 'rua_logcumsumexp_ws_bytes', 'rua_segment_logcumsumexp_backward')
NAMES = ('SeqCum', 'cummax', 'cummin', 'logcumsumexp', 'segment_cummax', 'segment_cummin', 'segment_logcumsumexp')


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.cumext')
    for name in NAMES:
        assert getattr(mod, name) is getattr(ta, name), name
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.cummax is ta.cummax and cls.cummin is ta.cummin and cls.logcumsumexp is ta.logcumsumexp, cls
    assert ta.SeqCum._fields == ('values', 'indices')
    from torchrua_amd import _ops
    for fn in ('_CumExtreme', '_CumRunSum', '_CumGather', '_LogCumSumExp'):
        assert issubclass(getattr(_ops, fn), torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import cummax, cummin, logcumsumexp, segment_cummax, segment_logcumsumexp, SeqCum; '
            'from torchrua.cumext import segment_cummin as s2; '
            'assert cummax is ta.cummax and s2 is ta.segment_cummin and SeqCum is ta.SeqCum; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    # a null layout, a dtype (or operator) the scans do not take: -1 before any launch
    assert lib.rua_segment_cumextreme(None, 8, 8, 8, 1, _lib.F32, _lib.MAX, 0, None, None) == -1
    assert lib.rua_segment_cumextreme(lay, 8, 8, 16, 1, _lib.I32, _lib.MAX, 0, None, None) == -1
    assert lib.rua_segment_cumextreme(lay, 8, 8, 16, 1, _lib.F32, _lib.SUM, 0, None, None) == -1
    assert lib.rua_segment_cumextreme(lay, 8, None, None, 1, _lib.F32, _lib.MAX, 0, None, None) == -1
    assert lib.rua_segment_cumextreme_backward(None, 8, 8, 8, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_cumextreme_backward(lay, 8, 8, 16, 1, _lib.I64, 0, None, None) == -1
    assert lib.rua_segment_logcumsumexp(None, 8, 8, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_logcumsumexp(lay, 8, 8, 1, _lib.I64, 0, None, None) == -1
    assert lib.rua_segment_logcumsumexp_backward(None, 8, 8, 8, 8, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_logcumsumexp_backward(lay, 8, 8, 8, 8, 1, _lib.I64, 0, None, None) == -1
    # the cut plan: one state per block and padded column —
    # B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * state bytes; the state of cummax / cummin is a
    # (value, position) pair of 16 bytes, that of logcumsumexp two accumulators (2 * 4, or 2 * 8 for float64)
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_cumextreme_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * 16
    assert lib.rua_cumextreme_ws_bytes(long_lay, 64, _lib.I64) == 2 * blocks * 4 * 16 * 16
    assert lib.rua_cumextreme_ws_bytes(long_lay, 64, _lib.BF16) == 2 * blocks * 1 * 64 * 16
    assert lib.rua_logcumsumexp_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * 8
    assert lib.rua_logcumsumexp_ws_bytes(long_lay, 64, _lib.F64) == 2 * blocks * 4 * 16 * 16
    assert lib.rua_logcumsumexp_ws_bytes(long_lay, 64, _lib.I64) == 0          # not a dtype of logcumsumexp
    for fn in (lib.rua_cumextreme_ws_bytes, lib.rua_logcumsumexp_ws_bytes):
        assert fn(long_lay, 2, _lib.F64) == 0 and fn(long_lay, 4, _lib.F32) == 0      # rows of one vector are never cut
        assert fn(lay, 64, _lib.F32) == 0 and fn(None, 64, _lib.F32) == 0


def test_no_cpu_fallback_and_refusals_before_launch():
    x, sizes = torch.randn(7, 3), torch.tensor([3, 4])
    for fn in (ta.segment_cummax, ta.segment_cummin, ta.segment_logcumsumexp):
        for reverse in (False, True):
            with pytest.raises(ta.RuaError):
                fn(x, sizes, reverse=reverse)
    with pytest.raises(ta.RuaError):
        ta.segment_logcumsumexp(torch.arange(7), sizes)
    with pytest.raises(ta.RuaError):
        ta.segment_cummax(torch.arange(7, dtype=torch.int32), sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        for name in ('cummax', 'cummin', 'logcumsumexp'):
            with pytest.raises(ta.RuaError):
                getattr(z, name)()
            with pytest.raises(ta.RuaError):
                getattr(ta, name)(z, reverse=True)


def test_torch_tie_and_nan_rule():
    """What the kernels reproduce bit for bit: a torch that changed its rule fails here, not on the GPU."""
    nan = float('nan')
    v, i = torch.cummax(torch.tensor([3., 3., 1., 3.]), 0)
    assert i.tolist() == [0, 1, 1, 3] and v.tolist() == [3., 3., 3., 3.]
    v, i = torch.cummin(torch.tensor([3., 3., 4., 3.]), 0)
    assert i.tolist() == [0, 1, 1, 3]
    v, i = torch.cummax(torch.tensor([1., 1., 0., nan, 2., nan, 3.]), 0)
    assert i.tolist() == [0, 1, 1, 3, 3, 5, 5] and bool(torch.isnan(v[3:]).all()) and v[:3].tolist() == [1., 1., 1.]
    v, i = torch.cummin(torch.tensor([1., 1., 2., nan, 0., nan, 3.]), 0)
    assert i.tolist() == [0, 1, 1, 3, 3, 5, 5] and bool(torch.isnan(v[3:]).all())
    v, i = torch.cummax(torch.tensor([0.0, -0.0, 0.0, -0.0]), 0)
    assert i.tolist() == [0, 1, 2, 3] and torch.signbit(v).tolist() == [False, True, False, True]
    v, i = torch.cummax(torch.tensor([float('-inf'), float('-inf')]), 0)
    assert i.tolist() == [0, 1]
    lo = torch.iinfo(torch.int64).min
    v, i = torch.cummax(torch.tensor([lo, lo, 5]), 0)
    assert i.tolist() == [0, 1, 2] and v.tolist() == [lo, lo, 5]
    for dtype in (torch.bfloat16, torch.float16):
        v, i = torch.cummax(torch.tensor([3., 3., 1., 3.]).to(dtype), 0)
        assert i.tolist() == [0, 1, 1, 3] and v.dtype == dtype
    # the helper's mirror rule: among equals the EARLIER position wins with `reverse`
    v, i = U.seg_cumextreme(torch.tensor([3., 1., 3., 3.]), torch.tensor([4]), True, True)
    assert i.tolist() == [0, 2, 2, 3]


def test_torch_logcumsumexp_special_values():
    inf = float('inf')
    y = torch.logcumsumexp(torch.tensor([-inf, -inf, 1., -inf, 2.], dtype=torch.float64), 0)
    assert y[:2].tolist() == [-inf, -inf] and bool(torch.isfinite(y[2:]).all())
    y = torch.logcumsumexp(torch.tensor([1., inf, 2.], dtype=torch.float64), 0)
    assert y.tolist() == [1., inf, inf]
    y = torch.logcumsumexp(torch.tensor([1., float('nan'), 2.], dtype=torch.float64), 0)
    assert y[0].item() == 1. and bool(torch.isnan(y[1:]).all())


@pytest.mark.parametrize('lens,hidden,seed', [(U.RAGGED, (), 11), (U.RAGGED, (64,), 11), (U.CROSSING, (8,), 21),
                                              (U.CUT, (64,), 11)], ids=('ragged1d', 'ragged64', 'crossing8', 'cut64'))
def test_fp32_torch_logcumsumexp_is_within_half_the_bar_of_float64(lens, hidden, seed):
    """The yardstick has to stay inside the bar on its own: fp32 torch.logcumsumexp on the GPU tests' inputs is within
    HALF of 1e-5 * (1 + |y|) of the float64 one — and the derived bound of the kernels' order is below the bar too."""
    x = U.draw((int(lens.sum()),) + hidden, U.F32, seed)
    for reverse in (False, True):
        want = U.seg_lse64(x, lens, reverse)
        got = torch.cat([(torch.logcumsumexp(p.flip(0), 0).flip(0) if reverse else torch.logcumsumexp(p, 0))
                         for p in U.pieces(x, lens)]).double()
        ratio = ((got - want).abs() / (0.5 * U.BAR * (1 + want.abs()))).max().item()
        print(f'cumext report: fp32 torch.logcumsumexp vs float64, worst / half the bar = {ratio:.4f}')
        assert ratio <= 1.0
        bound, bar = U.lse_bound(want, lens, reverse, U.F32)
        assert bool((bound <= bar).all())
