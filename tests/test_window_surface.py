"""Per-sequence sliding-window pooling without a GPU: the names and methods, the `torchrua` alias, "no CPU fallback",
every Python refusal (raised on host tensors, before the device check), the argument checks of the C ABI through ctypes
(none touches a device), the yardstick of tests/window_util.py against F.max_pool1d / F.avg_pool1d wherever torch accepts
the input, and the host-side length formula against the yardstick's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
from torchrua_amd import _lib, _ops
from window_util import F32, F64, I64, KS, MODES, host_formula, n_out, pool64

EINVAL, EALIGN, ERANGE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_c(dtype=F32, hidden=(3,)):
    lens = torch.tensor([4, 0, 5])
    return ta.C(torch.zeros((9,) + hidden).to(dtype), lens)


# ------------------------------------------------------------------ names
def test_names_and_methods():
    for name in ('window_pool', 'max_pool', 'avg_pool', 'segment_window_pool'):
        assert callable(getattr(ta, name)), name
        assert name in ta.window.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        for m in ('window_pool', 'max_pool', 'avg_pool'):
            assert callable(getattr(cls, m)), f'{cls.__name__}.{m}'
    assert _lib.WINDOW_MAX_K == 64 == ta.window.MAX_K
    assert _lib.WINDOW_TAKE not in (_lib.SUM, _lib.MEAN, _lib.MAX)
    assert _ops.WINDOW_MODES == {'sum': _lib.SUM, 'mean': _lib.MEAN, 'max': _lib.MAX}
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert '#define RUA_WINDOW_MAX_K 64' in header and f'#define RUA_WINDOW_TAKE {_lib.WINDOW_TAKE}' in header


def test_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.window"); '
            'from torchrua import window_pool, max_pool, avg_pool, segment_window_pool; '
            'assert window_pool is ta.window_pool and m.avg_pool is ta.avg_pool and max_pool is ta.max_pool; '
            'assert segment_window_pool is ta.segment_window_pool and torchrua.P.max_pool is ta.max_pool; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    c = host_c()
    for call in (lambda: c.window_pool(2), lambda: c.max_pool(2, 1), lambda: c.avg_pool(3, ceil_mode=True),
                 lambda: ta.window_pool(c, 2, mode='sum'), lambda: ta.segment_window_pool(c.data, c.token_sizes, 2),
                 lambda: ta.L(torch.zeros(3, 5, 2), c.token_sizes).window_pool(2),
                 lambda: ta.R(torch.zeros(3, 5, 2), c.token_sizes).max_pool(2),
                 lambda: torch.nn.utils.rnn.pack_sequence([torch.zeros(3, 2), torch.zeros(2, 2)]).avg_pool(2)):
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            call()


# ------------------------------------------------------------------ refusals, before the device check
@pytest.mark.parametrize('args, kwargs, says', [
    ((2,), dict(mode='min'), "'min'"),
    ((2,), dict(mode=None), 'None'),
    ((0,), {}, 'kernel_size is 0'),
    ((65,), {}, 'kernel_size is 65'),
    ((-3,), {}, 'kernel_size is -3'),
    ((2, 0), {}, 'stride is 0'),
    ((2, 2 ** 31), {}, f'stride is {2 ** 31}'),
    ((2.0,), {}, 'kernel_size is 2.0'),
    ((True,), {}, 'kernel_size is True'),
    ((2, 1.5), {}, 'stride is 1.5'),
    (('3',), {}, "kernel_size is '3'"),
])
def test_argument_refusals(args, kwargs, says):
    with pytest.raises(ta.RuaError) as e:
        host_c().window_pool(*args, **kwargs)
    assert says in str(e.value) and 'no CPU fallback' not in str(e.value)


def test_dtype_and_container_refusals():
    for dtype in (torch.int32, torch.bool, torch.uint8, torch.complex64):
        with pytest.raises(ta.RuaError, match=str(dtype).replace('.', r'\.')):
            host_c(dtype).window_pool(2)
    with pytest.raises(ta.RuaError, match='int64'):
        host_c(I64).window_pool(2, mode='mean')
    with pytest.raises(ta.RuaError, match='int64'):
        host_c(I64).avg_pool(2)
    for other in (torch.zeros(3, 2), [1, 2], None):
        with pytest.raises(ta.RuaError, match=type(other).__name__):
            ta.window_pool(other, 2)
    with pytest.raises(ta.RuaError, match='list'):
        ta.segment_window_pool([1, 2], torch.tensor([2]), 2)
    # int64 max / sum and every float dtype pass the argument checks and stop at the device check
    for dtype, mode in ((I64, 'max'), (I64, 'sum'), (F64, 'mean'), (torch.bfloat16, 'max'), (torch.float16, 'sum')):
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            host_c(dtype).window_pool(64, 2 ** 31 - 1, mode)


# ------------------------------------------------------------------ the C ABI's argument checks (no device is touched)
def fake_layouts(B_small=3):
    keep = [torch.tensor([4, 0, 5]), torch.tensor([0, 4, 4]), torch.tensor([2, 0, 2]), torch.tensor([0, 2, 2])]
    big = _lib.RuaLayout(kind=_lib.CAT, n_rows=9, B=3, lens=keep[0].data_ptr(), off=keep[1].data_ptr())
    small = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=B_small, lens=keep[2].data_ptr(), off=keep[3].data_ptr())
    return big, small, keep


def test_abi_argument_checks():
    lib = _lib.load()
    big, small, keep = fake_layouts()
    a, b, c = (torch.zeros(64, dtype=torch.float64) for _ in range(3))        # host memory: never dereferenced
    pa, pb, pc = a.data_ptr(), b.data_ptr(), c.data_ptr()
    R = ctypes.byref
    pool, spread, lens = lib.rua_segment_window_pool, lib.rua_segment_window_spread, lib.rua_window_lens
    ok = dict(H=3, K=2, S=2, mode=_lib.MAX, dtype=_lib.F32)

    def call(fn, first, second, p0, p1, p2, **kw):
        v = {**ok, **kw}
        return fn(first, second, p0, p1, p2, v['H'], v['K'], v['S'], v['mode'], v['dtype'], None)

    # rua_segment_window_pool(src_lay, dst_lay, data, out, arg, ...)
    assert call(pool, None, R(small), pa, pb, pc) == EINVAL
    assert call(pool, R(big), None, pa, pb, pc) == EINVAL
    assert call(pool, R(big), R(fake_layouts(2)[1]), pa, pb, pc) == EINVAL           # another B
    assert call(pool, R(big), R(small), pa, pb, pc, H=-1) == EINVAL
    for mode in (_lib.MIN, _lib.PROD, _lib.LOGSUMEXP, 7, -1):
        assert call(pool, R(big), R(small), pa, pb, pc, mode=mode) == EINVAL
    for dtype in (_lib.I32, _lib.U8, 9, -1):
        assert call(pool, R(big), R(small), pa, pb, pc, dtype=dtype) == EINVAL
    assert call(pool, R(big), R(small), pa, pb, pc, dtype=_lib.I64, mode=_lib.MEAN) == EINVAL
    assert call(pool, R(big), R(small), pa, pb, pc, K=0) == EINVAL
    assert call(pool, R(big), R(small), pa, pb, pc, S=0) == EINVAL
    assert call(pool, R(big), R(small), pa, pb, pc, K=65) == ERANGE
    assert call(pool, R(big), R(small), None, pb, pc) == EINVAL
    assert call(pool, R(big), R(small), pa, None, pc) == EINVAL
    assert call(pool, R(big), R(small), pa, pb, None, mode=_lib.WINDOW_TAKE) == EINVAL
    assert call(pool, R(big), R(small), pa, pa, pc) == EINVAL                        # out aliases data
    assert call(pool, R(big), R(small), pa, pb, pb) == EINVAL                        # arg aliases out
    assert call(pool, R(big), R(small), pa + 2, pb, pc) == EALIGN
    assert call(pool, R(big), R(small), pa, pb, pc, H=0) == 0                        # nothing to do: no launch
    empty = _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0)
    assert call(pool, R(empty), R(empty), None, None, None) == 0

    # rua_segment_window_spread(pooled_lay, big_lay, grad_out, arg, grad_in, ...)
    assert call(spread, None, R(big), pa, pc, pb) == EINVAL
    assert call(spread, R(small), None, pa, pc, pb) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pb, mode=_lib.MIN) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pb, dtype=_lib.I64, mode=_lib.MEAN) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pb, K=0) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pb, S=-1) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pb, K=65) == ERANGE
    assert call(spread, R(small), R(big), None, pc, pb) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, None) == EINVAL
    assert call(spread, R(small), R(big), pa, None, pb) == EINVAL                    # max reads arg
    assert call(spread, R(small), R(big), pa, None, pb, mode=_lib.WINDOW_TAKE) == EINVAL
    assert call(spread, R(small), R(big), pa, pc, pa) == EINVAL                      # grad_in aliases grad_out
    assert call(spread, R(small), R(big), pa, pc, pb, H=0) == 0
    assert call(spread, R(empty), R(empty), None, None, None) == 0

    # rua_window_lens(lay, K, S, ceil_mode, out_lens, own_lens)
    assert lens(None, 2, 2, 0, pa, pb, None) == EINVAL
    assert lens(R(big), 0, 2, 0, pa, pb, None) == EINVAL
    assert lens(R(big), 2, 0, 1, pa, pb, None) == EINVAL
    assert lens(R(big), 65, 2, 0, pa, pb, None) == ERANGE
    assert lens(R(big), 2, 2, 0, None, pb, None) == EINVAL
    assert lens(R(big), 2, 2, 0, pa, pa, None) == EINVAL
    assert lens(R(big), 2, 2, 0, pa + 4, None, None) == EALIGN
    assert lens(R(empty), 2, 2, 0, None, None, None) == 0
    assert keep


# ------------------------------------------------------------------ the yardstick against torch, the formula against it
def test_yardstick_matches_torch_pooling():
    checked = refused = 0
    g = torch.Generator().manual_seed(0)
    for K in range(1, 9):
        for S in range(1, 11):
            for n in range(1, 30):
                x = torch.randn(n, 2, generator=g, dtype=F64)
                for ceil_mode in (False, True):
                    try:
                        mx = F.max_pool1d(x.T[None], K, S, ceil_mode=ceil_mode)[0].T
                        av = F.avg_pool1d(x.T[None], K, S, ceil_mode=ceil_mode, count_include_pad=False)[0].T
                    except RuntimeError:
                        refused += 1
                        assert n < K                       # torch refuses only what is shorter than the window
                        continue
                    checked += 1
                    assert mx.shape[0] == av.shape[0] == n_out(n, K, S, ceil_mode), (K, S, n, ceil_mode)
                    assert torch.equal(pool64(x, [n], K, S, 'max', ceil_mode).want, mx), (K, S, n, ceil_mode)
                    # two float64 means of at most 8 terms, each within (cnt + 1) 2^-53 max |x| of the exact one
                    tol = 2 * (K + 1) * 2.0 ** -53 * float(x.abs().max())
                    assert float((pool64(x, [n], K, S, 'mean', ceil_mode).want - av).abs().max()) <= tol, (K, S, n)
    assert checked > 3000 and refused > 0
    # n < K: here defined — nothing in floor mode, one clipped window in ceil mode
    x = torch.arange(6, dtype=F64).reshape(3, 2)
    assert pool64(x, [3], 5, 5, 'sum', False).want.shape[0] == 0
    p = pool64(x, [3], 5, 5, 'mean', True)
    assert p.lens.tolist() == [1] and torch.equal(p.want, x.mean(0, keepdim=True))
    p = pool64(x, [1, 0, 2], 5, 2, 'max', True)
    assert p.lens.tolist() == [1, 0, 1] and torch.equal(p.want, torch.stack([x[0], x[2]]))


@pytest.mark.parametrize('ceil_mode', [False, True])
def test_host_formula_matches_yardstick(ceil_mode):
    n = np.arange(0, 201)
    for K, S in KS:
        want = [n_out(int(v), K, S, ceil_mode) for v in n]
        assert host_formula(n, K, S, ceil_mode).tolist() == want, (K, S)
    assert host_formula(np.array([-3, 0]), 2, 1, ceil_mode).tolist() == [0, 0]      # a corrupt length: clamped
    assert set(MODES) == set(_ops.WINDOW_MODES)
