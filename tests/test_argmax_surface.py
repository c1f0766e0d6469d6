"""Per-sequence argmax / argmin: what can be checked without a GPU — the public surface, the C ABI (declared, listed,
exported, its argument checks, the workspace formula), and the CPU semantics the GPU tests measure against."""
import importlib
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('segment_argmax', 'segment_argmin', 'argmax', 'argmin', 'seq_max', 'seq_min')
ENTRY_POINTS = ('rua_argreduce_ws_bytes', 'rua_segment_argreduce', 'rua_segment_take', 'rua_segment_put')


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.argmax')
    for name in NAMES:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    assert 'max' not in mod.__all__ and 'min' not in mod.__all__          # `import *` must not shadow the builtins
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.argmax is ta.argmax and cls.argmin is ta.argmin, cls
        assert cls.max is ta.seq_max and cls.min is ta.seq_min, cls
    from torchrua_amd import _ops
    for fn in ('launch_argreduce', 'launch_take', 'launch_put'):
        assert callable(getattr(_ops, fn)), fn
    for cls in ('_ArgReduce', '_Take', '_Put'):
        assert issubclass(getattr(_ops, cls), torch.autograd.Function), cls


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import argmax, argmin, seq_max, seq_min, segment_argmin; '
            'from torchrua.argmax import segment_argmax as s2; '
            'assert argmax is ta.argmax and seq_min is ta.seq_min and s2 is ta.segment_argmax '
            'and callable(torchrua.argmax); print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    from torchrua_amd import _ops
    x, sizes = torch.randn(7, 3), torch.tensor([3, 4])
    for fn in (ta.segment_argmax, ta.segment_argmin):
        with pytest.raises(ta.RuaError):
            fn(x, sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        for fn in (ta.argmax, ta.argmin, ta.seq_max, ta.seq_min):
            with pytest.raises(ta.RuaError):
                fn(z)
        for method in ('argmax', 'argmin', 'max', 'min'):
            with pytest.raises(ta.RuaError):
                getattr(z, method)()
    index = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ta.RuaError):
        _ops.launch_take(None, x, index, (3,))
    with pytest.raises(ta.RuaError):
        _ops.launch_put(None, torch.randn(2, 3), index, (3,), (7, 3))
    with pytest.raises(ta.RuaError):
        _ops.launch_argreduce(None, x, _lib.MAX, (3,))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def test_rejected_arguments_need_no_device():
    lib = _lib.load()
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    bad = _lib.RuaLayout(kind=_lib.PACK, n_rows=4, B=1, T=4)                # a PackedSequence without offsets
    einval = -1
    assert lib.rua_segment_argreduce(None, 8, 8, 8, 1, _lib.F32, _lib.MAX, None, None) == einval
    assert lib.rua_segment_argreduce(bad, 8, 8, 8, 1, _lib.F32, _lib.MAX, None, None) == einval
    assert lib.rua_segment_argreduce(lay, 8, 8, 8, 1, _lib.I32, _lib.MAX, None, None) == einval
    for op in (_lib.SUM, _lib.MEAN, _lib.PROD, _lib.LOGSUMEXP, 17):
        assert lib.rua_segment_argreduce(lay, 8, None, 8, 1, _lib.F32, op, None, None) == einval
    for fn in (lib.rua_segment_take, lib.rua_segment_put):
        assert fn(None, 8, 8, 16, 1, _lib.F32, None) == einval
        assert fn(bad, 8, 8, 16, 1, _lib.F32, None) == einval
        assert fn(lay, 8, 8, 16, 1, _lib.U8, None) == einval
        assert fn(lay, 8, 8, 16, -1, _lib.F32, None) == einval


def test_workspace_formula():
    """rua.h: B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * (8 + accumulator bytes) when the cut form
    applies — fewer than 1 024 (sequence x chunk) units with a length bound of at least 8 192 — else 0."""
    lib = _lib.load()
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_argreduce_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * (8 + 4)
    assert lib.rua_argreduce_ws_bytes(long_lay, 64, _lib.BF16) == 2 * blocks * 1 * 64 * (8 + 4)
    assert lib.rua_argreduce_ws_bytes(long_lay, 64, _lib.I64) == 2 * blocks * 4 * 16 * (8 + 8)
    short_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    assert lib.rua_argreduce_ws_bytes(short_lay, 64, _lib.F32) == 0       # short sequences are never cut
    assert lib.rua_argreduce_ws_bytes(long_lay, 2, _lib.I64) == 0         # nor are rows of one vector
    assert lib.rua_argreduce_ws_bytes(long_lay, 64, _lib.I32) == 0
    assert lib.rua_argreduce_ws_bytes(None, 64, _lib.F32) == 0


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int64),
                         ids=lambda d: str(d).replace('torch.', ''))
def test_the_yardstick_itself(dtype):
    """What tests/test_gpu_argmax.py compares with — torch.max(dim=0) / torch.min(dim=0) on the CPU — has the semantics
    include/rua.h states: ties to the smallest position; NaN on top for max AND min, the first NaN; +0.0 == -0.0."""
    x = torch.tensor([[1, 3], [3, 3], [3, -2], [0, -2]]).to(dtype)
    assert x.max(dim=0).indices.tolist() == [1, 0] and x.min(dim=0).indices.tolist() == [3, 2]
    if dtype == torch.int64:
        return
    nan, inf = float('nan'), float('inf')
    y = torch.tensor([[inf, 0.0, -0.0], [nan, -0.0, 0.0], [nan, 0.0, 0.0], [-inf, 0.0, -0.0]]).to(dtype)
    for r in (y.max(dim=0), y.min(dim=0)):
        assert r.indices.tolist() == [1, 0, 0] and bool(torch.isnan(r.values[0]))
