"""Per-sequence sort / argsort / reorder / topk: what can be checked without a GPU — the public surface, the Python-side
refusals, the C ABI's argument checks (none of them touches a device), the workspace formula of include/rua.h and the
host plan with its merge arithmetic under the sanitizers."""
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_sort_block_len', 'rua_sort_ws_bytes', 'rua_segment_sort', 'rua_segment_reorder')
NAMES = ['SeqSort', 'argsort', 'reorder', 'segment_argsort', 'segment_sort', 'sort', 'topk']
EINVAL, EALIGN, ERANGE = -1, -2, -3


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.sort')
    assert sorted(mod.__all__) == NAMES
    for name in mod.__all__:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.sort is ta.sort and cls.argsort is ta.argsort and cls.reorder is ta.reorder and cls.topk is ta.topk, cls
    assert ta.SeqSort._fields == ('values', 'indices')
    from torchrua_amd import _ops
    for name in ('launch_sort', 'launch_reorder', 'sort', 'reorder'):
        assert callable(getattr(_ops, name)), name
    assert issubclass(_ops._Sort, torch.autograd.Function) and issubclass(_ops._Reorder, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.sort"); '
            'from torchrua import sort, argsort, reorder, topk, segment_sort, segment_argsort, SeqSort; '
            'from torchrua.sort import argsort as a2; '
            'assert sort is ta.sort and a2 is ta.argsort and reorder is ta.reorder and topk is ta.topk; '
            'assert m.sort is ta.sort and m.segment_sort is ta.segment_sort; '
            'assert torchrua.C.sort is ta.sort and torchrua.P.argsort is ta.argsort; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers(dtype=torch.float32, hidden=(2,)):
    sizes = torch.tensor([3, 2])
    p = torch.nn.utils.rnn.pack_sequence([torch.ones((3,) + hidden).to(dtype), torch.ones((2,) + hidden).to(dtype)])
    return (ta.C(torch.ones((5,) + hidden).to(dtype), sizes), ta.L(torch.ones((2, 4) + hidden).to(dtype), sizes),
            ta.R(torch.ones((2, 4) + hidden).to(dtype), sizes), p)


def _lead(z):
    return tuple(z.data.shape[:1]) if isinstance(z, (ta.C, ta.P)) else tuple(z.data.shape[:2])


def test_no_cpu_fallback():
    for z in _containers():
        rows = torch.zeros(_lead(z), dtype=torch.long)
        elems = torch.zeros(tuple(z.data.shape), dtype=torch.long)
        for call in (lambda: z.sort(), lambda: z.sort(descending=True), lambda: z.argsort(), lambda: ta.sort(z),
                     lambda: ta.argsort(z, descending=True), lambda: z.topk(2), lambda: ta.topk(z, 1, largest=False),
                     lambda: z.reorder(rows), lambda: z.reorder(elems, inverse=True), lambda: ta.reorder(z, rows),
                     lambda: z.reorder(z._replace(data=rows))):
            with pytest.raises(ta.RuaError, match='no CPU fallback'):
                call()
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_sort(torch.randn(5, 2), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_argsort(torch.arange(5), torch.tensor([3, 2]), descending=True)


def test_python_refuses_unfit_arguments_before_any_launch():
    """Each of these is raised before the device check (the tensors are host tensors: the message tells them apart)."""
    for dtype in (torch.int32, torch.int8, torch.bool, torch.uint8, torch.complex64):
        for z in _containers(dtype):
            for call in (z.sort, z.argsort, lambda: z.topk(1)):
                with pytest.raises(ta.RuaError, match='supports'):
                    call()
        with pytest.raises(ta.RuaError, match='supports'):
            ta.segment_sort(torch.ones(5, 2).to(dtype), torch.tensor([3, 2]))
        with pytest.raises(ta.RuaError, match='supports'):
            ta.segment_argsort(torch.ones(5, 2).to(dtype), torch.tensor([3, 2]))
    for z in _containers():
        lead = _lead(z)
        with pytest.raises(ta.RuaError, match='must be torch.int64'):
            z.reorder(torch.zeros(lead, dtype=torch.int32))
        with pytest.raises(ta.RuaError, match='must be torch.int64'):
            z.reorder(torch.zeros(lead))
        with pytest.raises(ta.RuaError, match='indices has shape'):
            z.reorder(torch.zeros((lead[0] + 1,) + lead[1:], dtype=torch.long))
        with pytest.raises(ta.RuaError, match='indices has shape'):
            z.reorder(torch.zeros(lead + (3,), dtype=torch.long))              # neither the token dims nor the hidden shape
        with pytest.raises(ta.RuaError, match='indices lives on meta'):
            z.reorder(torch.zeros(lead, dtype=torch.long, device='meta'))
        with pytest.raises(ta.RuaError, match='or a container of the same type'):
            z.reorder([0] * lead[0])
        for k in (-1, 1.5, True, None):
            with pytest.raises(ta.RuaError, match='non-negative int'):
                z.topk(k)
    c, l = _containers()[:2]
    with pytest.raises(ta.RuaError, match='must be a CattedSequence'):
        c.reorder(ta.L(torch.zeros(2, 4, dtype=torch.long), l.token_sizes))
    with pytest.raises(ta.RuaError, match='must be a LeftAlignedSequence'):
        l.reorder(ta.C(torch.zeros(5, dtype=torch.long), c.token_sizes))
    with pytest.raises(ta.RuaError, match='takes a container'):
        ta.sort(torch.ones(3))
    with pytest.raises(ta.RuaError, match='takes a container'):
        ta.reorder(torch.ones(3), torch.zeros(3, dtype=torch.long))
    with pytest.raises(ta.RuaError, match='1, 2, 4 or 8 bytes'):
        c._replace(data=torch.ones(5, 2, dtype=torch.complex128)).reorder(torch.zeros(5, dtype=torch.long))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    assert lib.rua_abi_version() == 6
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    assert lib.rua_sort_block_len() == 2048


def _lay(kind=_lib.CAT, **kw):
    if kind == _lib.CAT:
        kw = dict(dict(n_rows=8, B=2, len_add=4), **kw)
    elif kind == _lib.PACK:
        kw = dict(dict(n_rows=8, B=2, T=4, boff=0x1000), **kw)
    else:
        kw = dict(dict(n_rows=8, B=2, T_phys=4, T_log=4), **kw)
    return _lib.RuaLayout(kind=kind, **kw)


def test_argument_checks_need_no_device():
    """(data, values, indices, ws) = (0x100, 0x200, 0x300, 0x400) and (data, index, out) = (0x100, 0x200, 0x300):
    made-up addresses, never dereferenced by a check.  Every call returns before a launch."""
    lib = _lib.load()
    sort, reorder = lib.rua_segment_sort, lib.rua_segment_reorder
    lay = _lay()
    F32 = _lib.F32
    for values in (0x200, None):
        assert sort(None, 0x100, values, 0x300, 2, F32, 0, None, None) == EINVAL
        assert sort(_lay(n_rows=-1), 0x100, values, 0x300, 2, F32, 0, None, None) == EINVAL
        assert sort(_lay(B=-1), 0x100, values, 0x300, 2, F32, 0, None, None) == EINVAL
        assert sort(_lib.RuaLayout(kind=_lib.LIST, n_rows=8, B=2), 0x100, values, 0x300, 2, F32, 0, None, None) == EINVAL
        assert sort(_lay(_lib.PACK, boff=None), 0x100, values, 0x300, 2, F32, 0, None, None) == EINVAL
        assert sort(lay, 0x100, values, 0x300, -1, F32, 0, None, None) == EINVAL          # a negative H
        for dtype in (_lib.I32, _lib.I16, _lib.I8, _lib.U8, 17, -1):                      # a bad dtype
            assert sort(lay, 0x100, values, 0x300, 2, dtype, 0, None, None) == EINVAL, dtype
        for dtype in (_lib.F32, _lib.F64, _lib.BF16, _lib.F16, _lib.I64):
            assert sort(lay, None, values, 0x300, 2, dtype, 0, None, None) == EINVAL       # null pointers
            assert sort(lay, 0x100, values, None, 2, dtype, 0, None, None) == EINVAL
            assert sort(lay, 0x300, values, 0x300, 2, dtype, 0, None, None) == EINVAL      # the indices are the input
            assert sort(lay, 0x100, values, 0x300, 0, dtype, 0, None, None) == 0           # no columns
            assert sort(_lay(B=0, n_rows=0), None, None, None, 2, dtype, 0, None, None) == 0
        assert sort(lay, 0x100, values, 0x304, 2, F32, 0, None, None) == EALIGN
        assert sort(lay, 0x102, values, 0x300, 2, F32, 0, None, None) == EALIGN
    assert sort(lay, 0x100, 0x100, 0x300, 2, F32, 0, None, None) == EINVAL                 # the values are the input
    assert sort(lay, 0x100, 0x300, 0x300, 2, F32, 0, None, None) == EINVAL                 # the values are the indices
    # a sequence of 2^31 tokens or more is refused; a long one without its workspace too
    assert sort(_lay(n_rows=2 ** 31, B=1, len_add=2 ** 31), 0x100, 0x200, 0x300, 1, F32, 0, 0x400, None) == ERANGE
    assert sort(_lay(_lib.LEFT, n_rows=2 ** 32, B=2, T_phys=2 ** 31, T_log=2 ** 31), 0x100, 0x200, 0x300, 1, F32, 0, 0x400,
                None) == ERANGE
    assert sort(_lay(n_rows=5000, B=1, len_add=5000), 0x100, 0x200, 0x300, 1, F32, 0, None, None) == EINVAL
    assert sort(_lay(n_rows=5000, B=1, len_add=5000), 0x100, 0x200, 0x300, 1, F32, 0, 0x404, None) == EALIGN

    for per_row in (0, 1):
        for inverse in (0, 1):
            assert reorder(None, 0x100, 0x200, 0x300, 2, 4, per_row, inverse, None) == EINVAL
            assert reorder(_lay(n_rows=-1), 0x100, 0x200, 0x300, 2, 4, per_row, inverse, None) == EINVAL
            assert reorder(lay, 0x100, 0x200, 0x300, -2, 4, per_row, inverse, None) == EINVAL
            for eb in (0, 3, 16, -4):
                assert reorder(lay, 0x100, 0x200, 0x300, 2, eb, per_row, inverse, None) == EINVAL, eb
            for eb in (1, 2, 4, 8):
                assert reorder(lay, None, 0x200, 0x300, 2, eb, per_row, inverse, None) == EINVAL
                assert reorder(lay, 0x100, None, 0x300, 2, eb, per_row, inverse, None) == EINVAL
                assert reorder(lay, 0x100, 0x200, None, 2, eb, per_row, inverse, None) == EINVAL
                assert reorder(lay, 0x100, 0x200, 0x100, 2, eb, per_row, inverse, None) == EINVAL   # out is the input
                assert reorder(lay, 0x100, 0x100, 0x300, 2, eb, per_row, inverse, None) == EINVAL   # the index is the input
                assert reorder(lay, 0x100, 0x200, 0x300, 0, eb, per_row, inverse, None) == 0
                assert reorder(_lay(B=0, n_rows=0), None, None, None, 2, eb, per_row, inverse, None) == 0
            assert reorder(lay, 0x100, 0x204, 0x300, 2, 4, per_row, inverse, None) == EALIGN
            assert reorder(lay, 0x101, 0x200, 0x300, 2, 2, per_row, inverse, None) == EALIGN


def _bound(lay):
    if lay.kind == _lib.CAT:
        return lay.T_log if 0 < lay.T_log < lay.n_rows else lay.n_rows
    return lay.T if lay.kind == _lib.PACK else lay.T_phys


def _pad256(n):
    return -(-n // 256) * 256


def _documented(lay, H, es):
    """include/rua.h: 256 + 2 * pad256(n_rows * H * 8) + (8-byte values: 2 * pad256(n_rows * H * 4)) when the bound is
    above 2 048."""
    if lay.B <= 0 or H <= 0 or not 2048 < _bound(lay) < 2 ** 31:
        return 0
    return 256 + 2 * _pad256(lay.n_rows * H * 8) + (2 * _pad256(lay.n_rows * H * 4) if es == 8 else 0)


def test_workspace_formula():
    ws = _lib.load().rua_sort_ws_bytes
    needed = 0
    sizes = {_lib.F32: 4, _lib.BF16: 2, _lib.F16: 2, _lib.F64: 8, _lib.I64: 8}
    for kind in (_lib.CAT, _lib.LEFT, _lib.PACK, _lib.RIGHT):
        for B in (1, 2, 1024, 65536):
            for bound in (0, 1, 64, 65, 2047, 2048, 2049, 8192, 200001):
                if kind == _lib.CAT:
                    lays = [_lay(kind, n_rows=bound, B=B, len_add=0), _lay(kind, n_rows=10 * bound + 1, B=B, len_add=0, T_log=bound)]
                elif kind == _lib.PACK:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T=bound)]
                else:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T_phys=bound, T_log=bound)]
                for lay in lays:
                    for H in (1, 3, 33):
                        for dtype, es in sizes.items():
                            assert ws(lay, H, dtype) == _documented(lay, H, es), (kind, B, bound, H, dtype)
                            needed += ws(lay, H, dtype) > 0
    assert needed >= 100
    assert ws(_lay(n_rows=2049, B=1, len_add=2049), 1, _lib.F32) == 256 + 2 * 16640      # by hand: 2049 * 8 = 16392 -> 16640
    assert ws(_lay(n_rows=2049, B=1, len_add=2049), 1, _lib.I64) == 256 + 2 * 16640 + 2 * 8448
    assert ws(_lay(n_rows=2048, B=1, len_add=2048), 1, _lib.F32) == 0
    assert ws(None, 1, _lib.F32) == 0 and ws(_lay(n_rows=-1), 1, _lib.F32) == 0 and ws(_lay(B=0, n_rows=0), 1, _lib.F32) == 0
    assert ws(_lay(n_rows=5000, B=1, len_add=5000), 1, _lib.I32) == 0 and ws(_lay(n_rows=5000, B=1, len_add=5000), -1, _lib.F32) == 0


def test_host_plan_under_host_sanitizers(tmp_path):
    """rua_sort_plan.h is plain host C++: tests/c/sort_plan_host.cpp includes it (and rua_seg_plan.h) alone, runs the
    merge arithmetic — passes, pairing, destination, parity — on keys from {0, 1, 2} with block lengths 4, 8 and the real
    one against std::stable_sort, and walks the plan's grids and workspace over sizes no GPU test can allocate, under
    ASan + UBSan, as its own process."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'sort_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'sort_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]
