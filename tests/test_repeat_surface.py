"""Per-sequence repeat_interleave: what can be checked without a GPU — the public surface, the Python-side refusals, the
C ABI's argument checks (none of them touches a device), the workspace formula of include/rua.h, the host plan under
the sanitizers, and the yardstick of tests/repeat_util.py against a plain loop."""
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import torchrua_amd as ta
from repeat_util import padded, repeat, repeat_by_loop, repeat_cat, same_bits, split
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_repeat_ws_bytes', 'rua_segment_repeat_plan', 'rua_segment_repeat_move', 'rua_segment_repeat_sum')
EINVAL = -1


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.repeat')
    assert sorted(mod.__all__) == ['repeat_interleave', 'segment_repeat_interleave']
    for name in mod.__all__:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.repeat_interleave is ta.repeat_interleave, cls
    from torchrua_amd import _ops
    for name in ('launch_repeat_plan', 'launch_repeat_move', 'launch_repeat_sum', 'repeat', 'run_sum'):
        assert callable(getattr(_ops, name)), name
    assert issubclass(_ops._Repeat, torch.autograd.Function) and issubclass(_ops._RunSum, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.repeat"); '
            'from torchrua import repeat_interleave, segment_repeat_interleave; '
            'from torchrua.repeat import segment_repeat_interleave as s2; '
            'assert repeat_interleave is ta.repeat_interleave and s2 is ta.segment_repeat_interleave; '
            'assert m.repeat_interleave is ta.repeat_interleave and torchrua.repeat is m; '
            'assert torchrua.C.repeat_interleave is ta.repeat_interleave and torchrua.P.repeat_interleave is ta.repeat_interleave; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers():
    sizes = torch.tensor([3, 2])
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    return (ta.C(torch.randn(5, 2), sizes), ta.L(torch.randn(2, 4, 2), sizes), ta.R(torch.randn(2, 4, 2), sizes), p)


def _lead(z):
    return tuple(z.data.shape[:1]) if isinstance(z, (ta.C, ta.P)) else tuple(z.data.shape[:2])


def test_no_cpu_fallback():
    for z in _containers():
        counts = torch.ones(_lead(z), dtype=torch.long)
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            z.repeat_interleave(counts)
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            z.repeat_interleave(2)
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            ta.repeat_interleave(z, z._replace(data=counts))      # the counts as a container of the same type
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_repeat_interleave(torch.randn(5, 2), torch.ones(5, dtype=torch.long), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_repeat_interleave(torch.arange(5), 3, torch.tensor([3, 2]))                    # 1-D int64, int count


def test_python_refuses_unfit_repeats_before_any_launch():
    """Each of these is raised before the device check (the tensors are host tensors: the message tells them apart)."""
    for z in _containers():
        lead = _lead(z)
        with pytest.raises(ta.RuaError, match='must be torch.int64'):
            z.repeat_interleave(torch.ones(lead, dtype=torch.int32))
        with pytest.raises(ta.RuaError, match='must be torch.int64'):
            z.repeat_interleave(torch.ones(lead))
        with pytest.raises(ta.RuaError, match=r'torch.bool.*compress\(mask\)'):
            z.repeat_interleave(torch.ones(lead, dtype=torch.bool))
        with pytest.raises(ta.RuaError, match='hidden dimensions'):
            z.repeat_interleave(torch.ones(lead + (2,), dtype=torch.long))
        with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
            z.repeat_interleave(torch.ones((lead[0] + 1,) + lead[1:], dtype=torch.long))
        with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
            z.repeat_interleave(torch.ones(lead, dtype=torch.long).reshape(-1)[:-1])
        with pytest.raises(ta.RuaError, match='repeats lives on meta'):
            z.repeat_interleave(torch.ones(lead, dtype=torch.long, device='meta'))
        with pytest.raises(ta.RuaError, match='negative int'):
            z.repeat_interleave(-1)
        with pytest.raises(ta.RuaError, match='or an int; got'):
            z.repeat_interleave([1] * lead[0])
        with pytest.raises(ta.RuaError, match='or an int; got'):
            z.repeat_interleave(1.5)
        with pytest.raises(ta.RuaError, match='or an int; got'):
            z.repeat_interleave(True)
    c, l = _containers()[:2]
    with pytest.raises(ta.RuaError, match='must be a CattedSequence'):
        c.repeat_interleave(ta.L(torch.ones(2, 4, dtype=torch.long), l.token_sizes))
    with pytest.raises(ta.RuaError, match='must be torch.int64'):
        ta.segment_repeat_interleave(torch.randn(5, 2), torch.ones(5), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='hidden dimensions'):
        ta.segment_repeat_interleave(torch.randn(5, 2), torch.ones(5, 2, dtype=torch.long), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
        ta.segment_repeat_interleave(torch.randn(5, 2), torch.ones(4, dtype=torch.long), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='negative int'):
        ta.segment_repeat_interleave(torch.randn(5, 2), -2, torch.tensor([3, 2]))


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


def _lay(kind=_lib.CAT, **kw):
    if kind == _lib.CAT:
        kw = dict(dict(n_rows=8, B=2, len_add=4), **kw)
    elif kind == _lib.PACK:
        kw = dict(dict(n_rows=8, B=2, T=4, boff=0x1000), **kw)
    else:
        kw = dict(dict(n_rows=8, B=2, T_phys=4, T_log=4), **kw)
    return _lib.RuaLayout(kind=kind, **kw)


def test_argument_checks_need_no_device():
    """(counts, first, new_lens, ws) = (8, 16, 32, 64), (first, dst, src) = (16, 32, 64) and (first, counts, grad_src,
    grad_dst) = (16, 8, 32, 64): made-up addresses, never dereferenced by a check.  Every call returns before a launch."""
    lib = _lib.load()
    plan, move, rsum = lib.rua_segment_repeat_plan, lib.rua_segment_repeat_move, lib.rua_segment_repeat_sum
    lay = _lay()
    # a null layout, a negative size, a bad kind, an inconsistent layout
    assert plan(None, 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(n_rows=-1), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(B=-1), 8, 16, 32, None, None) == EINVAL
    assert plan(_lib.RuaLayout(kind=7, n_rows=8, B=2), 8, 16, 32, None, None) == EINVAL
    assert plan(_lib.RuaLayout(kind=_lib.LIST, n_rows=8, B=2), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(_lib.PACK, boff=None), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(_lib.LEFT, T_phys=-1), 8, 16, 32, None, None) == EINVAL
    # null pointers and aliasing
    assert plan(lay, None, 16, 32, None, None) == EINVAL
    assert plan(lay, 8, None, 32, None, None) == EINVAL
    assert plan(lay, 8, 16, None, None, None) == EINVAL
    assert plan(lay, 16, 16, 32, None, None) == EINVAL               # first is the counts
    assert plan(lay, 8, 32, 32, None, None) == EINVAL                # new_lens is first
    assert plan(lay, 32, 16, 32, None, None) == EINVAL               # new_lens is the counts
    assert plan(lay, 8, 16, 36, None, None) == -2                    # RUA_EALIGN: int64 vectors
    # nothing to do: no sequence
    assert plan(_lay(B=0, n_rows=0), None, None, None, None, None) == 0

    # the move: src's checks, then dst's, then B, then nothing-to-do, then the pointers
    dst = _lay(n_rows=12, len_add=6)
    for first in (16, None):
        assert move(None, lay, first, 2, 32, 64, 4, None) == EINVAL
        assert move(dst, None, first, 2, 32, 64, 4, None) == EINVAL
        assert move(dst, _lay(n_rows=-1), first, 2, 32, 64, 4, None) == EINVAL
        assert move(_lay(n_rows=-1), lay, first, 2, 32, 64, 4, None) == EINVAL
        assert move(_lib.RuaLayout(kind=9, n_rows=4, B=2), lay, first, 2, 32, 64, 4, None) == EINVAL
        assert move(dst, lay, first, 2, 32, 64, -4, None) == EINVAL              # a negative row width
        assert move(_lay(n_rows=12, B=3, len_add=4), lay, first, 2, 32, 64, 4, None) == EINVAL       # another B
        assert move(dst, lay, first, 2, None, 64, 4, None) == EINVAL
        assert move(dst, lay, first, 2, 32, None, 4, None) == EINVAL
        assert move(dst, lay, first, 2, 64, 64, 4, None) == EINVAL               # dst_data == src_data
        assert move(dst, lay, first, 2, 32, 64, 0, None) == 0                    # rows of no bytes
        assert move(_lay(B=0, n_rows=0), _lay(B=0, n_rows=0), None, 2, None, None, 4, None) == 0
        assert move(_lay(n_rows=0, len_add=0), lay, first, 0, None, None, 4, None) == 0     # every count was 0
    assert move(dst, lay, None, -1, 32, 64, 4, None) == EINVAL                   # no table and a negative count

    # the sum: the dtype first of all, then as the move
    for dtype in (_lib.I64, _lib.I32, 17, -1):
        assert rsum(lay, dst, 16, 8, 0, 32, 64, 4, dtype, None) == EINVAL, dtype
    for dtype in (_lib.F32, _lib.F64, _lib.BF16, _lib.F16):
        assert rsum(None, dst, 16, 8, 0, 32, 64, 4, dtype, None) == EINVAL
        assert rsum(lay, None, 16, 8, 0, 32, 64, 4, dtype, None) == EINVAL
        assert rsum(lay, _lay(n_rows=12, B=3, len_add=4), 16, 8, 0, 32, 64, 4, dtype, None) == EINVAL
        assert rsum(lay, dst, 16, None, 0, 32, 64, 4, dtype, None) == EINVAL     # a table without its counts
        assert rsum(lay, dst, None, None, -1, 32, 64, 4, dtype, None) == EINVAL
        assert rsum(lay, dst, 16, 8, 0, None, 64, 4, dtype, None) == EINVAL
        assert rsum(lay, dst, 16, 8, 0, 32, None, 4, dtype, None) == EINVAL
        assert rsum(lay, dst, 16, 8, 0, 64, 64, 4, dtype, None) == EINVAL        # grad_src == grad_dst
        assert rsum(lay, dst, 16, 8, 0, 16, 64, 4, dtype, None) == EINVAL        # grad_src is the table
        assert rsum(lay, dst, 16, 8, 0, 32, 64, -1, dtype, None) == EINVAL
        assert rsum(lay, dst, 16, 8, 0, 32, 64, 0, dtype, None) == 0             # no columns
        assert rsum(_lay(B=0, n_rows=0), _lay(B=0, n_rows=0), None, None, 2, None, None, 4, dtype, None) == 0


def _bound(lay):
    if lay.kind == _lib.CAT:
        return lay.T_log if 0 < lay.T_log < lay.n_rows else lay.n_rows
    return lay.T if lay.kind == _lib.PACK else lay.T_phys


def _documented(lay):
    """include/rua.h: B * ceil(bound / 2 048) * 8 bytes when fewer than 1 024 sequences have a bound of at least 8 192."""
    if not lay.B < 1024 or not _bound(lay) >= 8192:
        return 0
    return lay.B * -(-_bound(lay) // 2048) * 8


def test_workspace_formula():
    ws = _lib.load().rua_repeat_ws_bytes
    cut = 0
    for kind in (_lib.CAT, _lib.LEFT, _lib.PACK, _lib.RIGHT):
        for B in (1, 2, 1023, 1024, 65536):
            for bound in (0, 1, 64, 2048, 8191, 8192, 8193, 40000, 200000):
                if kind == _lib.CAT:
                    lays = [_lay(kind, n_rows=bound, B=B, len_add=0), _lay(kind, n_rows=10 * bound + 1, B=B, len_add=0, T_log=bound)]
                elif kind == _lib.PACK:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T=bound)]
                else:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T_phys=bound, T_log=bound)]
                for lay in lays:
                    assert ws(lay) == _documented(lay), (kind, B, bound)
                    cut += ws(lay) > 0
    assert cut >= 30                                             # (the edges do exercise the cut side)
    assert ws(_lay(n_rows=40000, B=2, len_add=20000)) == 2 * 20 * 8          # by hand: ceil(40000 / 2048) = 20 blocks
    assert ws(_lay(n_rows=8191, B=1, len_add=8191)) == 0 and ws(_lay(n_rows=8192, B=1, len_add=8192)) == 4 * 8
    assert ws(None) == 0 and ws(_lay(n_rows=-1)) == 0 and ws(_lay(B=0, n_rows=0)) == 0
    assert ws(_lay(_lib.PACK, n_rows=40000, B=2, T=20000, boff=None)) == 0   # PACK without boff: not a layout


def test_host_plan_under_host_sanitizers(tmp_path):
    """rua_repeat_plan.h is plain host C++: tests/c/repeat_plan_host.cpp includes it (and rua_seg_plan.h) alone and walks
    the plan's form, grid and workspace and the grid of the move / run sum over a grid of (kind, B, bound, row width)
    under ASan + UBSan, as its own process; it fails on a report and on a plan that could not be launched as computed."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'repeat_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'repeat_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]


def test_the_yardstick_is_the_definition():
    """The yardstick checks ITSELF against a plain Python loop.  This test touches nothing of the library and passes
    without the operator: it is no coverage of repeat_interleave, only of what the GPU tests compare against."""
    g = torch.Generator().manual_seed(7)
    lens = torch.tensor([0, 1, 4, 0, 7])
    for data in (torch.randn(12, 3, generator=g), torch.arange(12), torch.randn(12, 2, 2, generator=g).bfloat16()):
        if data.is_floating_point():
            data.view(-1)[3] = float('nan')
        counts = torch.randint(0, 4, (12,), generator=g)
        counts[1], counts[4], counts[11] = 0, 0, 0                # leading and trailing zeros
        seqs, cs = split(data, lens), split(counts, lens)
        fast, slow = repeat(seqs, cs), repeat_by_loop(seqs, cs)
        assert len(fast) == len(slow) == 5
        for a, b in zip(fast, slow):
            assert same_bits(a, b)
        out, new = repeat_cat(data, counts, lens)
        assert new.dtype == torch.int64 and new.tolist() == [int(c.sum()) for c in cs]
        assert same_bits(out, torch.repeat_interleave(data, counts, dim=0))
        assert same_bits(repeat_cat(data, torch.ones(12, dtype=torch.long), lens)[0], data)
        assert repeat_cat(data, torch.zeros(12, dtype=torch.long), lens)[0].shape == (0,) + tuple(data.shape[1:])
        left, right = padded(fast, data), padded(fast, data, right=True)
        T = int(new.max())
        for b, s in enumerate(fast):
            n = s.shape[0]
            assert same_bits(left[b, :n], s) and same_bits(right[b, T - n:], s)
            assert not bool(left[b, n:].any()) and not bool(right[b, :T - n].any())
